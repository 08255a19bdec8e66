"""The value rule of csx_pattern_outer restated in plain Python / numpy from the comment in include/csx.h (not from the C code), and
the pull-back of an assembly plan.  Python floats are IEEE doubles and every operation below is one rounded operation, so the
restatement gives the rule's bits.

Two mistakes are kept, to show that the cases of tests/outer_cases.py tell them from the rule:
    mistake="left_to_right"    the sum over the columns taken left to right in one partial sum
    mistake="diagonal_twice"   sym mode counting a diagonal entry at two places, like an entry above the diagonal"""
import numpy as np


def width(nrhs, lanes):
    """W = min(PO_LANES, smallest power of two >= nrhs)"""
    w = 1
    while w < nrhs and w < lanes:
        w *= 2
    return w


def entry(u_i, v_j, u_j, v_i, nrhs, lanes, two, mistake=None):
    """the sum of one entry before alpha: u_i, v_j the rows U[i, :], V[j, :]; two: the mirrored products U[j, c] V[i, c] follow"""
    W = 1 if mistake == "left_to_right" else width(nrhs, lanes)
    s = [0.0] * W
    for l in range(W):
        first = True
        for c in range(l, nrhs, W):
            t = float(u_i[c]) * float(v_j[c])
            s[l] = t if first else s[l] + t
            first = False
            if two:
                s[l] = s[l] + float(u_j[c]) * float(v_i[c])
    d = W // 2
    while d >= 1:
        for l in range(d):
            s[l] = s[l] + s[l + d]
        d //= 2
    return s[0]


def pattern_outer(m, n, p, i, U, V, nrhs, alpha=1.0, sym=False, lanes=16, mistake=None):
    """out[q] for every stored entry q of the m x n pattern (p, i); U m x nrhs, V n x nrhs"""
    U = np.asarray(U, np.float64).reshape(-1, nrhs) if m else np.zeros((0, nrhs))
    V = np.asarray(V, np.float64).reshape(-1, nrhs) if n else np.zeros((0, nrhs))
    out = np.zeros(int(p[n]), np.float64)
    for j in range(n):
        for q in range(int(p[j]), int(p[j + 1])):
            r = int(i[q])
            if sym and r > j:
                out[q] = 0.0
                continue
            two = sym and (r < j or (mistake == "diagonal_twice" and r == j))
            s = entry(U[r], V[j], U[j] if sym else None, V[r] if sym else None, nrhs, lanes, two, mistake)
            out[q] = float(alpha) * s
    return out


def pullback(sp, src, g):
    """gT[t] = g[slot of t] through the plan's slot pointers sp and grouped triplets src"""
    out = np.zeros(len(src), np.float64)
    for s in range(len(sp) - 1):
        for u in range(int(sp[s]), int(sp[s + 1])):
            out[int(src[u])] = g[s]
    return out
