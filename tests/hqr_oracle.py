"""The symbolic step and the value rule of csx_hqr_factor / csx_hqr_host, CPU side -- TEST INFRASTRUCTURE, NOT
PRODUCT.  Plain Python floats: every multiply, add, subtract, divide and square root rounded on its own.

symbolic(): the loop of csx_qr_host with the values left out -- V.p, V.i (the diagonal first, then the rows in the order the
loop finds them) and R.p, R.i (the order the reflections are applied in, the diagonal last).

hqr(): for every column k ascending
    work = +0.0; A(:, q[k]) scattered at pinv[row], of duplicates the last stored
    for every c = R.i[t] before the diagonal, in stored order:
        part[l] = +0.0 (l = 0..63);  part[(p - V.p[c]) % 64] += V.x[p] * work[V.i[p]] over the column, ascending p
        for s = 32, 16, 8, 4, 2, 1:  part[l] = part[l] + part[l + s] for l < s
        tau = part[0] * beta[c];  work[V.i[p]] = work[V.i[p]] - V.x[p] * tau;  R.x[t] = work[c]
    V.x[p] = work[V.i[p]];  tail2 = the same 64 sums and tree over V.x[p]^2 after the head;  cs_house on (head, tail2)

sequential=True and fused=True are two MISTAKES a kernel could make -- the dot product summed entry by entry as the reference
does, and the update's product fused into the subtraction (exact rational arithmetic, one rounding) -- kept here so that the
tests can show that neither gives the right bytes."""
import math
from fractions import Fraction

import numpy as np


def symbolic(S):
    """(Vp, Vi, Rp, Ri) as lists, from the analysis S of tests/hqr_cases.py"""
    n, m2 = S.n, S.m2
    Ap, Ai, parent, pinv, leftmost = S.p.tolist(), S.i.tolist(), S.parent.tolist(), S.pinv.tolist(), S.leftmost.tolist()
    stamp = [-1] * m2
    Vp, Vi, Rp, Ri = [], [], [], []
    for k in range(n):
        Rp.append(len(Ri))
        Vp.append(len(Vi))
        stamp[k] = k
        Vi.append(k)
        order = []
        col = k if S.q is None else int(S.q[k])
        for p in range(Ap[col], Ap[col + 1]):
            path = []
            c = leftmost[Ai[p]]
            while stamp[c] != k:
                path.append(c)
                stamp[c] = k
                c = parent[c]
            order = path + order                 # later paths in front of earlier ones, each root-ward
            r = pinv[Ai[p]]
            if r > k and stamp[r] < k:
                Vi.append(r)
                stamp[r] = k
        for c in order:
            Ri.append(c)
            if parent[c] == k:
                for p in range(Vp[c], Vp[c + 1]):
                    r = Vi[p]
                    if stamp[r] < k:
                        stamp[r] = k
                        Vi.append(r)
        Ri.append(k)
    Rp.append(len(Ri))
    Vp.append(len(Vi))
    return Vp, Vi, Rp, Ri


def _tree(part):
    s = 32
    while s >= 1:
        for l in range(s):
            part[l] = part[l] + part[l + s]
        s >>= 1
    return part[0]


def house(head, tail2):
    """(s, new head, beta): cs_house statement for statement"""
    if tail2 == 0.0:
        return abs(head), 1.0, (2.0 if head <= 0.0 else 0.0)
    s = math.sqrt(head * head + tail2)
    v0 = head - s if head <= 0.0 else -tail2 / (head + s)
    return s, v0, -1.0 / (s * v0)


def hqr(S, x, pattern, sequential=False, fused=False):
    """(Vx, Rx, beta) as float64 arrays; x: the values in the storage order of the factored matrix"""
    Vp, Vi, Rp, Ri = pattern
    n = S.n
    Ap, Ai, pinv = S.p.tolist(), S.i.tolist(), S.pinv.tolist()
    x = [float(v) for v in x]
    Vx, Rx, beta = [0.0] * Vp[n], [0.0] * Rp[n], [0.0] * n
    work = [0.0] * S.m2
    for k in range(n):
        col = k if S.q is None else int(S.q[k])
        for p in range(Ap[col], Ap[col + 1]):
            work[pinv[Ai[p]]] = x[p]
        for t in range(Rp[k], Rp[k + 1] - 1):
            c = Ri[t]
            lo, hi = Vp[c], Vp[c + 1]
            if sequential:
                dot = 0.0
                for p in range(lo, hi):
                    dot = dot + Vx[p] * work[Vi[p]]
            else:
                part = [0.0] * 64
                for p in range(lo, hi):
                    l = (p - lo) & 63
                    part[l] = part[l] + Vx[p] * work[Vi[p]]
                dot = _tree(part)
            tau = dot * beta[c]
            for p in range(lo, hi):
                r = Vi[p]
                if fused:
                    work[r] = float(Fraction(work[r]) - Fraction(Vx[p]) * Fraction(tau))
                else:
                    prod = Vx[p] * tau
                    work[r] = work[r] - prod
            Rx[t] = work[c]
            work[c] = 0.0
        lo, hi = Vp[k], Vp[k + 1]
        for p in range(lo, hi):
            Vx[p] = work[Vi[p]]
            work[Vi[p]] = 0.0
        part = [0.0] * 64
        for p in range(lo + 1, hi):
            l = (p - lo - 1) & 63
            part[l] = part[l] + Vx[p] * Vx[p]
        Rx[Rp[k + 1] - 1], Vx[lo], beta[k] = house(Vx[lo], _tree(part))
    return np.asarray(Vx, np.float64), np.asarray(Rx, np.float64), np.asarray(beta, np.float64)


# ---- the host functions on a case's analysis, and the shared reference: computed once per (case, value set), never changed -----

_CACHE = {}


def pattern_of(case):
    key = ("pattern", case.name)
    if key not in _CACHE:
        _CACHE[key] = symbolic(case.analysis)
    return _CACHE[key]


def factored_values(case, x):
    """the values x (A's storage order) in the storage order of the factored matrix"""
    return np.ascontiguousarray(np.asarray(x, np.float64)[case.analysis.perm])


def host(case, x, fn="csx_hqr_host", S=None):
    """fn (csx_hqr_host or csx_qr_host) on the analysis S (default the case's) with the values x in A's storage order:
    (status, Vp, Vi, Vx, Rp, Ri, Rx, beta)"""
    import _csx
    S = case.analysis if S is None else S
    n = S.n
    vcap, rcap = max(S.vnz, 1), max(S.rnz, 1)
    Vp, Rp = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    Vi, Ri = np.zeros(vcap, np.int32), np.zeros(rcap, np.int32)
    Vx, Rx, beta = np.zeros(vcap), np.zeros(rcap), np.zeros(max(n, 1))
    fx = np.ascontiguousarray(np.asarray(x, np.float64)[S.perm]) if len(S.perm) else np.zeros(1)
    fi = S.i if len(S.i) else np.zeros(1, np.int32)
    st = getattr(_csx.load(), fn)(S.m, n, S.m2, _csx.pi(S.p), _csx.pi(fi), _csx.pd(fx), _csx.pi(S.q), _csx.pi(S.parent),
                                 _csx.pi(S.pinv), _csx.pi(S.leftmost), vcap, rcap, _csx.pi(Vp), _csx.pi(Vi), _csx.pd(Vx),
                                 _csx.pi(Rp), _csx.pi(Ri), _csx.pd(Rx), _csx.pd(beta))
    return st, Vp, Vi[:Vp[n]], Vx[:Vp[n]], Rp, Ri[:Rp[n]], Rx[:Rp[n]], beta[:n]


def reference(case, which):
    """csx_hqr_host's (Vp, Vi, Vx, Rp, Ri, Rx, beta) of value set `which` ("A", 0, 1)"""
    key = ("ref", case.name, which)
    if key not in _CACHE:
        out = host(case, case.values(which))
        assert out[0] == 0
        _CACHE[key] = out[1:]
    return _CACHE[key]


# ---- solves on host factors: the existing plain-C reflection loop and triangular solves in plain Python -----------------------

def apply_q(S, Vp, Vi, Vx, beta, x, transpose):
    import _csx
    x = np.ascontiguousarray(x, np.float64).copy()
    assert _csx.load().csx_qr_apply_host(S.n, _csx.pi(Vp), _csx.pi(Vi if len(Vi) else np.zeros(1, np.int32)),
                                         _csx.pd(Vx if len(Vx) else np.zeros(1)), _csx.pd(beta if len(beta) else np.zeros(1)),
                                         1 if transpose else 0, _csx.pd(x)) == 0
    return x


def usolve(n, Rp, Ri, Rx, x):
    """cs_usolve: the diagonal last in every column"""
    x = [float(v) for v in x]
    for j in range(n - 1, -1, -1):
        x[j] = x[j] / Rx[Rp[j + 1] - 1]
        for p in range(Rp[j], Rp[j + 1] - 1):
            x[Ri[p]] = x[Ri[p]] - Rx[p] * x[j]
    return x


def utsolve(n, Rp, Ri, Rx, x):
    """cs_utsolve"""
    x = [float(v) for v in x]
    for j in range(n):
        for p in range(Rp[j], Rp[j + 1] - 1):
            x[j] = x[j] - Rx[p] * x[Ri[p]]
        x[j] = x[j] / Rx[Rp[j + 1] - 1]
    return x


def solve(S, factors, b, second=False):
    """cs_qrsol's first sequence (least squares: b of S.m entries, x of S.n) or its second (b of S.n entries, x of S.m) on the
    factors (Vp, Vi, Vx, Rp, Ri, Rx, beta) of the factored matrix"""
    Vp, Vi, Vx, Rp, Ri, Rx, beta = factors
    m, n = S.m, S.n
    q = np.arange(n) if S.q is None else np.asarray(S.q)
    x = np.zeros(S.m2)
    rp, ri, rx = Rp.tolist(), Ri.tolist(), Rx.tolist()
    if not second:
        x[S.pinv[:m]] = np.asarray(b, np.float64)[:m]
        x = apply_q(S, Vp, Vi, Vx, beta, x, True)
        x[:n] = usolve(n, rp, ri, rx, x[:n])
        out = np.zeros(n)
        out[q] = x[:n]
        return out
    x[:n] = np.asarray(b, np.float64)[q]
    x[:n] = utsolve(n, rp, ri, rx, x[:n])
    x = apply_q(S, Vp, Vi, Vx, beta, x, False)
    return x[S.pinv[:m]]


def omega(case, xs, b, trans=False, values=None):
    """(R, omega) of one square system by the residual's restatement"""
    import residual_oracle as RO
    R, w, _ = RO.residual(case.m, case.n, case.p, case.i, case.x if values is None else values, 1, trans, xs, b)
    return np.asarray(R), w[0]


def refined(case, factors, b, steps, trans=False):
    """[omega0, omega1, ...] of plain iterative refinement on a square case"""
    S = case.analysis
    x = solve(S, factors, b, trans)
    R, w = omega(case, x, b, trans)
    out = [w]
    for _ in range(steps):
        x = x + solve(S, factors, R, trans)
        R, w = omega(case, x, b, trans)
        out.append(w)
    return out
