"""The value rule of csx_slu_factor / csx_slu_host, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

L U = C = P A1 P', A1 = A(prow, :), on the Cholesky pattern of the pattern of A1 + A1' under pinv (the restated cs_schol and
cs_ereach, ldl_oracle.pattern), in plain Python floats: every multiply, subtract and divide rounded on its own.  Lx is unit lower
L; Ux is Ut: column k = row k of U, the pivot first.

    for every column j ascending:
        accL[r] = C(r, j), accU[r] = C(j, r) on the rows of column j of the pattern
        for every column k < j with (j,k) in the pattern, k ascending:
            l = L(j,k);  u = Ut(j,k);  for the stored p of column k from the slot of row j on, r = L.i[p]:
                a = L.x[p] * u;  accL[r] -= a;  b = Ut.x[p] * l;  accU[r] -= b
        d = accU[j];  |d| < tau (tau > 0): d = copysign(tau, d), counted;  d == 0 or not finite: breakdown
        Ut(j,j) = d;  Ut(r,j) = accU[r];  L(j,j) = 1.0;  L(r,j) = accL[r] / d

descending=True and fused=True are two MISTAKES a kernel could make -- the updates of a column from the last k to the first, and
the subtraction fused with the product (exact rational arithmetic, one rounding) -- kept here so that the tests can show that
neither gives the right bytes.  vectorised=True applies one update (one k) with numpy's elementwise multiply and subtract: the
same IEEE operations on the same operands (the rows of one update are distinct), for the two cases whose factor is a dense
triangle of 130 000 entries; the CPU test holds it to the plain loop on other cases."""
import math
from fractions import Fraction

import numpy as np

from ldl_oracle import _div, pattern


def prinv_of(case):
    """row i of A is row prinv[i] of A1 = A(prow, :); None without a matching"""
    if case.prow is None:
        return None
    prinv = np.empty(case.n, np.int64)
    prinv[case.prow] = np.arange(case.n)
    return prinv


def symmetrised(O, case):
    """B = A1 + A1' as the product forms it (cs_permute, cs_transpose, cs_add on the pattern), a `cs` of the restated module"""
    A = O.cs_spalloc(case.n, case.n, max(len(case.i), 1), False, False)
    A.p, A.i, A.x = case.p.tolist(), case.i.tolist() or [0], None
    prinv = prinv_of(case)
    A1 = A if prinv is None else O.cs_permute(A, prinv.tolist(), None, False)
    return O.cs_add(A1, O.cs_transpose(A1, False), 1.0, 1.0)


def scatter(case, x, pinv, Lp, Li):
    """(Lx, Ux) with C in its slots, 0.0 elsewhere"""
    n, prinv = case.n, prinv_of(case)
    slot = [{Li[q]: q for q in range(Lp[j], Lp[j + 1])} for j in range(n)]
    Lx, Ux = [0.0] * Lp[n], [0.0] * Lp[n]
    for q in range(len(case.i)):
        i1 = int(case.i[q]) if prinv is None else int(prinv[case.i[q]])
        j = int(case.cols[q])
        i2, j2 = (i1, j) if pinv is None else (int(pinv[i1]), int(pinv[j]))
        if i2 >= j2:
            Lx[slot[j2][i2]] = float(x[q])
        if i2 <= j2:
            Ux[slot[i2][j2]] = float(x[q])
    return Lx, Ux


def slu(case, x, pinv, Lp, Li, tau=0.0, descending=False, fused=False, vectorised=False):
    """(Lx, Ux, (positive, negative, perturbed, breakdown column or -1)); after a breakdown Lx and Ux mean nothing"""
    n = case.n
    Lx, Ux = scatter(case, x, pinv, Lp, Li)
    rows = [[] for _ in range(n)]                  # row j: (k, slot of (j,k)), k ascending, the diagonal last
    for k in range(n):
        for q in range(Lp[k], Lp[k + 1]):
            rows[Li[q]].append((k, q))
    pos = neg = perturbed = 0
    broke = -1
    if vectorised:
        Lx, Ux, Lia, where = np.asarray(Lx, np.float64), np.asarray(Ux, np.float64), np.asarray(Li, np.int64), np.zeros(n, np.int64)
    for j in range(n):
        base, end = Lp[j], Lp[j + 1]
        ups = rows[j][:-1]
        if descending:
            ups = ups[::-1]
        if vectorised:
            where[Lia[base:end]] = np.arange(base, end)
            with np.errstate(all="ignore"):
                for k, at in ups:
                    l, u = float(Lx[at]), float(Ux[at])
                    t = where[Lia[at:Lp[k + 1]]]
                    a, b = Lx[at:Lp[k + 1]] * u, Ux[at:Lp[k + 1]] * l
                    Lx[t] = Lx[t] - a
                    Ux[t] = Ux[t] - b
        else:
            where = {Li[q]: q for q in range(base, end)}
            for k, at in ups:
                l, u = Lx[at], Ux[at]
                for q in range(at, Lp[k + 1]):
                    s = where[Li[q]]
                    if fused:
                        Lx[s] = float(Fraction(Lx[s]) - Fraction(Lx[q]) * Fraction(u))
                        Ux[s] = float(Fraction(Ux[s]) - Fraction(Ux[q]) * Fraction(l))
                    else:
                        a = Lx[q] * u
                        Lx[s] = Lx[s] - a
                        b = Ux[q] * l
                        Ux[s] = Ux[s] - b
        dj = float(Ux[base])
        if tau > 0.0 and abs(dj) < tau:
            dj = math.copysign(tau, dj)
            perturbed += 1
        if (dj == 0.0 or not math.isfinite(dj)) and broke < 0:
            broke = j
        pos += dj > 0.0
        neg += dj < 0.0
        Ux[base] = dj
        Lx[base] = 1.0
        if vectorised:
            with np.errstate(all="ignore"):
                Lx[base + 1:end] = Lx[base + 1:end] / dj
        else:
            for q in range(base + 1, end):
                Lx[q] = _div(Lx[q], dj)
    return [float(v) for v in Lx], [float(v) for v in Ux], (pos, neg, perturbed, broke)


# ---- the shared reference of the CPU and GPU tests: computed once per (case, value set), never changed -------------------------

_CACHE = {}


def pinv_of(case):
    """None in natural order, else the inverse of the product's own nested dissection of B = A1 + A1' (host code)"""
    if case.order == 0:
        return None
    key = ("pinv", case.name)
    if key not in _CACHE:
        import csparse as cs
        import csparse_oracle as O
        B0 = symmetrised(O, case)
        B = cs.cs_spalloc(case.n, case.n, max(B0.p[case.n], 1), False, False)
        B.p, B.i, B.x = list(B0.p), list(B0.i[:B0.p[case.n]]) or [0], None
        perm = cs.cs_amd(1, B)
        assert sorted(perm) == list(range(case.n))
        pinv = [0] * case.n
        for k, v in enumerate(perm):
            pinv[v] = k
        _CACHE[key] = pinv
    return _CACHE[key]


def first_pivot(case):
    """(row, column) of the entry of A that is the pivot of the column eliminated first"""
    pinv = pinv_of(case)
    j0 = 0 if pinv is None else pinv.index(0)
    return (j0 if case.prow is None else int(case.prow[j0])), j0


def pattern_of(case):
    """(Lp, Li, parent) of the Cholesky pattern of B under pinv"""
    key = ("pattern", case.name)
    if key not in _CACHE:
        import csparse_oracle as O
        B = symmetrised(O, case)
        nb = B.p[case.n]
        keep = [(r, c) for c in range(case.n) for r in B.i[B.p[c]:B.p[c + 1]] if r <= c]     # its upper triangle, as cs_schol reads it
        up, ui = [0] * (case.n + 1), []
        for r, c in keep:
            up[c + 1] += 1
            ui.append(r)
        assert nb >= len(ui)
        _CACHE[key] = pattern(O, case.n, np.cumsum(up).tolist(), ui, pinv_of(case))
    return _CACHE[key]


def norm1(case, x):
    """|A|_1 as csx_norm1 computes it: the largest column sum of |x| over the stored entries, each sum in storage order"""
    best = 0.0
    for j in range(case.n):
        s = 0.0
        for q in range(int(case.p[j]), int(case.p[j + 1])):
            s = s + abs(float(x[q]))
        if s > best or s != s:
            best = s
    return best


def tau_of(case, x, perturb=None):
    perturb = case.perturb if perturb is None else perturb
    return 0.0 if perturb == 0.0 else perturb * norm1(case, x)


def host(case, x, tau):
    """csx_slu_host on the case's pattern with the values x: (status, Lx, Ux, (positive, negative, perturbed, breakdown))"""
    import _csx
    lib = _csx.load()
    Lp, Li, _ = pattern_of(case)
    n, pinv = case.n, pinv_of(case)
    Lx, Ux, info = np.zeros(Lp[n]), np.zeros(Lp[n]), (_csx.C.c_int64 * 4)()
    pv = None if pinv is None else _csx.i32(pinv)
    st = lib.csx_slu_host(n, _csx.pi(case.p), _csx.pi(case.i), _csx.pd(_csx.f64(x)), _csx.pi(case.prow), _csx.pi(pv),
                          _csx.pi(_csx.i32(Lp)), _csx.pi(_csx.i32(Li)), float(tau), _csx.pd(Lx), _csx.pd(Ux), info)
    return st, Lx, Ux, tuple(int(v) for v in info)


def reference(case, which):
    """the host rule's (Lx, Ux, info) of value set `which` ("A", 0, 1) under the case's own perturbation"""
    key = ("ref", case.name, which)
    if key not in _CACHE:
        x = case.values(which)
        st, Lx, Ux, info = host(case, x, tau_of(case, x))
        assert st == 0
        _CACHE[key] = (Lx, Ux, info)
    return _CACHE[key]


# ---- solves and refinement on the host factors (plain-C triangular solves, the residual's restatement) -----------------------

def solve(case, Lx, Ux, b):
    """A^-1 b: x(pinv o prinv) = b, L \\ x, Ut' \\ x, x = x(pinv)"""
    import c_oracle as CO
    Lp, Li, _ = pattern_of(case)
    n, pinv, prinv = case.n, pinv_of(case), prinv_of(case)
    comb = prinv if pinv is None else (np.asarray(pinv) if prinv is None else np.asarray(pinv)[prinv])
    x = np.asarray(b, np.float64).copy()
    if comb is not None:
        y = np.empty(n)
        y[comb] = x
        x = y
    x = CO.lsolve(n, Lp, Li, Lx, x)
    x = CO.ltsolve(n, Lp, Li, Ux, x)
    return x if pinv is None else x[np.asarray(pinv)]


def omega(case, xs, b, values=None):
    """(R, omega) of one system by the residual's restatement"""
    import residual_oracle as RO
    R, w, _ = RO.residual(case.n, case.n, case.p, case.i, case.x if values is None else values, 1, False, xs, b)
    return np.asarray(R), w[0]


def refined(case, Lx, Ux, b, steps):
    """[omega0, omega1, ...] of plain iterative refinement"""
    x = solve(case, Lx, Ux, b)
    R, w = omega(case, x, b)
    out = [w]
    for _ in range(steps):
        x = x + solve(case, Lx, Ux, R)
        R, w = omega(case, x, b)
        out.append(w)
    return out
