"""The value rule of csx_ldl_factor / csx_ldl_host, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

L D L' = C, C = upper(P A P') as cs_chol reads it (stored entries with row <= column, of duplicates the last, lower entries
ignored), on the pattern that the restated cs_schol and cs_ereach give (pattern()), in plain Python floats: every multiply,
subtract and divide rounded on its own.

    for every column j ascending:
        acc[r] = C(r, j) on the rows of column j of L
        for every column k < j with L(j,k) in the pattern, k ascending:
            w = L(j,k) * d[k];  for the stored p of column k from the slot of L(j,k) on:  v = L.x[p] * w;  acc[L.i[p]] -= v
        d[j] = acc[j];  |d[j]| < tau (tau > 0): d[j] = copysign(tau, d[j]), counted;  d[j] == 0 or not finite: breakdown
        L(j,j) = 1.0;  L(r,j) = acc[r] / d[j]

descending=True and fused=True are two MISTAKES a kernel could make -- the updates of a column from the last k to the first, and
the subtraction fused with the product (exact rational arithmetic, one rounding) -- kept here so that the tests can show that
neither gives the right bytes.  vectorised=True applies one update (one k) with numpy's elementwise multiply and subtract:
the same IEEE operations on the same operands (the rows of one update are distinct), for the two cases whose factor is a dense
triangle of 130 000 entries; the CPU test holds it to the plain loop on every other case."""
import math
from fractions import Fraction

import numpy as np


def pattern(O, n, p, i, pinv=None):
    """(Lp, Li) of chol(P A P'): the restated cs_schol for the counts, cs_ereach for row k's columns; rows ascending, the
    diagonal first"""
    A = O.cs_spalloc(n, n, max(len(i), 1), False, False)
    A.p, A.i, A.x = [int(v) for v in p], [int(v) for v in i] or [0], None
    C = A if pinv is None else O.cs_symperm(A, [int(v) for v in pinv], False)
    S = O.cs_schol(0, C)
    cols = [[j] for j in range(n)]
    s, w = [0] * n, [0] * n
    for k in range(n):
        top = O.cs_ereach(C, k, S.parent, s, 0, w)
        for t in range(top, n):
            cols[s[t]].append(k)
    Lp = [0]
    for j in range(n):
        assert cols[j] == sorted(cols[j]) and len(cols[j]) == S.cp[j + 1] - S.cp[j]
        Lp.append(Lp[-1] + len(cols[j]))
    return Lp, [r for c in cols for r in c], S.parent


def _div(a, b):
    """a / b as IEEE 754 has it (Python raises for b == 0)"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def scatter(n, p, i, x, pinv, Lp, Li):
    """L.x with C in its slots, 0.0 elsewhere"""
    slot = [{Li[q]: q for q in range(Lp[j], Lp[j + 1])} for j in range(n)]
    Lx = [0.0] * Lp[n]
    for j in range(n):
        j2 = j if pinv is None else int(pinv[j])
        for q in range(int(p[j]), int(p[j + 1])):
            r = int(i[q])
            if r > j:
                continue
            r2 = r if pinv is None else int(pinv[r])
            Lx[slot[min(r2, j2)][max(r2, j2)]] = float(x[q])
    return Lx


def ldl(n, p, i, x, pinv, Lp, Li, tau=0.0, descending=False, fused=False, vectorised=False):
    """(Lx, d, (positive, negative, perturbed, breakdown column or -1)); after a breakdown Lx and d mean nothing"""
    Lx = scatter(n, p, i, x, pinv, Lp, Li)
    rows = [[] for _ in range(n)]                  # row j: (k, slot of L(j,k)), k ascending, the diagonal last
    for k in range(n):
        for q in range(Lp[k], Lp[k + 1]):
            rows[Li[q]].append((k, q))
    d = [0.0] * n
    pos = neg = perturbed = 0
    broke = -1
    if vectorised:
        Lx, Lia, where = np.asarray(Lx, np.float64), np.asarray(Li, np.int64), np.zeros(n, np.int64)
    for j in range(n):
        base, end = Lp[j], Lp[j + 1]
        ups = rows[j][:-1]
        if descending:
            ups = ups[::-1]
        if vectorised:
            where[Lia[base:end]] = np.arange(base, end)
            with np.errstate(all="ignore"):
                for k, at in ups:
                    w = float(Lx[at]) * d[k]
                    t = where[Lia[at:Lp[k + 1]]]
                    v = Lx[at:Lp[k + 1]] * w
                    Lx[t] = Lx[t] - v
        else:
            where = {Li[q]: q for q in range(base, end)}
            for k, at in ups:
                w = Lx[at] * d[k]
                for q in range(at, Lp[k + 1]):
                    s = where[Li[q]]
                    if fused:
                        Lx[s] = float(Fraction(Lx[s]) - Fraction(Lx[q]) * Fraction(w))
                    else:
                        v = Lx[q] * w
                        Lx[s] = Lx[s] - v
        dj = float(Lx[base])
        if tau > 0.0 and abs(dj) < tau:
            dj = math.copysign(tau, dj)
            perturbed += 1
        if (dj == 0.0 or not math.isfinite(dj)) and broke < 0:
            broke = j
        pos += dj > 0.0
        neg += dj < 0.0
        d[j] = dj
        Lx[base] = 1.0
        if vectorised:
            with np.errstate(all="ignore"):
                Lx[base + 1:end] = Lx[base + 1:end] / dj
        else:
            for q in range(base + 1, end):
                Lx[q] = _div(Lx[q], dj)
    return [float(v) for v in Lx], d, (pos, neg, perturbed, broke)


# ---- the shared reference of the CPU and GPU tests: computed once per (case, value set), never changed -------------------------

_CACHE = {}


def pinv_of(case):
    """None in natural order, else the inverse of the product's own nested dissection of the case's pattern (host code)"""
    if case.order == 0:
        return None
    key = ("pinv", case.name)
    if key not in _CACHE:
        import csparse as cs
        perm = cs.cs_amd(1, case.matrix(cs))
        assert sorted(perm) == list(range(case.n))
        pinv = [0] * case.n
        for k, v in enumerate(perm):
            pinv[v] = k
        _CACHE[key] = pinv
    return _CACHE[key]


def first_column(case):
    """the column of A that is eliminated first"""
    pinv = pinv_of(case)
    return 0 if pinv is None else pinv.index(0)


def pattern_of(case):
    key = ("pattern", case.name)
    if key not in _CACHE:
        import csparse_oracle as O
        _CACHE[key] = pattern(O, case.n, case.p, case.i, pinv_of(case))
    return _CACHE[key]


def tau_of(case, x, perturb=None):
    """perturb |S|_1 with the norm as csx_norm1_sym computes it"""
    import residual_sym_oracle as RSO
    perturb = case.perturb if perturb is None else perturb
    return 0.0 if perturb == 0.0 else perturb * RSO.norm1(case.n, case.p, case.i, x)


def host(case, x, tau):
    """csx_ldl_host on the case's pattern with the values x: (status, Lx, d, (positive, negative, perturbed, breakdown))"""
    import _csx
    lib = _csx.load()
    Lp, Li, _ = pattern_of(case)
    n, pinv = case.n, pinv_of(case)
    Lx, d, info = np.zeros(Lp[n]), np.zeros(n), (_csx.C.c_int64 * 4)()
    pv = None if pinv is None else _csx.i32(pinv)
    st = lib.csx_ldl_host(n, _csx.pi(case.p), _csx.pi(case.i), _csx.pd(_csx.f64(x)), _csx.pi(pv), _csx.pi(_csx.i32(Lp)),
                          _csx.pi(_csx.i32(Li)), float(tau), _csx.pd(Lx), _csx.pd(d), info)
    return st, Lx, d, tuple(int(v) for v in info)


def reference(case, which):
    """the host rule's (Lx, d, info) of value set `which` ("A", 0, 1) under the case's own perturbation"""
    key = ("ref", case.name, which)
    if key not in _CACHE:
        x = case.values(which)
        st, Lx, d, info = host(case, x, tau_of(case, x))
        assert st == 0
        _CACHE[key] = (Lx, d, info)
    return _CACHE[key]
