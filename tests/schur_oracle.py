"""The value rule of csx_schur_factor / csx_schur_host, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

On the FULL pattern Lf of chol(P A P') (ldl_oracle.pattern: the restated cs_schol and cs_ereach), in plain Python floats, every
multiply, subtract and divide rounded on its own:

    columns j < n1: ldl_oracle.ldl's loop (the LDL' rule), stopped after n1 columns
    columns j >= n1:
        acc[r] = C(r, j) for r >= j (0.0 where nothing is stored)
        for every k < n1 with L(j,k) in the pattern, k ascending:
            w = L(j,k) * d[k];  for the stored p of column k from the slot of L(j,k) on:  v = L.x[p] * w;  acc[L.i[p]] -= v
        S(r - n1, j - n1) = S(j - n1, r - n1) = acc[r]

unstopped=True and descending=True are two MISTAKES a kernel could make in the trailing columns -- the updates of the columns
k >= n1 taken too (with the pivot 1.0 that Lp's unit columns stand for), and the updates from the last k to the first -- kept here
so that the tests can show that neither gives the right bytes.  vectorised=True applies one update (one k) of a trailing column
with numpy's elementwise multiply and subtract: the same IEEE operations on the same operands (the rows of one update are
distinct), for the dense-border cases whose S has up to a million entries; the CPU test holds it to the plain loop elsewhere.

condense_list / expand_list: the solves of a list in the reference's order (cs_ipvec, cs_lsolve, the division; cs_ltsolve,
cs_pvec), restated in plain Python on Lp."""
import math

import numpy as np

import ldl_oracle as LO


def schur(n, p, i, x, pinv, Lp, Li, n1, tau=0.0, unstopped=False, descending=False, vectorised=False):
    """(Lpx, d, S as an ns x ns array, (positive, negative, perturbed, breakdown column or -1))"""
    W = LO.scatter(n, p, i, x, pinv, Lp, Li)
    rows = [[] for _ in range(n)]                  # row j: (k, slot of L(j,k)), k ascending, the diagonal last
    for k in range(n):
        for q in range(Lp[k], Lp[k + 1]):
            rows[Li[q]].append((k, q))
    d = [0.0] * n1
    pos = neg = perturbed = 0
    broke = -1
    for j in range(n1):
        base, end = Lp[j], Lp[j + 1]
        where = {Li[q]: q for q in range(base, end)}
        for k, at in rows[j][:-1]:
            w = W[at] * d[k]
            for q in range(at, Lp[k + 1]):
                s = where[Li[q]]
                v = W[q] * w
                W[s] = W[s] - v
        dj = float(W[base])
        if tau > 0.0 and abs(dj) < tau:
            dj = math.copysign(tau, dj)
            perturbed += 1
        if (dj == 0.0 or not math.isfinite(dj)) and broke < 0:
            broke = j
        pos += dj > 0.0
        neg += dj < 0.0
        d[j] = dj
        W[base] = 1.0
        for q in range(base + 1, end):
            W[q] = LO._div(W[q], dj)
    ns = n - n1
    S = np.zeros((ns, ns))
    if vectorised:
        Wa, Lia = np.asarray(W, np.float64), np.asarray(Li, np.int64)
    for j in range(n1, n):
        ups = [(k, at) for k, at in rows[j][:-1] if unstopped or k < n1]
        if descending:
            ups = ups[::-1]
        if vectorised:
            acc = np.zeros(n)
            acc[Lia[Lp[j]:Lp[j + 1]]] = Wa[Lp[j]:Lp[j + 1]]
            with np.errstate(all="ignore"):
                for k, at in ups:
                    w = float(Wa[at]) * (d[k] if k < n1 else 1.0)
                    t = Lia[at:Lp[k + 1]]
                    v = Wa[at:Lp[k + 1]] * w
                    acc[t] = acc[t] - v
        else:
            acc = [0.0] * n
            for q in range(Lp[j], Lp[j + 1]):
                acc[Li[q]] = W[q]
            for k, at in ups:
                w = W[at] * (d[k] if k < n1 else 1.0)
                for q in range(at, Lp[k + 1]):
                    v = W[q] * w
                    acc[Li[q]] = acc[Li[q]] - v
        for r in range(j, n):
            S[r - n1, j - n1] = S[j - n1, r - n1] = acc[r]
    Lpx = [float(v) for v in W[:Lp[n1]]] + [1.0] * ns
    return Lpx, d, S, (pos, neg, perturbed, broke)


def lp_pattern(Lp, Li, n, n1):
    """(p, i) of the output Lp: the interior columns of the full pattern, then one diagonal entry per kept column"""
    head = Lp[n1]
    return list(Lp[:n1 + 1]) + [head + t for t in range(1, n - n1 + 1)], list(Li[:head]) + list(range(n1, n))


def condense_list(n, n1, pinv, p, i, x, d, b):
    """state = [inv(D1) inv(L11) b1; g] as a list: cs_ipvec(pinv), cs_lsolve(Lp) in the reference's column order, the division"""
    y = [0.0] * n
    for k in range(n):
        y[pinv[k]] = float(b[k])
    for j in range(n):
        y[j] = y[j] / x[p[j]]
        for q in range(p[j] + 1, p[j + 1]):
            y[i[q]] = y[i[q]] - x[q] * y[j]
    for j in range(n1):
        y[j] = LO._div(y[j], d[j])
    return y


def expand_list(n, n1, pinv, p, i, x, state, x2):
    """x in A's numbering: rows >= n1 of state replaced by x2, cs_ltsolve(Lp) in the reference's order, cs_pvec(pinv)"""
    y = [float(v) for v in state[:n1]] + [float(v) for v in x2]
    for j in range(n - 1, -1, -1):
        for q in range(p[j] + 1, p[j + 1]):
            y[j] = y[j] - x[q] * y[i[q]]
        y[j] = y[j] / x[p[j]]
    return [y[pinv[k]] for k in range(n)]


# ---- the shared reference of the CPU and GPU tests: computed once per (case, value set), never changed -------------------------

_CACHE = {}


def perm_of(sc):
    """the product's own order (host code): the interior first -- ascending or by its nested dissection -- then keep"""
    key = ("perm", sc.name)
    if key not in _CACHE:
        import csparse as cs
        perm = cs._schur_order(sc.matrix(cs), sc.keep, sc.order).tolist()
        assert sorted(perm) == list(range(sc.n)) and perm[sc.n1:] == sc.keep
        if sc.order == 0:
            assert perm[:sc.n1] == sorted(perm[:sc.n1])
        _CACHE[key] = perm
    return _CACHE[key]


def pinv_of(sc):
    key = ("pinv", sc.name)
    if key not in _CACHE:
        pinv = [0] * sc.n
        for k, v in enumerate(perm_of(sc)):
            pinv[v] = k
        _CACHE[key] = pinv
    return _CACHE[key]


def first_column(sc):
    """the interior column of A that is eliminated first"""
    return perm_of(sc)[0]


def pattern_of(sc):
    """(Lfp, Lfi, parent) of the full pattern"""
    key = ("pattern", sc.name)
    if key not in _CACHE:
        import csparse_oracle as O
        _CACHE[key] = LO.pattern(O, sc.n, sc.case.p, sc.case.i, pinv_of(sc))
    return _CACHE[key]


def host(sc, x, tau=0.0, n1=None, pinv="own"):
    """csx_schur_host on the case's full pattern with the values x: (status, Lpx, d, S, info)"""
    import _csx
    lib = _csx.load()
    Lp, Li, _ = pattern_of(sc)
    n = sc.n
    n1 = sc.n1 if n1 is None else n1
    pinv = pinv_of(sc) if pinv == "own" else pinv
    ns = max(n - n1, 0)
    Lpx, d, S = np.zeros(max(Lp[min(max(n1, 0), n)] + ns, 1)), np.zeros(max(n1, 1)), np.zeros(max(ns * ns, 1))
    info = (_csx.C.c_int64 * 4)()
    pv = None if pinv is None else _csx.i32(pinv)
    st = lib.csx_schur_host(n, _csx.pi(sc.case.p), _csx.pi(sc.case.i), _csx.pd(_csx.f64(x)), _csx.pi(pv), _csx.pi(_csx.i32(Lp)),
                            _csx.pi(_csx.i32(Li)), n1, float(tau), _csx.pd(Lpx), _csx.pd(d), _csx.pd(S), info)
    return st, Lpx[:Lp[min(max(n1, 0), n)] + ns], d[:max(n1, 0)], S[:ns * ns].reshape(ns, ns), tuple(int(v) for v in info)


def reference(sc, which):
    """the host rule's (Lpx, d, S, info) of value set `which` ("A", 0, 1, "kept-zero")"""
    key = ("ref", sc.name, which)
    if key not in _CACHE:
        x = sc.kept_zero() if which == "kept-zero" else sc.values(which)
        st, Lpx, d, S, info = host(sc, x)
        assert st == 0
        _CACHE[key] = (Lpx, d, S, info)
    return _CACHE[key]
