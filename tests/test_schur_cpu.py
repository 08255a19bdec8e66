"""csx_schur_host (the value rule of csx_schur_factor on host arrays) against the Python restatement
(tests/schur_oracle.py), two deliberate mistakes that must give other bytes, csx_ldl_host for ns = 0, the componentwise backward
error of the partial factorisation in exact rational arithmetic, Haynsworth's inertia sum against the dense spectrum, S against
numpy's own Schur complement, kkt-zero without a perturbation, and the CSX_EINVAL / ValueError cases that need no device."""
from fractions import Fraction

import numpy as np
import pytest

import ldl_oracle as LO
import schur_cases as SC
import schur_oracle as SO
import tol

EPS = 2.0 ** -52


def _same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def _rule(sc, x, **kw):
    Lp, Li, _ = SO.pattern_of(sc)
    return SO.schur(sc.n, sc.case.p, sc.case.i, x, SO.pinv_of(sc), Lp, Li, sc.n1, 0.0, **kw)


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_rule_is_the_restatement(name):
    sc = SC.BY_NAME[name]
    for which in SC.VALUE_SETS + ("kept-zero",):
        if which == "kept-zero" and sc.ns == 0:
            continue
        x = sc.kept_zero() if which == "kept-zero" else sc.values(which)
        Lpx, d, S, info = SO.reference(sc, which)
        rx, rd, rS, rinfo = _rule(sc, x, vectorised=name in SC.BORDERS)
        assert info == rinfo and info[3] == -1, which
        assert info[0] + info[1] == sc.n1
        assert _same(Lpx, rx) and _same(d, rd) and _same(S, rS), which
        assert _same(S, S.T)
    if sc.n1:
        # the breaking value set: the same column reported, nothing said about the values
        bad = sc.case.breaking(SO.first_column(sc))
        st, _, _, _, info = SO.host(sc, bad)
        assert st == 0 and info[3] == 0
        assert _rule(sc, bad, vectorised=name in SC.BORDERS)[3][3] == 0


@pytest.mark.parametrize("name", [n for n in SC.NAMES if n not in SC.BORDERS])
def test_the_vectorised_restatement_is_the_plain_one(name):
    sc = SC.BY_NAME[name]
    a, b = _rule(sc, sc.case.A2[0]), _rule(sc, sc.case.A2[0], vectorised=True)
    assert a[3] == b[3] and _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[2], b[2])


@pytest.mark.parametrize("name", ["grid-line-0", "grid-line-1", "grid-cross-1"])
def test_unstopped_or_descending_updates_give_other_bytes(name):
    sc = SC.BY_NAME[name]
    _, _, S, _ = SO.reference(sc, "A")
    for mistake in ("unstopped", "descending"):
        rS = _rule(sc, sc.case.x, **{mistake: True})[2]
        assert not _same(S, rS), mistake
    rS = _rule(sc, sc.case.x, descending=True)[2]
    assert np.allclose(S, rS, rtol=1e-6, atol=1e-9)                    # (a mistake of rounding, not of arithmetic)


def test_border_batches_has_the_rows_it_names():
    """the row views of the four trailing columns, in ascending k: nothing; 9 interior columns; 7 interior columns and then a
    kept one; 8 interior columns and then kept ones -- what the update loop's fetches of eight are to meet (tests/schur_cases.py)"""
    sc = SC.BY_NAME["border-batches"]
    Lp, Li, _ = SO.pattern_of(sc)
    n1 = sc.n1
    assert SO.perm_of(sc) == list(range(sc.n)) and sc.ns == 4
    rows = [[k for k in range(j) if j in Li[Lp[k]:Lp[k + 1]]] for j in range(n1, sc.n)]
    interior = [[k for k in r if k < n1] for r in rows]
    assert [len(r) for r in interior] == [0, 9, 7, 8]
    assert [r[len(i):] for r, i in zip(rows, interior)] == [[], [], [n1], [n1, n1 + 2]]
    _, d, S, info = SO.reference(sc, "A")
    assert info[2:] == (0, -1) and np.all(d != 0.0)
    assert S[1, 0] == 0.0 and S[2, 0] != 0.0 and S[3, 0] != 0.0 and S[3, 2] == 0.0          # what the kept couplings leave in S


@pytest.mark.parametrize("name", ["one-keep-none", "grid-line-1"])
def test_nothing_kept_is_the_ldl_rule(name):
    """ns = 0 on the case's own full pattern and order: Lp.x and d are csx_ldl_host's"""
    import _csx
    sc = SC.BY_NAME[name]
    Lp, Li, _ = SO.pattern_of(sc)
    n, pinv = sc.n, SO.pinv_of(sc)
    for which in SC.VALUE_SETS:
        x = sc.values(which)
        st, Lpx, d, S, info = SO.host(sc, x, n1=n)
        assert st == 0 and S.size == 0
        Lx, dd, linfo = np.zeros(Lp[n]), np.zeros(n), (_csx.C.c_int64 * 4)()
        st = _csx.load().csx_ldl_host(n, _csx.pi(sc.case.p), _csx.pi(sc.case.i), _csx.pd(_csx.f64(x)), _csx.pi(_csx.i32(pinv)),
                                      _csx.pi(_csx.i32(Lp)), _csx.pi(_csx.i32(Li)), 0.0, _csx.pd(Lx), _csx.pd(dd), linfo)
        assert st == 0 and tuple(linfo) == info
        assert _same(Lpx, Lx) and _same(d, dd)


def _lower_entries(sc, x):
    pinv, c = SO.pinv_of(sc), sc.case
    out = {}
    for q in range(len(c.i)):
        r, k = int(c.i[q]), int(c.cols[q])
        if r <= k:
            r2, k2 = pinv[r], pinv[k]
            out[(max(r2, k2), min(r2, k2))] = float(x[q])
    return out


@pytest.mark.parametrize("name", ["grid-line-1", "kkt-sqd", "kkt-zero"])
def test_componentwise_backward_error_of_the_partial_factorisation(name):
    """|C - Lp blockdiag(D1, S) Lp'| <= (n + 1) 2^-52 |Lp| blockdiag(|D1|, |S|) |Lp'| entry by entry on the lower triangle, in
    exact rationals: an entry takes at most n1 updates of two roundings each (w, the product) plus as many subtractions -- the
    form of the LDL' check of tests/test_ldl_cpu.py, derived and not measured"""
    sc = SC.BY_NAME[name]
    Lfp, Lfi, _ = SO.pattern_of(sc)
    n, n1 = sc.n, sc.n1
    Lpx, d, S, _ = SO.reference(sc, "A")
    p, i = SO.lp_pattern(Lfp, Lfi, n, n1)
    exact, size = {}, {}
    fx, fd = [Fraction(float(v)) for v in Lpx], [Fraction(float(v)) for v in d]
    for k in range(n1):
        for a in range(p[k], p[k + 1]):
            t = fx[a] * fd[k]
            for b in range(p[k], a + 1):
                key = (i[a], i[b])
                term = t * fx[b]
                exact[key] = exact.get(key, 0) + term
                size[key] = size.get(key, 0) + abs(term)
    for r in range(n1, n):
        for c in range(n1, r + 1):
            v = Fraction(float(S[r - n1, c - n1]))
            exact[(r, c)] = exact.get((r, c), 0) + v
            size[(r, c)] = size.get((r, c), 0) + abs(v)
    C = _lower_entries(sc, sc.case.x)
    gamma = (n + 1) * Fraction(EPS)
    assert set(C) <= set(exact)
    assert all(abs(Fraction(C.get(key, 0.0)) - exact[key]) <= gamma * size[key] for key in exact)


def _inertia(w):
    return int(np.sum(w > 0)), int(np.sum(w < 0))


EXPECTED_INERTIA = {"grid-line-0": ((315, 237), (18, 6)), "grid-line-1": ((315, 237), (18, 6)),
                    "kkt-sqd-natural": ((200, 0), (0, 80)), "kkt-sqd": ((200, 0), (0, 80)), "kkt-zero": ((200, 0), (0, 80))}


@pytest.mark.parametrize("name", SC.SMALL)
def test_inertia_adds_up(name):
    """inertia(A) = inertia(A11) + inertia(S) (Haynsworth)"""
    sc = SC.BY_NAME[name]
    for which in SC.VALUE_SETS:
        _, d, S, info = SO.reference(sc, which)
        inner = (int(np.sum(d > 0)), int(np.sum(d < 0)))
        assert inner == info[:2]
        outer = _inertia(np.linalg.eigvalsh(S)) if sc.ns else (0, 0)
        whole = _inertia(np.linalg.eigvalsh(sc.dense(sc.values(which))))
        assert (inner[0] + outer[0], inner[1] + outer[1]) == whole, which
        if name in EXPECTED_INERTIA and which == "A":
            assert (inner, outer) == EXPECTED_INERTIA[name]
            if name.startswith("grid"):
                assert whole == (333, 243)


def test_kkt_sqd_against_numpys_schur_complement():
    sc = SC.BY_NAME["kkt-sqd"]
    _, _, S, _ = SO.reference(sc, "A")
    A = sc.dense()
    perm = SO.perm_of(sc)
    inner, kept = perm[:sc.n1], perm[sc.n1:]
    A11, A12, A22 = A[np.ix_(inner, inner)], A[np.ix_(inner, kept)], A[np.ix_(kept, kept)]
    ref = A22 - A12.T @ np.linalg.solve(A11, A12)
    err = np.linalg.norm(S - ref, 1) / np.linalg.norm(ref, 1)
    bound = tol.cross_bound(np.linalg.cond(A11, 1))
    print("kkt-sqd: |S - ref|_1 / |ref|_1 =", err, "bound", bound)
    assert err <= bound


def test_kkt_zero_needs_no_perturbation():
    sc = SC.BY_NAME["kkt-zero"]
    _, d, S, info = SO.reference(sc, "A")
    assert info == (200, 0, 0, -1)
    print("kkt-zero: min |d| =", np.min(np.abs(d)))
    assert np.min(np.abs(d)) >= 3.7                                     # (the issue's dense check: no pivot of H below 3.7)
    assert np.all(np.linalg.eigvalsh(S) < 0.0)                          # S = -A inv(H) A': negative definite


def test_bad_arguments_of_the_host_rule():
    import _csx
    sc = SC.BY_NAME["grid-line-0"]
    x = sc.case.x
    assert SO.host(sc, x)[0] == _csx.OK
    assert SO.host(sc, x, tau=-1.0)[0] == _csx.EINVAL and SO.host(sc, x, tau=float("nan"))[0] == _csx.EINVAL
    assert SO.host(sc, x, n1=-1)[0] == _csx.EINVAL and SO.host(sc, x, n1=sc.n + 1)[0] == _csx.EINVAL
    assert SO.host(sc, x, pinv=None)[0] == _csx.EINVAL                  # the pattern is that of P A P', not of A: an entry without a slot
    # ns ns >= 2^31, refused before anything is read but the ends of Lfp
    n = 46341
    Lfp, one, info = _csx.i32(np.arange(n + 1)), np.zeros(1), (_csx.C.c_int64 * 4)()
    st = _csx.load().csx_schur_host(n, _csx.pi(Lfp), None, None, None, _csx.pi(Lfp), None, 0, 0.0, _csx.pd(one), _csx.pd(one),
                                    _csx.pd(one), info)
    assert st == _csx.EINVAL


def test_python_face_without_a_device():
    import csparse as cs
    sc = SC.BY_NAME["two"]
    A = sc.matrix(cs)
    with pytest.raises(ValueError):
        cs.schur_factor(A, [1, 1])
    with pytest.raises(ValueError):
        cs.schur_factor(A, [2])
    with pytest.raises(ValueError):
        cs.schur_factor(A, [-1])
    with pytest.raises(ValueError):
        cs.schur_factor(A, [1], perturb=-1.0)
    T = cs.cs_spalloc(3, 3, 1, True, True)
    R = cs.cs_spalloc(3, 2, 2, True, False)
    assert cs.schur_factor(T, [0]) is None and cs.schur_factor(R, [0]) is None
