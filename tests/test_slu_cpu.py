"""csx_slu_host (the value rule of csx_slu_factor on host arrays) against the Python restatement
(tests/slu_oracle.py), the textbook backward-error bound of the recurrence in exact rational arithmetic, csx_lu_host on a
diagonally dominant matrix where partial pivoting keeps the diagonal, and the conditions that the GPU tests
(tests/test_gpu_slu.py) rely on, held here so that the host rule alone meets them for the committed seeds.  No device.

Observed (omega / eps, unrefined -> after each step, worst of the three committed right-hand sides):
    grid24-shift 968 -> 0.79; grid24-shift-natural 2160 -> 0.85; one-sided 5640 -> 0.92; west (matched, seed 3) 115 -> 0.67;
    west-nd 1890 -> 0.88; fs183 6.3 -> 0.57; saddle-natural 99.5 -> 0.87; saddle (15 pivots perturbed) 1.2e9 -> 3.8e3 -> 0.95."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import _csx
import slu_cases as SC
import slu_oracle as SO

EPS = 2.0 ** -52
VECTORISED = ("long-column", "long-column-updated")     # see slu_oracle.slu


def _same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def _rule(case, x, tau, **kw):
    Lp, Li, _ = SO.pattern_of(case)
    return SO.slu(case, x, SO.pinv_of(case), Lp, Li, tau, **kw)


def test_the_library_says_its_window_without_a_device():
    assert SC.WINDOW >= 64 and SC.RUN_LEVELS >= 1
    assert _csx.load().csx_slu_window(None, None) == _csx.EINVAL


@pytest.mark.parametrize("name", SC.NAMES)
def test_host_rule_is_the_restatement(name):
    case = SC.BY_NAME[name]
    for which in SC.VALUE_SETS:
        x = case.values(which)
        Lx, Ux, info = SO.reference(case, which)
        rx, ru, rinfo = _rule(case, x, SO.tau_of(case, x), vectorised=name in VECTORISED)
        assert info == rinfo and info[3] == -1, which
        assert _same(Lx, rx) and _same(Ux, ru), which
        assert np.all(Lx[np.asarray(SO.pattern_of(case)[0][:-1])] == 1.0)
    # the breaking value set: the same column reported, nothing said about the values
    bad = case.breaking(*SO.first_pivot(case))
    tau = SO.tau_of(case, bad)
    st, _, _, info = SO.host(case, bad, tau)
    assert st == 0 and info[3] == 0
    assert _rule(case, bad, tau, vectorised=name in VECTORISED)[2][3] == 0


@pytest.mark.parametrize("name", ["blocks", "grid24-shift", "one-sided", "dups", "west-nd", "saddle"])
def test_the_vectorised_restatement_is_the_plain_one(name):
    case = SC.BY_NAME[name]
    x = case.A2[0]
    tau = SO.tau_of(case, x)
    a, b = _rule(case, x, tau), _rule(case, x, tau, vectorised=True)
    assert a[2] == b[2] and _same(a[0], b[0]) and _same(a[1], b[1])


@pytest.mark.parametrize("name", ["grid24-shift", "grid24-shift-natural"])
def test_descending_updates_or_a_fused_subtraction_give_other_bytes(name):
    case = SC.BY_NAME[name]
    Lx, Ux, _ = SO.reference(case, "A")
    for mistake in ("descending", "fused"):
        rx, ru, _ = _rule(case, case.x, 0.0, **{mistake: True})
        assert not _same(Lx, rx) and not _same(Ux, ru), mistake
        assert np.allclose(Lx, rx, rtol=1e-6, atol=1e-9) and np.allclose(Ux, ru, rtol=1e-6, atol=1e-9), mistake


def test_update_batches_has_the_rows_it_names_and_no_vanishing_pivot():
    """the forest of stars of tests/ldl_cases.py with unsymmetric values: no fill, the hub rows hold exactly 0, 1, 7, 8, 9, 16 and
    17 entries before the diagonal (the updates their columns take); no pivot of any value set is zero, perturbed or a breakdown"""
    import ldl_cases as LC
    case = SC.BY_NAME["update-batches"]
    Lp, Li, _ = SO.pattern_of(case)
    assert case.n == 65 and case.prow is None and SO.pinv_of(case) is None and Lp[-1] == case.n + sum(LC.STAR_LEAVES)
    updates = np.bincount(np.asarray(Li), minlength=case.n) - 1
    hubs = LC.star_hubs()
    assert all(updates[j] == hubs.get(j, 0) for j in range(case.n))
    D = case.dense()
    assert not np.array_equal(D, D.T) and len(set(np.diag(D).tolist())) == case.n
    for which in SC.VALUE_SETS:
        _, Ux, info = SO.reference(case, which)
        d = Ux[np.asarray(Lp[:-1])]
        assert info[2:] == (0, -1) and np.all(np.isfinite(d)) and np.all(d != 0.0), which


def test_duplicates_and_one_sided_entries():
    """of duplicate entries the last counts: the factor of `dups` is that of the matrix without them; a one-sided entry leaves an
    exact 0.0 in the other triangle's starting values, not a missing slot"""
    a, b = SO.reference(SC.BY_NAME["dups"], "A"), SO.reference(SC.BY_NAME["grid24-shift"], "A")
    assert SO.pattern_of(SC.BY_NAME["dups"])[:2] == SO.pattern_of(SC.BY_NAME["grid24-shift"])[:2]
    assert _same(a[0], b[0]) and _same(a[1], b[1])
    assert SO.pattern_of(SC.BY_NAME["one-sided"])[:2] == SO.pattern_of(SC.BY_NAME["grid24-shift"])[:2]
    assert not _same(SO.reference(SC.BY_NAME["one-sided"], "A")[1], b[1])


def _matrix_c(case, x):
    """{(r, c): value} of C = P A(prow, :) P' in the factor's numbering, of duplicates the last"""
    pinv, prinv = SO.pinv_of(case), SO.prinv_of(case)
    out = {}
    for q in range(len(case.i)):
        r = int(case.i[q]) if prinv is None else int(prinv[case.i[q]])
        c = int(case.cols[q])
        out[(r, c) if pinv is None else (pinv[r], pinv[c])] = float(x[q])
    return out


def _bound_holds(n, Lp, Li, Lx, Ux, C):
    """|C - L U| <= (n + 1) 2^-52 |L| |U| entry by entry, in exact rationals.  Entries outside the pattern are structurally zero
    on both sides."""
    exact, size = {}, {}
    fl, fu = [Fraction(float(v)) for v in Lx], [Fraction(float(v)) for v in Ux]
    for k in range(n):
        for a in range(Lp[k], Lp[k + 1]):
            for b in range(Lp[k], Lp[k + 1]):
                key = (Li[a], Li[b])                 # L(r, k) U(k, c)
                term = fl[a] * fu[b]
                exact[key] = exact.get(key, 0) + term
                size[key] = size.get(key, 0) + abs(term)
    gamma = (n + 1) * Fraction(EPS)
    assert set(C) <= set(exact)
    return all(abs(Fraction(C.get(key, 0.0)) - exact[key]) <= gamma * size[key] for key in exact)


@pytest.mark.parametrize("name", ["grid24-shift", "west", "saddle-natural"])
def test_componentwise_backward_error_of_the_factorisation(name):
    case = SC.BY_NAME[name]
    Lp, Li, _ = SO.pattern_of(case)
    Lx, Ux, _ = SO.reference(case, "A")
    assert _bound_holds(case.n, Lp, Li, Lx, Ux, _matrix_c(case, case.x))


def _lu_host(case, tol):
    """csx_lu_host on the case's matrix in natural order: dense L, U and pinv"""
    C, lib, n = ctypes, _csx.load(), case.n
    out = [C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(),
           C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()]
    pinv = np.empty(n, np.int32)
    st = lib.csx_lu_host(n, _csx.pi(case.p), _csx.pi(case.i), _csx.pd(case.x), float(tol), *[C.byref(o) for o in out], _csx.pi(pinv))
    assert st == _csx.OK
    try:
        def dense(op, oi, ox):
            p = np.ctypeslib.as_array(op, shape=(n + 1,)).copy()
            i = np.ctypeslib.as_array(oi, shape=(p[n],)).copy()
            x = np.ctypeslib.as_array(ox, shape=(p[n],)).copy()
            D, S = np.zeros((n, n)), np.zeros((n, n), bool)
            cols = np.repeat(np.arange(n), np.diff(p))
            D[i, cols], S[i, cols] = x, True
            return D, S
        (L, SL), (U, SU) = dense(*out[:3]), dense(*out[3:])
    finally:
        for o in out:
            lib.csx_host_free(C.cast(o, C.c_void_p))
    return L, SL, U, SU, pinv


def test_the_pivoting_lu_agrees_where_it_keeps_the_diagonal():
    case = SC.BY_NAME["grid24-natural"]
    n = case.n
    L0, SL, U0, SU, pinv = _lu_host(case, 0.1)
    assert pinv.tolist() == list(range(n))                   # diagonally dominant: the diagonal is within 0.1 of every column's largest
    Lp, Li, _ = SO.pattern_of(case)
    Lx, Ux, info = SO.reference(case, "A")
    assert info[3] == -1
    cols = np.repeat(np.arange(n), np.diff(Lp))
    L, U, S = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n), bool)
    L[Li, cols], U[cols, Li], S[Li, cols] = Lx, Ux, True
    assert not (SL & ~S).any() and not (SU & ~S.T).any()     # cs_lu's pattern lies inside the static one
    for got, ref, on in ((L, L0, SL), (U, U0, SU)):
        assert np.all(ref[on] != 0.0) and np.all(np.abs(got[on] - ref[on]) <= 1e-10 * np.abs(ref[on]))
    assert np.all(L[S & ~SL] == 0.0) and np.all(U[S.T & ~SU] == 0.0)   # the extra slots of the static pattern: exactly 0.0


# ---- the conditions tests/test_gpu_slu.py relies on --------------------------------------------------------------------------

def _steps(case, steps):
    Lx, Ux, info = SO.reference(case, "A")
    assert info[3] == -1
    out = [SO.refined(case, Lx, Ux, b, steps) for b in SC.rhs(case)]
    print(case.name, info, [[round(w / EPS, 3) for w in ws] for ws in out])
    return out


@pytest.mark.parametrize("name", ["grid24-shift", "grid24-shift-natural", "one-sided"])
def test_conditions_shifted_grid(name):
    """refinement has work to do and does it"""
    for ws in _steps(SC.BY_NAME[name], 3):
        assert ws[0] >= 16 * EPS and min(ws) <= EPS


@pytest.mark.parametrize("name", ["west", "west-nd", "fs183", "saddle-natural"])
def test_conditions_matched_and_natural(name):
    case = SC.BY_NAME[name]
    if case.prow is not None:                               # the committed rows are a matching: a zero-free diagonal
        D = case.dense()
        assert sorted(case.prow.tolist()) == list(range(case.n)) and np.all(D[case.prow, np.arange(case.n)] != 0.0)
        assert int(np.sum(np.diag(D) == 0.0)) == 65         # ... which the matrix itself does not have
    for ws in _steps(case, 3):
        assert min(ws) <= EPS


def test_conditions_saddle():
    case = SC.BY_NAME["saddle"]
    assert case.breaks and case.perturb == 1e-10
    assert SO.host(case, case.x, 0.0)[3][3] >= 0            # a breakdown without the perturbation
    info = SO.reference(case, "A")[2]
    assert 9 <= info[2] <= 17 and info[3] == -1
    for ws in _steps(case, 4):
        assert min(ws) <= EPS


def test_bad_arguments_of_the_host_rule():
    case = SC.BY_NAME["grid24-shift-natural"]
    lib, n = _csx.load(), case.n
    Lp, Li, _ = SO.pattern_of(case)
    Lp, Li = _csx.i32(Lp), _csx.i32(Li)
    Lx, Ux, info = np.zeros(Lp[n]), np.zeros(Lp[n]), (_csx.C.c_int64 * 4)()

    def call(prow=None, pinv=None, tau=0.0, Li=Li):
        return lib.csx_slu_host(n, _csx.pi(case.p), _csx.pi(case.i), _csx.pd(case.x), _csx.pi(prow), _csx.pi(pinv), _csx.pi(Lp),
                                _csx.pi(Li), tau, _csx.pd(Lx), _csx.pd(Ux), info)

    assert call() == _csx.OK
    assert call(tau=-1.0) == _csx.EINVAL and call(tau=float("nan")) == _csx.EINVAL
    twice = np.arange(n, dtype=np.int32)
    twice[1] = 0
    assert call(prow=twice) == _csx.EINVAL and call(pinv=twice) == _csx.EINVAL
    swap = np.arange(n, dtype=np.int32)
    swap[[0, n - 1]] = [n - 1, 0]
    assert call(prow=swap) == _csx.EINVAL                    # an entry of A(prow, :) without a slot in this pattern
    broken = Li.copy()
    broken[1] = 0
    assert call(Li=broken) == _csx.EINVAL
