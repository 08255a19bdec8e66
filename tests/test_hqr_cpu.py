"""csx_hqr_symbolic_host and csx_hqr_host (the symbolic step and the value rule of csx_hqr_factor on host arrays)
against csx_qr_host's patterns, the Python restatement (tests/hqr_oracle.py), the columnwise backward error of the reference
order, and the conditions that the GPU tests (tests/test_gpu_hqr.py) rely on, held here so that the host rule alone meets them
for the committed seeds.  No device.

Observed, max over the columns of eta_k / eps (new rule, reference order):
    see DESIGN.md §24; every case is printed by test_columnwise_backward_error.
Observed, omega / eps unrefined -> after each step, worst of the three committed right-hand sides (seed 20241017):
    printed by test_conditions; the spread over seeds 20241017 + 0..7 is in DESIGN.md §24."""
import numpy as np
import pytest

import _csx
import hqr_cases as HC
import hqr_oracle as HO

EPS = 2.0 ** -52


def _same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def test_the_library_says_its_window_without_a_device():
    assert HC.WINDOW >= 64 and HC.RUN_LEVELS == 256
    assert _csx.load().csx_hqr_window(None, None) == _csx.EINVAL


@pytest.mark.parametrize("name", HC.NAMES)
def test_symbolic_is_the_reference_loop(name):
    case = HC.BY_NAME[name]
    S = case.analysis
    st, Vp0, Vi0, _, Rp0, Ri0, _, _ = HO.host(case, case.x, "csx_qr_host")
    assert st == 0
    Vp, Rp = np.zeros(S.n + 1, np.int32), np.zeros(S.n + 1, np.int32)
    Vi, Ri = np.zeros(max(S.vnz, 1), np.int32), np.zeros(max(S.rnz, 1), np.int32)
    fi = S.i if len(S.i) else np.zeros(1, np.int32)
    st = _csx.load().csx_hqr_symbolic_host(S.m, S.n, S.m2, _csx.pi(S.p), _csx.pi(fi), _csx.pi(S.q), _csx.pi(S.parent),
                                           _csx.pi(S.pinv), _csx.pi(S.leftmost), max(S.vnz, 1), max(S.rnz, 1), _csx.pi(Vp),
                                           _csx.pi(Vi), _csx.pi(Rp), _csx.pi(Ri))
    assert st == 0
    assert Vp.tolist() == Vp0.tolist() and Rp.tolist() == Rp0.tolist()
    assert Vi[:Vp[-1]].tolist() == Vi0.tolist() and Ri[:Rp[-1]].tolist() == Ri0.tolist()
    assert [list(v) for v in HO.pattern_of(case)] == [Vp0.tolist(), Vi0.tolist(), Rp0.tolist(), Ri0.tolist()]
    assert Vp[-1] <= S.vnz and Rp[-1] <= S.rnz


def test_fictitious_rows_and_a_column_order():
    assert HC.BY_NAME["empty-row"].analysis.m2 > HC.BY_NAME["empty-row"].m
    for name in ("west-nd", "grid24-shift"):
        S = HC.BY_NAME[name].analysis
        assert S.q is not None and S.q.tolist() != list(range(S.n))
    S = HC.BY_NAME["lp_afiro"].analysis
    assert (S.m, S.n) == (51, 27)                              # the transpose is factored


@pytest.mark.parametrize("name", HC.NAMES)
def test_host_rule_is_the_restatement(name):
    case = HC.BY_NAME[name]
    pat = HO.pattern_of(case)
    for which in HC.VALUE_SETS:
        Vp, Vi, Vx, Rp, Ri, Rx, beta = HO.reference(case, which)
        vx, rx, bt = HO.hqr(case.analysis, HO.factored_values(case, case.values(which)), pat)
        assert _same(Vx, vx) and _same(Rx, rx) and _same(beta, bt), which
        # equal to the reference order's to rounding
        ref = HO.host(case, case.values(which), "csx_qr_host")
        assert np.allclose(Vx, ref[3], rtol=1e-9, atol=1e-12) and np.allclose(Rx, ref[6], rtol=1e-9, atol=1e-12)
    # the NaN set: a diagonal of R that is not finite, the only breakdown
    st, _, _, _, Rp, _, Rx, _ = HO.host(case, case.breaking())
    assert st == 0 and not np.isfinite(Rx[Rp[1] - 1])


def test_small_cases_by_hand():
    one = HO.reference(HC.BY_NAME["one"], "A")
    assert one[2].tolist() == [1.0] and one[5].tolist() == [3.0] and one[6].tolist() == [2.0]
    d = HO.reference(HC.BY_NAME["diagonal"], "A")
    assert d[5].tolist() == [1.0, 2.0, 0.0, 4.0, 5.0] and d[6].tolist() == [0.0, 2.0, 2.0, 2.0, 0.0]
    t = HO.reference(HC.BY_NAME["three-by-one"], "A")
    assert t[5].tolist() == [3.0]
    # of duplicate entries the last counts
    import slu_cases as SC
    clean = HC.Case("clean", *HC._square(SC.grid(6, sigma=HC.SIGMA)), seed=13)
    a, b = HO.reference(HC.BY_NAME["dups"], "A"), HO.reference(clean, "A")
    assert _same(a[2], b[2]) and _same(a[5], b[5]) and _same(a[6], b[6])


@pytest.mark.parametrize("name", ["grid24-shift", "grid24-shift-natural"])
def test_a_sequential_dot_product_or_a_fused_update_give_other_bytes(name):
    case = HC.BY_NAME[name]
    _, _, Vx, _, _, Rx, beta = HO.reference(case, "A")
    for mistake in ("sequential", "fused"):
        vx, rx, bt = HO.hqr(case.analysis, HO.factored_values(case, case.x), HO.pattern_of(case), **{mistake: True})
        assert not _same(Vx, vx) and not _same(Rx, rx), mistake
        assert np.allclose(Vx, vx, rtol=1e-8, atol=1e-11) and np.allclose(Rx, rx, rtol=1e-8, atol=1e-11), mistake


def _eta(case, factors):
    """max over the columns k of || Q R(:,k) - P A(:,q[k]) ||_2 / || A(:,q[k]) ||_2, norms in long double"""
    S = case.analysis
    Vp, Vi, Vx, Rp, Ri, Rx, beta = factors
    fx = HO.factored_values(case, case.x)
    worst = 0.0
    for k in range(S.n):
        r = np.zeros(S.m2)
        r[Ri[Rp[k]:Rp[k + 1]]] = Rx[Rp[k]:Rp[k + 1]]
        qr = HO.apply_q(S, Vp, Vi, Vx, beta, r, False).astype(np.longdouble)
        col = k if S.q is None else int(S.q[k])
        a = np.zeros(S.m2, np.longdouble)
        for p in range(S.p[col], S.p[col + 1]):
            a[S.pinv[S.i[p]]] = fx[p]
        den = np.sqrt(np.sum(a * a))
        if den == 0:
            continue
        worst = max(worst, float(np.sqrt(np.sum((qr - a) ** 2)) / den))
    return worst


@pytest.mark.parametrize("name", HC.NAMES)
def test_columnwise_backward_error(name):
    """both are Householder QR under error bounds of the same form, and a strided sum's bound is no worse than a sequential
    one's: the factor 4 covers the luck of one summation order on one matrix, the 4 eps floor the cases where the reference
    order is exact"""
    case = HC.BY_NAME[name]
    new = _eta(case, HO.reference(case, "A"))
    ref = _eta(case, HO.host(case, case.x, "csx_qr_host")[1:])
    print(name, "eta / eps: new rule", new / EPS, "reference order", ref / EPS)
    assert new <= max(4.0 * ref, 4.0 * EPS)


def test_least_squares_on_ash219():
    case = HC.BY_NAME["ash219"]
    S, A = case.analysis, case.dense()
    for b in HC.rhs(case):
        out = []
        for factors in (HO.reference(case, "A"), HO.host(case, case.x, "csx_qr_host")[1:]):
            x = HO.solve(S, factors, b)
            out.append(float(np.max(np.abs(A.T.astype(np.longdouble) @ (b - A.astype(np.longdouble) @ x)))))
        print("ash219 |A'(b - A x)|_inf: new rule", out[0], "reference order", out[1])
        # the floor: the size of one rounding error of the normal equations' residual, eps |A'| (|b| + |A| |x|)
        floor = 4.0 * EPS * float(np.max(np.abs(A.T) @ (np.abs(b) + np.abs(A) @ np.abs(x))))
        assert out[0] <= max(4.0 * out[1], floor)


def test_minimum_norm_on_lp_afiro():
    case = HC.BY_NAME["lp_afiro"]
    A = case.dense()
    for b in HC.rhs(case):
        x = HO.solve(case.analysis, HO.reference(case, "A"), b, second=True)
        want = np.linalg.lstsq(A, b, rcond=None)[0]            # the minimum-norm solution of the consistent system
        assert np.allclose(A @ x, b, rtol=0, atol=1e-10 * np.abs(b).max()) and np.allclose(x, want, rtol=1e-8, atol=1e-10)


# ---- the conditions tests/test_gpu_hqr.py relies on --------------------------------------------------------------------------
# Householder QR is backward stable as it stands, columnwise: A + dA = Q R with |dA(:,j)|_2 <= g |A(:,j)|_2, g of the form
# c m n eps (Higham, Accuracy and Stability, Thm 19.4), and the two triangular sweeps add terms of the same form.  omega is the
# COMPONENTWISE backward error, which that bound does not cover entry by entry; it is held here to the same form with c = 1,
# unrefined: omega0 <= m n eps.  What the GPU test relies on is the second condition: omega <= eps within WITHIN steps.
WITHIN = 3


@pytest.mark.parametrize("name", ["west", "west-nd", "grid24-shift", "grid24-shift-natural"])
def test_conditions(name):
    case = HC.BY_NAME[name]
    factors = HO.reference(case, "A")
    for trans in (False, True):
        out = [HO.refined(case, factors, b, WITHIN, trans) for b in HC.rhs(case)]
        print(name, "trans", trans, [[round(w / EPS, 3) for w in ws] for ws in out])
        for ws in out:
            assert ws[0] <= case.m * case.n * EPS and min(ws) <= EPS


def test_bad_arguments_of_the_host_functions():
    case = HC.BY_NAME["grid24-shift"]
    S = case.analysis
    lib = _csx.load()
    Vp, Rp = np.zeros(S.n + 1, np.int32), np.zeros(S.n + 1, np.int32)
    Vi, Ri = np.zeros(S.vnz, np.int32), np.zeros(S.rnz, np.int32)

    def call(m=S.m, parent=S.parent, pinv=S.pinv, leftmost=S.leftmost, q=S.q, vcap=S.vnz, rcap=S.rnz, m2=S.m2):
        return lib.csx_hqr_symbolic_host(m, S.n, m2, _csx.pi(S.p), _csx.pi(S.i), _csx.pi(q), _csx.pi(parent), _csx.pi(pinv),
                                         _csx.pi(leftmost), vcap, rcap, _csx.pi(Vp), _csx.pi(Vi), _csx.pi(Rp), _csx.pi(Ri))

    assert call() == _csx.OK
    assert call(vcap=int(Vp[-1]) - 1) == _csx.EINVAL and call(rcap=int(Rp[-1]) - 1) == _csx.EINVAL
    assert call(m=S.n - 1) == _csx.EINVAL and call(m2=S.m - 1) == _csx.EINVAL
    assert call(parent=np.full(S.n, -1, np.int32)) == _csx.EINVAL         # a forest of roots: the walks never reach k
    twice = S.pinv.copy()
    twice[1] = twice[0]
    assert call(pinv=twice) == _csx.EINVAL
    assert call(q=np.zeros(S.n, np.int32)) == _csx.EINVAL
    assert call(q=None) == _csx.EINVAL                                    # the analysis of A(:, q) is not A's own
    assert call(leftmost=np.full(S.m, S.n - 1, np.int32)) == _csx.EINVAL
    assert call(leftmost=np.zeros(S.m, np.int32)) == _csx.EINVAL
