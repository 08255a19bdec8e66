"""backward_error(), refine(), condest() and operator_info() of cholsol_factor on the fixture of
tests/residual_sym_cases.py -- tests/test_residual_sym_cpu.py confirms on restated solves that a solve with A's factor starts at
omega0 >= 1e6 eps against the nearby A2 and that the loop ends at omega <= eps within 3 steps; the device is held to 4 eps
(its blocks are solved in the rounding-equal order) -- at order 0 and 1, exact None and True, on a list and on blocks of 1, 3
and 70 columns; against the factored matrix itself; after refactor() with a matrix and with values; after update(); and the
condition estimate against the dense restatement."""
import numpy as np
import pytest

import residual_sym_cases as SC
import trans_oracle as T
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = SC.EPS
BLOCKS = (1, 3, 70)


def _host_cs(cs, n, Ap, Ai, Ax):
    A = cs.cs_spalloc(n, n, max(len(Ai), 1), True, False)
    A.p, A.i, A.x = np.asarray(Ap).tolist(), np.asarray(Ai).tolist(), np.asarray(Ax).tolist()
    return A


@pytest.fixture(scope="module")
def case():
    return SC.perturbed_spd(SC.SEEDS[0])


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("exact", [None, True])
def test_refine_against_a_nearby_matrix_and_against_the_factored_one(cs, case, order, exact):
    n, Ap, Ai, Ax, Ax2 = case
    A, A2 = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax)), cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax2))
    F = cs.cholsol_factor(A, order, exact)
    assert F is not None and F.operator_info() == {"source": "factored", "builds": 0}
    for k in BLOCKS:
        B = SC.rhs(n, k, k)
        # a plain solve with the stale factor
        dX = cs.dvec(B)
        assert F.solve(dX) is True
        w_plain = F.backward_error(dX, cs.dvec(B), A=A2)
        print(order, exact, k, "plain omega / eps", w_plain.min() / EPS, w_plain.max() / EPS)
        assert w_plain.shape == (k,) and (w_plain >= 1e6 * EPS).all()
        dX = cs.dvec(B)
        out = F.refine(dX, A=A2)
        print(order, exact, k, "omega / eps", out["omega"].max() / EPS, "steps", out["steps"].max())
        assert sorted(out) == ["omega", "omega0", "rnorm", "solves", "steps"]
        assert out["omega0"].tobytes() == w_plain.tobytes()
        assert (out["omega"] <= 4.0 * EPS).all() and (out["omega"] <= out["omega0"]).all()
        assert F.backward_error(dX, cs.dvec(B), A=A2).tobytes() == out["omega"].tobytes()
        X = dX.numpy().reshape(n, k)
        assert F.backward_error(X, B, A=A2).tobytes() == out["omega"].tobytes()               # host blocks
        R, w, rn = cs.residual_block(A2, X, B, sym=True)
        assert w.tobytes() == out["omega"].tobytes() and rn.tobytes() == out["rnorm"].tobytes()
        assert F.operator_info()["source"] == "given"
        # against the factored matrix itself a solve is backward stable: at most one step
        dX = cs.dvec(B)
        own = F.refine(dX)
        print(order, exact, k, "own: omega0 / eps", own["omega0"].max() / EPS, "omega / eps", own["omega"].max() / EPS)
        assert (own["steps"] <= 1).all() and (own["omega"] <= 4.0 * EPS).all() and (own["omega"] <= own["omega0"]).all()
        assert F.backward_error(dX, cs.dvec(B)).tobytes() == own["omega"].tobytes()
        assert F.operator_info() == {"source": "factored", "builds": 0}
    # a list: one system, written back into the list
    b = SC.rhs(n, 1, 7)[:, 0].tolist()
    x = list(b)
    assert F.solve(x) is True
    w1 = F.backward_error(x, b, A=A2)
    assert isinstance(w1, float) and w1 >= 1e6 * EPS
    x = list(b)
    one = F.refine(x, A=A2)
    assert isinstance(x, list) and len(x) == n
    assert one["omega0"][0] == w1 and one["omega"][0] <= 4.0 * EPS and one["omega"][0] <= w1
    assert F.backward_error(x, b, A=A2) == one["omega"][0]
    x = list(b)
    own = F.refine(x)
    assert own["steps"][0] <= 1 and own["omega"][0] <= 4.0 * EPS and F.backward_error(x, b) == own["omega"][0]
    # A= of another shape, without values, or no matrix
    W = cs.cs_spalloc(n + 1, n + 1, 1, True, False)
    W.p = [0] * (n + 2)
    P = cs.cs_spalloc(n, n, 1, False, False)
    P.p = [0] * (n + 1)
    for bad, err in ((W, ValueError), (P, TypeError), (cs.cs_spalloc(n, n, 1, True, True), ValueError)):
        with pytest.raises(err):
            F.backward_error(x, b, A=bad)
        with pytest.raises(err):
            F.refine(list(b), A=bad)
        with pytest.raises(err):
            F.condest(A=bad)


def test_a_refused_step_leaves_the_column_as_it_was(cs):
    """The loop on a solver whose solve does nothing (x = b) for A = 2 I: omega0 = |b| / 3 |b| = 1 / 3, the step x + d = 0 has
    omega 1 and is refused; column 1 (b = 0) is never live.  One step tried, x still b bit for bit."""
    n, k = 70, 3
    A = cs.cs_spalloc(n, n, n, True, False)
    A.p, A.i, A.x = list(range(n + 1)), list(range(n)), [2.0] * n
    F = cs.cholsol_factor(A)
    calls = []

    def nothing(blk, trans, from_list):
        calls.append(from_list)
        return blk

    F._solve_block = nothing
    B = np.random.default_rng(3).integers(1, 1000, (n, k)) / 8.0          # 3 b is exact: b / 3 b rounds to the double 1 / 3
    B[:, 1] = 0.0
    dX = cs.dvec(B)
    out = F.refine(dX)
    assert dX.numpy().tobytes() == B.tobytes()
    assert out["steps"].tolist() == [0, 0, 0] and out["solves"] == 2 == len(calls)
    assert out["omega"].tolist() == [1.0 / 3.0, 0.0, 1.0 / 3.0] == out["omega0"].tolist()
    assert out["rnorm"].tobytes() == np.max(B, axis=0).tobytes()
    x = B[:, 0].tolist()
    out = F.refine(x, A=A)
    assert x == B[:, 0].tolist() and out["steps"].tolist() == [0] and F.backward_error(x, B[:, 0].tolist()) == 1.0 / 3.0
    assert calls == [False, False, True, True]


@pytest.mark.parametrize("order", [0, 1])
def test_after_a_refactor_the_operator_is_the_new_values(cs, case, order):
    n, Ap, Ai, Ax, Ax2 = case
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    A2 = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax2))
    F = cs.cholsol_factor(A, order)
    B = SC.rhs(n, 3, 5)

    def fresh():
        dX = cs.dvec(B)
        assert F.solve(dX) is True
        return dX

    assert F.refactor(Ax2) is True                                                # values: wrapped over A's pattern, once
    assert F.operator_info() == {"source": "refactored", "builds": 0}
    dX = fresh()
    w = F.backward_error(dX, cs.dvec(B))
    assert (w <= 4.0 * EPS).all()
    assert F.backward_error(dX, cs.dvec(B), A=A2).tobytes() == w.tobytes()
    assert (F.backward_error(dX, cs.dvec(B), A=A) >= 1e6 * EPS).all()              # not the factored matrix any more
    out = F.refine(cs.dvec(B))
    assert (out["steps"] <= 1).all() and (out["omega"] <= 4.0 * EPS).all()
    assert F.condest() == F.condest()
    assert F.operator_info() == {"source": "refactored", "builds": 1}
    # a dvec of values: kept (copied) until the next refactor, wrapped once more
    vals = cs.dvec(Ax2 * 1.0)
    assert F.refactor(vals) is True
    assert F.operator_info()["builds"] == 1
    assert F.backward_error(dX, cs.dvec(B)).tobytes() == w.tobytes()
    assert F.backward_error(dX, cs.dvec(B)).tobytes() == w.tobytes()
    assert F.operator_info() == {"source": "refactored", "builds": 2}
    # a `cs` with the values: no wrapped handle, the same numbers
    assert F.refactor(A2) is True
    assert F.backward_error(dX, cs.dvec(B)).tobytes() == w.tobytes()
    assert F.operator_info() == {"source": "refactored", "builds": 2}
    # back to A's own values: the stale solution shows
    assert F.refactor(Ax) is True
    assert (F.backward_error(dX, cs.dvec(B)) >= 1e6 * EPS).all()
    assert F.operator_info()["builds"] == 3
    # a refactor that fails changes nothing: the operator stays
    bad = Ax.copy()
    bad[0] = -bad[0]
    assert F.refactor(bad) is False
    assert (F.backward_error(fresh(), cs.dvec(B)) <= 4.0 * EPS).all() and F.operator_info()["builds"] == 3


@pytest.mark.parametrize("order", [0, 1])
def test_after_an_update_the_factor_stands_for_another_matrix(cs, case, order):
    n, Ap, Ai, Ax, Ax2 = case
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    F = cs.cholsol_factor(A, order)
    B = SC.rhs(n, 3, 6)
    # C = [0.5 e_0 + 0.25 e_1, 0.75 e_(n-1)]: rows 0 and 1 share the first block, which is dense
    Cm = cs.cs_spalloc(n, 2, 3, True, False)
    Cm.p, Cm.i, Cm.x = [0, 2, 3], [0, 1, n - 1], [0.5, 0.25, 0.75]
    assert F.update(Cm) is True
    b = B[:, 0].tolist()
    x = list(b)
    for call in (lambda: F.backward_error(x, b), lambda: F.refine(x), lambda: F.condest()):
        with pytest.raises(RuntimeError, match="A="):
            call()
    assert x == b
    # A + C C' on A's pattern: (0, 0), (0, 1), (1, 1) and (n-1, n-1)
    Ax3 = Ax.copy()
    cols = np.repeat(np.arange(n), np.diff(Ap))
    for r, c, v in ((0, 0, 0.25), (0, 1, 0.125), (1, 1, 0.0625), (n - 1, n - 1, 0.5625)):
        Ax3[np.flatnonzero((Ai == r) & (cols == c))[0]] += v
    A3 = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax3))
    dX = cs.dvec(B)
    assert F.solve(dX) is True
    w = F.backward_error(dX, cs.dvec(B), A=A3)
    print(order, "updated: omega / eps", w / EPS)
    assert (w <= 4.0 * EPS).all()
    assert (F.backward_error(dX, cs.dvec(B), A=A) > 1e6 * EPS).any()               # it is not A's factor any more
    assert F.operator_info()["source"] == "given"
    out = F.refine(cs.dvec(B), A=A3)
    assert (out["omega"] <= 4.0 * EPS).all()
    # a downdate that is refused changes nothing, and does not make the factor A's again
    big = cs.cs_spalloc(n, 1, 1, True, False)
    big.p, big.i, big.x = [0, 1], [n - 1], [1e3]
    assert F.downdate(big) is False
    with pytest.raises(RuntimeError):
        F.backward_error(dX, cs.dvec(B))
    # a refactor overwrites L from its values: A=None is legal again
    assert F.refactor(Ax) is True
    dX = cs.dvec(B)
    assert F.solve(dX) is True
    assert (F.backward_error(dX, cs.dvec(B)) <= 4.0 * EPS).all()
    assert F.operator_info()["source"] == "refactored"
    # ... until the next change in place
    assert F.downdate(Cm) is True
    with pytest.raises(RuntimeError):
        F.refine(cs.dvec(B))


def test_an_outside_cs_updown_on_the_factor_is_noticed(cs, case):
    n, Ap, Ai, Ax, Ax2 = case
    F = cs.cholsol_factor(cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax)))
    b = SC.rhs(n, 1, 8)[:, 0].tolist()
    x = list(b)
    assert F.solve(x) is True and F.backward_error(x, b) <= 4.0 * EPS
    Cm = cs.cs_spalloc(n, 1, 1, True, False)
    Cm.p, Cm.i, Cm.x = [0, 1], [n - 1], [0.5]
    assert cs.cs_updown(F.L, 1, Cm, F.symbolic.parent) is True
    with pytest.raises(RuntimeError, match="A="):
        F.backward_error(x, b)
    Ax3 = Ax.copy()
    Ax3[-1] += 0.25                                                              # the last stored entry is (n-1, n-1)
    x = list(b)
    assert F.solve(x) is True
    assert F.backward_error(x, b, A=_host_cs(cs, n, Ap, Ai, Ax3)) <= 4.0 * EPS


@pytest.mark.parametrize("order", [0, 1])
def test_condest_is_the_dense_estimate(cs, case, order):
    n, Ap, Ai, Ax, Ax2 = case
    want = T.condest_dense(SC.dense(n, Ap, Ai, Ax))
    F = cs.cholsol_factor(_host_cs(cs, n, Ap, Ai, Ax), order)
    e1, e2 = F.condest(), F.condest()
    assert e1 == e2
    assert abs(e1 - want) <= 1e-10 * want, (e1, want)
    # the strictly lower triangle is not part of the operator
    n2, p2, i2, x2 = SC.with_lower(n, Ap, Ai, Ax, 4, True)
    F2 = cs.cholsol_factor(_host_cs(cs, n2, p2, i2, x2), order)
    assert abs(F2.condest() - e1) <= 1e-10 * e1


def test_condest_of_one_by_one(cs):
    """cond_1 of a 1 x 1 matrix is 1.  |a| |solve(1)| alone gives 0.9999999999999999 for [2] -- the exact-order solve divides by
    l = sqrt(2) twice, as cs_lsolve and cs_ltsolve do, and (1 / l) / l is one unit in the last place below 1 / 2 --; condest()
    never reports less than 1, the least a condition number can be."""
    A = cs.cs_spalloc(1, 1, 1, True, False)
    A.p, A.i, A.x = [0, 1], [0], [2.0]
    assert cs.cholsol_factor(A).condest() == 1.0
    A.x = [3.0]                                                                    # sqrt(3) twice: just above 1 / 3 or just below
    assert 1.0 <= cs.cholsol_factor(A).condest() <= 1.0 + 4.0 * EPS
