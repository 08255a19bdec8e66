"""backward_error() and refine() of lusol_factor and btf_factor on the stale-pivot fixture of
tests/refine_cases.py -- tests/test_refine_cpu.py confirms on the CPU restatement that a solve on the kept pivots starts
at omega0 >= 1e3 eps and that the loop ends at omega <= eps within 3 steps; the device is held to 4 eps (its blocks are
solved in the rounding-equal order) -- forward and transposed, dvec block and list; on well-conditioned matrices; and the
loop's own guarantees: omega <= omega0, a refused step leaves the column bit for bit as it was."""
import numpy as np
import pytest

import btf_oracle
import refine_cases as RC
import tol
from conftest import golden, unpack
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = RC.EPS
NONZERO = np.arange(RC.K) != RC.ZERO_COLUMN


def _host_cs(cs, n, Ap, Ai, Ax):
    A = cs.cs_spalloc(n, n, max(len(Ai), 1), True, False)
    A.p, A.i, A.x = np.asarray(Ap).tolist(), np.asarray(Ai).tolist(), np.asarray(Ax).tolist()
    return A


def _factor(cs, which, A):
    return cs.lusol_factor(A, 0, 1.0) if which == "lusol" else cs.btf_factor(A, 1.0)


@pytest.fixture(scope="module")
def case():
    return RC.stale_pivot(RC.SEEDS[0])


@pytest.mark.parametrize("which", ["lusol", "btf"])
@pytest.mark.parametrize("trans", [False, True])
def test_refine_wins_back_the_digits_stale_pivots_lose(cs, case, which, trans):
    n, Ap, Ai, Ax, Ax2, B = case
    F = _factor(cs, which, cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax)))
    assert F is not None
    assert F.refactor(Ax2) is True and F.refactor_info()["pivot_ratio"] <= 1e-5
    # a plain solve on the kept pivots
    dX = cs.dvec(B)
    assert F.solve(dX, trans=trans) is True
    w_plain = F.backward_error(dX, cs.dvec(B), trans=trans)
    print(which, trans, "plain omega / eps", w_plain / EPS)
    assert w_plain.shape == (RC.K,) and (w_plain[NONZERO] >= 1e3 * EPS).all() and w_plain[RC.ZERO_COLUMN] == 0.0
    # the block
    dX = cs.dvec(B)
    out = F.refine(dX, trans=trans)
    print(which, trans, "omega0 / eps", out["omega0"] / EPS, "omega / eps", out["omega"] / EPS, "steps", out["steps"])
    assert sorted(out) == ["omega", "omega0", "rnorm", "solves", "steps"]
    assert out["omega0"].tobytes() == w_plain.tobytes()
    assert (out["omega"] <= 4.0 * EPS).all() and (out["omega"] <= out["omega0"]).all() and (out["steps"] <= 3).all()
    assert out["omega"][RC.ZERO_COLUMN] == 0.0 and out["steps"][RC.ZERO_COLUMN] == 0
    X = dX.numpy()
    assert not X[:, RC.ZERO_COLUMN].any()
    assert F.backward_error(dX, cs.dvec(B), trans=trans).tobytes() == out["omega"].tobytes()
    assert F.backward_error(X, B, trans=trans).tobytes() == out["omega"].tobytes()           # host blocks
    R, w, rn = cs.residual_block(_host_cs(cs, n, Ap, Ai, Ax2), X, B, trans=trans)
    assert w.tobytes() == out["omega"].tobytes() and rn.tobytes() == out["rnorm"].tobytes()
    assert out["solves"] == 1 + int(out["steps"].max()) or out["solves"] == 2 + int(out["steps"].max())
    # a list: one system, written back into the list
    for c in (0, RC.ZERO_COLUMN):
        b = B[:, c].tolist()
        x = list(b)
        assert F.solve(x, trans=trans) is True
        w1 = F.backward_error(x, b, trans=trans)
        assert isinstance(w1, float) and (w1 >= 1e3 * EPS if c != RC.ZERO_COLUMN else w1 == 0.0)
        x = list(b)
        one = F.refine(x, trans=trans)
        assert isinstance(x, list) and len(x) == n
        assert one["omega0"][0] == w1 and one["omega"][0] <= min(4.0 * EPS, w1) and one["steps"][0] <= 3
        assert F.backward_error(x, b, trans=trans) == one["omega"][0]
        if c == RC.ZERO_COLUMN:
            assert one["steps"][0] == 0 and not any(x)
    # the matrix the solver stands for was wrapped once for all of these calls; the next refactor wraps the new values
    assert F._operator_builds == 1
    assert F.refactor(Ax2 * 1.0) is True
    assert F._operator_builds == 1
    assert F.backward_error(dX, cs.dvec(B), trans=trans).tobytes() == out["omega"].tobytes()
    assert F._operator_builds == 2
    # a `cs` with the values: no wrapped handle, the same numbers
    assert F.refactor(cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax2))) is True
    assert F.backward_error(dX, cs.dvec(B), trans=trans).tobytes() == out["omega"].tobytes()
    assert F._operator_builds == 2


@pytest.mark.parametrize("which", ["lusol", "btf"])
def test_columns_that_take_no_step_do_not_move(cs, case, which):
    n, Ap, Ai, Ax, Ax2, B = case
    F = _factor(cs, which, cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax)))
    assert F.refactor(Ax2) is True
    runs = []
    for maxit in range(4):
        dX = cs.dvec(B)
        out = F.refine(dX, maxit=maxit)
        runs.append((dX.numpy(), out))
    plain = cs.dvec(B)
    assert F.solve(plain) is True
    assert runs[0][0].tobytes() == plain.numpy().tobytes() and not runs[0][1]["steps"].any() and runs[0][1]["solves"] == 1
    for (xa, a), (xb, b) in zip(runs, runs[1:]):
        assert (b["omega"] <= a["omega"]).all()
        for c in range(RC.K):
            if a["steps"][c] == b["steps"][c]:
                assert xa[:, c].tobytes() == xb[:, c].tobytes() and a["omega"][c] == b["omega"][c]
            else:
                assert b["omega"][c] < a["omega"][c]


def test_a_refused_step_leaves_the_column_as_it_was(cs):
    """The loop on a solver that does not solve (x = b) for A = 2 I: omega0 = |b| / 3 |b| = 1 / 3, the step x + d = 0 has
    omega 1 and is refused; column 1 (b = 0) is never live.  One step tried, x still b bit for bit."""
    n, k = 70, 3
    A = cs.cs_spalloc(n, n, n, True, False)
    A.p, A.i, A.x = list(range(n + 1)), list(range(n)), [2.0] * n

    class Identity(cs._Refinable):
        def __init__(self):
            self._A2 = A
            self._refine_init(A, n)
            self.calls = 0

        def _solve_block(self, blk, trans, from_list):
            self.calls += 1
            return blk

    B = np.random.default_rng(3).integers(1, 1000, (n, k)) / 8.0          # 3 b is exact: b / 3 b rounds to the double 1 / 3
    B[:, 1] = 0.0
    S = Identity()
    dX = cs.dvec(B)
    out = S.refine(dX)
    assert dX.numpy().tobytes() == B.tobytes()
    assert out["steps"].tolist() == [0, 0, 0] and out["solves"] == 2 == S.calls
    assert out["omega"].tolist() == [1.0 / 3.0, 0.0, 1.0 / 3.0] == out["omega0"].tolist()
    assert out["rnorm"].tobytes() == np.max(B, axis=0).tobytes()
    x = B[:, 0].tolist()
    out = S.refine(x)
    assert x == B[:, 0].tolist() and out["steps"].tolist() == [0] and S.backward_error(x, B[:, 0].tolist()) == 1.0 / 3.0


def test_well_conditioned_systems_take_at_most_one_step(cs):
    g = golden("west0067")
    A = unpack(cs, g, "C")
    n = A.n
    B = np.random.default_rng(1).uniform(-1.0, 1.0, (n, 4))
    S, _, _ = btf_oracle.reducible(btf_oracle.block_sizes(300, 3), 3, 3)
    Ared = _host_cs(cs, S.shape[0], S.indptr, S.indices, S.data)
    Bred = np.random.default_rng(2).uniform(-1.0, 1.0, (S.shape[0], 4))
    for F, Bk in ((cs.lusol_factor(cs.cs_pin(A), 0, 1.0), B), (cs.btf_factor(cs.cs_pin(Ared), 1.0), Bred)):
        assert F is not None
        for trans in (False, True):
            plain = cs.dvec(Bk)
            assert F.solve(plain, trans=trans) is True
            dX = cs.dvec(Bk)
            out = F.refine(dX, trans=trans)
            print("omega0 / eps", out["omega0"] / EPS, "omega / eps", out["omega"] / EPS, "steps", out["steps"])
            assert (out["steps"] <= 1).all() and (out["omega"] <= out["omega0"]).all()
            X, P = dX.numpy(), plain.numpy()
            for c in range(Bk.shape[1]):
                assert tol.componentwise(X[:, c], P[:, c]) <= tol.X_RTOL, (trans, c)
            b = Bk[:, 0].tolist()
            x = list(b)
            one = F.refine(x, trans=trans)
            assert one["steps"][0] <= 1 and tol.componentwise(x, P[:, 0]) <= tol.X_RTOL
            assert F._operator_builds == 0                                     # never refactored: the matrix itself
