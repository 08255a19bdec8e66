"""The stale-pivot fixture of tests/refine_cases.py does what tests/test_gpu_refine.py relies on, confirmed on the CPU
restatement: csparse_oracle.cs_lu at tol = 1 keeps A's diagonal, tests/refactor_oracle.py gives the factors of the new values
on those pivots (pivot_ratio <= 1e-5), and the refinement loop on the plain-C solves and tests/residual_oracle.py starts
from omega0 >= 1e3 eps on every non-zero column and ends at omega <= eps within 3 steps -- forward and transposed.  Then
the loop's own properties: omega <= omega0, and a column whose step count did not move did not move either."""
import numpy as np
import pytest

import c_oracle as CO
import csparse_oracle as O
import refactor_oracle
import refine_cases as RC
import residual_oracle as RO

EPS = RC.EPS


def _restatement(seed, trans):
    n, Ap, Ai, Ax, Ax2, B = RC.stale_pivot(seed)
    A = O.cs_spalloc(n, n, len(Ai), True, False)
    A.p, A.i, A.x = Ap.tolist(), Ai.tolist(), Ax.tolist()
    N = O.cs_lu(A, O.cs_sqr(0, A, False), 1.0)
    assert N is not None and list(N.pinv) == list(range(n))                    # the diagonal, by dominance
    Lx, Ux, ok, ratio = refactor_oracle.refactor(N.L, N.U, N.pinv, (Ap, Ai, Ax2))
    assert ok and ratio <= 1e-5
    Lp, Li = np.asarray(N.L.p, np.int32), np.asarray(N.L.i[:N.L.p[n]], np.int32)
    Up, Ui = np.asarray(N.U.p, np.int32), np.asarray(N.U.i[:N.U.p[n]], np.int32)
    Lx, Ux = np.asarray(Lx), np.asarray(Ux)

    def solve_one(b):
        if trans:                                                               # cs_pvec(q), U', L', cs_pvec(pinv); q natural
            y = CO.ltsolve(n, Lp, Li, Lx, CO.utsolve(n, Up, Ui, Ux, b))
            return CO.pvec(N.pinv, y)
        return CO.usolve(n, Up, Ui, Ux, CO.lsolve(n, Lp, Li, Lx, CO.ipvec(N.pinv, b)))

    def solve(Bk):
        return np.column_stack([solve_one(np.ascontiguousarray(Bk[:, c])) for c in range(Bk.shape[1])])

    def residual(X, Bk):
        k = Bk.shape[1]
        R, w, _ = RO.residual(n, n, Ap, Ai, Ax2, k, trans, X.reshape(-1).tolist(), Bk.reshape(-1).tolist())
        return np.asarray(R).reshape(n, k), w

    return B, solve, residual


@pytest.mark.parametrize("seed", RC.SEEDS)
@pytest.mark.parametrize("trans", [False, True])
def test_stale_pivots_lose_digits_and_refinement_wins_them_back(seed, trans):
    B, solve, residual = _restatement(seed, trans)
    out = RC.refine_loop(solve, residual, B)
    nonzero = np.arange(RC.K) != RC.ZERO_COLUMN
    print("omega0 / eps", out["omega0"] / EPS, "omega / eps", out["omega"] / EPS, "steps", out["steps"])
    assert (out["omega0"][nonzero] >= 1e3 * EPS).all()
    assert (out["omega"] <= EPS).all() and (out["steps"] <= 3).all()
    assert out["omega0"][RC.ZERO_COLUMN] == 0.0 and out["steps"][RC.ZERO_COLUMN] == 0
    assert not out["x"][:, RC.ZERO_COLUMN].any()
    assert (out["omega"] <= out["omega0"]).all()
    assert out["solves"] == 1 + int(out["steps"].max()) or out["solves"] == 2 + int(out["steps"].max())
    assert np.asarray(residual(out["x"], B)[1]).tobytes() == out["omega"].tobytes()


def test_a_column_that_took_no_step_is_bit_for_bit_as_it_was():
    B, solve, residual = _restatement(RC.SEEDS[0], False)
    runs = [RC.refine_loop(solve, residual, B, maxit=t) for t in range(5)]
    assert runs[0]["x"].tobytes() == solve(B).tobytes() and not runs[0]["steps"].any()
    for a, b in zip(runs, runs[1:]):
        assert (b["omega"] <= a["omega"]).all()
        for c in range(RC.K):
            if a["steps"][c] == b["steps"][c]:
                assert a["x"][:, c].tobytes() == b["x"][:, c].tobytes() and a["omega"][c] == b["omega"][c]
            else:
                assert b["omega"][c] < a["omega"][c]


def test_a_step_that_does_not_lower_omega_is_rejected():
    """a solver that is exact to rounding and a residual that reports a constant omega above eps: every step is refused,
    one step is tried (the column then stops), x stays the first solve's"""
    B = np.array([[1.0, 2.0], [3.0, 4.0]])
    calls = []

    def solve(Bk):
        calls.append(1)
        return Bk * 0.5

    def residual(X, Bk):
        return Bk - 2.0 * X + 1e-3, [3.0 * EPS, 0.0]

    out = RC.refine_loop(solve, residual, B)
    assert out["x"].tobytes() == (B * 0.5).tobytes() and out["steps"].tolist() == [0, 0]
    assert out["solves"] == 2 == len(calls) and out["omega"].tolist() == [3.0 * EPS, 0.0]
