"""The supernodal solve (csx_snsolve.hip) at every kernel route, width class and cut of its schedule (needs an MI355X).

The inputs are the synthetic factors of tests/sn_cases.py, one per edge (tests/test_sn_cases_cpu.py shows without a device
that each sits on its edge).  For every case:
  * it got there: the route is the supernodal one, the plan's geometry (csx_cholsol_sn_geometry) equals the model's field
    for field, and the launches of every solve (csx_cholsol_sn_launches, counted under "tri.graph" = 0) are exactly the ones
    the model expects for that number of right-hand sides;
  * it is right: columns 0, k // 2 and k - 1 against the plain-C oracle's cs_lsolve + cs_ltsolve on the same arrays, in
    SURVEY 8d's componentwise measure at 1e-10 and normwise at 1e-12;
  * it is the same whatever ran: the same bits on a second run, and column r of a batch of k has the bits it has in the
    case's largest batch -- across lanes per task, a wave per task and a workgroup per task, across one wave per 16 and per
    64 right-hand sides of a triangle;
  * the exact order on the same plan stays bit-identical to the oracle;
  * columns do not leak: a non-finite column in a block of 70 leaves every other column's bits alone.  (Inside its own
    column a non-finite entry spreads further than in the reference: the padded lanes of a sum multiply 0.0 by row 0 of X,
    the dense tiles multiply structural zeros.  DESIGN.md says so.)

The 1e-10 componentwise budget is asserted on right-hand sides made from a solution of size 1 (`manufactured_rhs` says why);
the bound that holds for any right-hand side is SN_EPS_UNITS (tests/tol.py), in roundings of the terms of a component.
tools/measure_snsolve_edges.py runs `run_case` for every case and writes profiles/snsolve_edges.jsonl, from which that bound
was taken."""
import numpy as np
import pytest

import conftest  # noqa: F401  (the package and oracle paths, also for tools/measure_snsolve_edges.py)
import _csx
import c_oracle as CO
import sn_cases as SC
import tol as TOL
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu


def _solve(cs, lib, plan, B):
    n, k = B.shape
    X = cs.dvec(np.ascontiguousarray(B))
    _csx.check(lib.csx_cholsol_solve(plan, X.handle, k), "csx_cholsol_solve")
    return X.numpy().reshape(n, k).copy()


def manufactured_rhs(n, Lp, Li, Lx, k, seed):
    """B = L L' X0 with every |X0[i, r]| in [0.5, 1.5]: no component of a solution is a chance cancellation.  Among the
    250 000 components of a solution to a random right-hand side some land at 1e-8 of the terms they were summed from (seen
    on the device: x = 1.2e-8 from terms of 1.7e-2, off the oracle by 6e-18 -- 1.6 roundings of those terms, a normwise error
    of 7e-16).  There SURVEY 8d's measure at 1e-10 asks for a third of ONE rounding of the terms, less than the reference's own
    error in its own order of summation; the measure is meant for components that carry their terms' magnitude."""
    rng = np.random.default_rng(seed)
    X0 = rng.choice([-1.0, 1.0], (n, k)) * rng.uniform(0.5, 1.5, (n, k))
    L = TOL.csc(n, Lp, Li, Lx)
    return np.ascontiguousarray(L @ (L.T @ X0))


def run_case(cs, name):
    """all the checks of one case; returns the largest |x - ref| / (eps * terms) over the compared columns"""
    case = SC.BY_NAME[name]
    n, Lp, Li, Lx, growth, M, expected = SC.built(name)
    lib = _csx.lib()
    kmax = max(max(case.ks), 70)
    if case.bad_block is None:
        B = manufactured_rhs(n, Lp, Li, Lx, kmax, len(name) + n)
    else:
        # the guard's cases (a few hundred columns) take random right-hand sides, as the ill-conditioned-block test of
        # tests/test_gpu_cholesky.py does: through a block whose inverse has entries of 1e4 a solution of size 1 is an
        # ill-conditioned problem, on which two correct orders of summation differ by that factor
        B = np.random.default_rng(len(name) + n).uniform(-1.0, 1.0, (n, kmax))
    oracle = {}

    def ref(r):
        if r not in oracle:
            y = CO.lsolve(n, Lp, Li, Lx, B[:, r].copy())
            x = CO.ltsolve(n, Lp, Li, Lx, y)
            oracle[r] = (x, TOL.cholsolve_terms(n, Lp, Li, Lx, y, x))
        return oracle[r]

    hL, plan = _csx.new_handle(), _csx.new_handle()
    worst = 0.0
    with _csx.option("tri.supernodes", case.mode), _csx.option("tri.graph", 0):
        _csx.check(lib.csx_csc_upload(n, n, _csx.pi(Lp), _csx.pi(Li), _csx.pd(Lx), hL))
        try:
            _csx.check(lib.csx_cholsol_plan(hL, None, plan))
            _csx.check(lib.csx_cholsol_set_order(plan, 0))
            # ---- it got there
            path, mc, g = _csx.C.c_int32(-1), _csx.C.c_int32(-1), _csx.C.c_double(-1.0)
            _csx.check(lib.csx_cholsol_info(plan, path, None, None))
            assert path.value == case.path, path.value
            if M is None:
                count = _csx.C.c_int32(0)
                assert lib.csx_cholsol_sn_geometry(plan, None, 0, count) == _csx.EINVAL
                assert lib.csx_cholsol_sn_launches(plan, None, 0, count) == _csx.EINVAL
            else:
                got, want = _csx.cholsol_sn_geometry(plan), SC.model_geometry(M)
                assert got == want, (got, want)
                _csx.check(lib.csx_cholsol_sn_info(plan, None, None, None, mc, g))
                assert mc.value == M["matrix_cores"]
                if case.mode == 1:           # the guard's measure as numpy has it (sums in another order)
                    assert abs(g.value - growth) <= 1e-9 * growth, (g.value, growth)
            # ---- it is right, and the same whatever ran
            Xmax = _solve(cs, lib, plan, B[:, :max(case.ks)])
            for k in case.ks:
                X = _solve(cs, lib, plan, B[:, :k])
                if M is not None:
                    got, want = _csx.cholsol_sn_launches(plan), expected(k)
                    assert got == want, (k, got, want)
                assert X.tobytes() == _solve(cs, lib, plan, B[:, :k]).tobytes(), k
                assert X.tobytes() == np.ascontiguousarray(Xmax[:, :k]).tobytes(), k
                for r in sorted({0, k // 2, k - 1}):
                    x, terms = ref(r)
                    assert TOL.componentwise(X[:, r], x, terms) <= TOL.X_RTOL, (k, r)
                    assert TOL.normwise(X[:, r], x) <= 1e-12, (k, r)
                    worst = max(worst, float(np.max(np.abs(X[:, r] - x) / (TOL.EPS * terms))))
            # ---- columns do not leak
            clean = _solve(cs, lib, plan, B[:, :70])
            Bad = B[:, :70].copy()
            Bad[0, 5] = np.inf
            Bad[n - 1, 5] = np.nan
            dirty = _solve(cs, lib, plan, Bad)
            others = [r for r in range(70) if r != 5]
            assert dirty[:, others].tobytes() == clean[:, others].tobytes()
            assert not np.all(np.isfinite(dirty[:, 5]))
            # ---- the exact order on the same plan: the oracle's bits
            _csx.check(lib.csx_cholsol_set_order(plan, 1))
            Xe = _solve(cs, lib, plan, B[:, :2])
            for r in range(2):
                assert Xe[:, r].tobytes() == ref(r)[0].tobytes(), r
        finally:
            _csx.free(plan)
            _csx.free(hL)
    return worst


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_supernodal_solve_on_the_edge(cs, name):
    units = run_case(cs, name)
    print("%s: largest |x - ref| / (eps * terms) = %.3f" % (name, units))
    if SC.BY_NAME[name].bad_block is None:
        assert units <= TOL.SN_EPS_UNITS

