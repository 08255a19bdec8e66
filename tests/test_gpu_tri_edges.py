"""The generic triangular solve (csx_trisolve.hip) on the constructed cases of tests/tri_cases.py: one matrix per side of every
cut of tri_route, make_segments and walk_levels, solved through cs_lsolve / cs_ltsolve / cs_usolve / cs_utsolve.  For every case
  * the library's read-backs say what ran: csx_tri_route_info equals the Python model field for field, and csx_tri_launches
    counts exactly the kernel instances the model predicts, each as often;
  * the result equals the plain-C oracle's byte for byte in every right-hand-side column, a second solve gives the same bytes
    (and launches the same kernels), and where the case names options that force another route, that route gives the same bytes;
and per route: a NaN in one right-hand-side column leaves every other column's bytes alone; a zero on the diagonal is refused
with ZeroDivisionError; csx_lusol_solve / csx_lusol_solve_trans in the exact order fuse exactly when both factors route Local, and the fused and the
four-step form give the bytes of permute, oracle, oracle, permute.  The rounding-equal orders are held to tol.TRI_EPS_UNITS
roundings of a component's terms: the matrix-core sweep with the three outcomes of its guard, the pair of them fused in
csx_lusol_solve / csx_lusol_solve_trans, and cholsol_factor(exact=False) on a band, whose plan's two triangular plans are read
back through the cholsol plan (L' on the rows of L; the relaxed chain walker on a schedule from the elimination tree's hint).
tests/test_tri_cases_cpu.py shows without a device that every case sits on the edge it is named for."""
import contextlib

import numpy as np
import pytest

import c_oracle as CO
import tri_cases as TC
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _options(opts):
    import _csx
    with contextlib.ExitStack() as held:
        for name, value in opts.items():
            held.enter_context(_csx.option(name, value))
        yield


def _pinned(cs, T):
    n, Tp, Ti, Tx = T
    A = cs.cs_spalloc(n, n, len(Ti), True, False)
    A.p, A.i, A.x = Tp.tolist(), Ti.tolist(), Tx.tolist()
    return cs.cs_pin(A)


def _solve(cs, case, A, B):
    X = cs.dvec(B if B.shape[1] > 1 else B[:, 0].copy())
    assert getattr(cs, "cs_" + case.kind)(A, X) is True
    return X.numpy().reshape(B.shape)


@pytest.mark.parametrize("cid", TC.IDS)
def test_what_ran_is_what_the_model_says_and_the_bytes_are_the_oracles(cs, cid):
    import _csx
    case = TC.BY_ID[cid]
    want_info, want_launches = TC.predicted(cid)
    ref, B = TC.oracle(cid), TC.rhs(case)
    with _options(case.options):
        A = _pinned(cs, TC.matrix(case))
        got = _solve(cs, case, A, B)
        plan = A._dev.plans[TC.KIND_ID[case.kind]]
        launches = _csx.tri_launches(plan)
        info = _csx.tri_route_info(plan, case.nrhs)
        assert _csx.tri_launches(plan) == launches                      # asking about the route launches nothing
        for key in _csx.TRI_ROUTE_INFO:
            assert info[key] == want_info[key], (cid, key, info, want_info)
        assert launches == want_launches, (cid, launches, want_launches)
        assert set(case.must) == set(launches)
        for r in range(case.nrhs):
            assert got[:, r].tobytes() == ref[:, r].tobytes(), (cid, "column", r)
        again = _solve(cs, case, A, B)
        assert again.tobytes() == got.tobytes(), cid
        want_launches = {k: v for k, v in want_launches.items() if k != "level_of"}     # the level of every row is kept
        assert _csx.tri_launches(plan) == want_launches, cid
    for alt in case.alt:
        with _options(dict(case.options, **alt)):
            A2 = _pinned(cs, TC.matrix(case))
            other = _solve(cs, case, A2, B)
            took = _csx.tri_route_info(A2._dev.plans[TC.KIND_ID[case.kind]], case.nrhs)
            assert took["route"] == TC.model(TC.matrix(case), case.kind, case.nrhs, dict(case.options, **alt))[0]["route"]
            assert other.tobytes() == got.tobytes(), (cid, alt)


def _one_per(key, needs):
    seen, out = set(), []
    for c in TC.CASES:
        k = key(c)
        if needs(c) and k not in seen and c.system not in TC.LARGE:
            seen.add(k)
            out.append(c.id)
    return out


NAN_CASES = ["wband60-lsolve-2", "wband60-utsolve-2", "col15360-usolve-2", "col15360-ltsolve-2", "malformed-lsolve-3"] + \
    _one_per(lambda c: tuple(c.must), lambda c: c.nrhs >= 3 and c.proper)


@pytest.mark.parametrize("cid", NAN_CASES)
def test_a_nan_stays_in_its_right_hand_side_column(cs, cid):
    case = TC.BY_ID[cid]
    ref = TC.oracle(cid)
    B = TC.rhs(case).copy()
    B[B.shape[0] // 3, 1] = np.nan
    with _options(case.options):
        got = _solve(cs, case, _pinned(cs, TC.matrix(case)), B)
    assert np.isnan(got[:, 1]).any()
    for r in range(case.nrhs):
        if r != 1:
            assert got[:, r].tobytes() == ref[:, r].tobytes(), (cid, r)


def test_the_nan_cases_cover_every_route():
    assert {TC.BY_ID[cid].route for cid in NAN_CASES} == {c.route for c in TC.CASES}


@pytest.mark.parametrize("cid", ["wband60-lsolve-2", "wband60-ltsolve-2"] + _one_per(lambda c: (c.route, c.kind in TC.PUSH), lambda c: c.proper))
def test_a_zero_pivot_is_refused(cs, cid):
    case = TC.BY_ID[cid]
    n, Tp, Ti, Tx = TC.matrix(case)
    Tx = Tx.copy()
    j = n // 2
    Tx[Tp[j] if case.kind in ("lsolve", "ltsolve") else Tp[j + 1] - 1] = 0.0
    with _options(case.options):
        A = _pinned(cs, (n, Tp, Ti, Tx))
        X = cs.dvec(TC.rhs(case))
        before = X.numpy().tobytes()
        with pytest.raises(ZeroDivisionError):
            getattr(cs, "cs_" + case.kind)(A, X)
        assert X.numpy().tobytes() == before


@pytest.mark.parametrize("pair", TC.LU_PAIRS, ids=[p[0] for p in TC.LU_PAIRS])
@pytest.mark.parametrize("trans", [False, True], ids=["lusol", "lusol_trans"])
def test_the_fused_lu_solve_and_the_four_steps(cs, pair, trans):
    import _csx
    name, sl, su, nrhs, fused = pair
    L, U = TC.to_matrix(TC._system(sl), "lsolve", 1), TC.to_matrix(TC._system(su), "usolve", 2)
    n = L[0]
    rng = np.random.default_rng(11)
    pinv, q = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    B = rng.uniform(-1.0, 1.0, (n, nrhs))
    ref = np.empty_like(B)
    for r in range(nrhs):
        if not trans:                                       # x(pinv) = b, L x = x, U x = x, b(q) = x
            x = np.empty(n)
            x[pinv] = B[:, r]
            x = CO.usolve(n, *U[1:], CO.lsolve(n, *L[1:], x))
            ref[q, r] = x
        else:                                               # y = b(q), U' y = y, L' y = y, x = y(pinv)
            y = CO.ltsolve(n, *L[1:], CO.utsolve(n, *U[1:], B[q, r]))
            ref[:, r] = y[pinv]
    AL, AU = _pinned(cs, L), _pinned(cs, U)
    kinds = (cs.TRI_UT, cs.TRI_LT) if trans else (cs.TRI_L, cs.TRI_U)
    first, second = (AU, AL) if trans else (AL, AU)
    p1, p2 = cs._plan(first._dev, kinds[0]), cs._plan(second._dev, kinds[1])
    hp, keep_p = cs._perm_handle(pinv.tolist(), n)
    hq, keep_q = cs._perm_handle(q.tolist(), n)
    try:
        X, W = cs.dvec(B), cs.dvec(n, nrhs)
        flag = _csx.C.c_int(-1)
        fn = _csx.lib().csx_lusol_solve_trans if trans else _csx.lib().csx_lusol_solve
        _csx.check(fn(p1, p2, hp, hq, X.handle, W.handle, nrhs, _csx.C.byref(flag)))
        assert bool(flag.value) is fused, (name, flag.value)
        got = X.numpy()
        for r in range(nrhs):
            assert got[:, r].tobytes() == ref[:, r].tobytes(), (name, r)
        for plan, kind in ((p1, kinds[0]), (p2, kinds[1])):             # a fused solve counts on both plans
            route = _csx.tri_route_info(plan, nrhs)["route"]
            assert (route == "Local") or not fused
            ran = _csx.tri_launches(plan)
            assert sum(ran.values()) == 1 and (not fused or set(ran) == {"local_fwd" if kind in (cs.TRI_L, cs.TRI_UT) else "local_bwd"})
    finally:
        for h in (keep_p, keep_q):
            if h is not None:
                _csx.free(h)


@pytest.mark.parametrize("rid", [r.id for r in TC.ROUNDING])
def test_the_rounding_equal_order_and_its_guard(cs, rid):
    """csx_tri_set_order(plan, 0): above PUSH_MAX_RHS right-hand sides a forest of components of at most 80 rows goes to the matrix
    cores and is held to tol.TRI_EPS_UNITS roundings of the terms of each component (the bound is 4 x the ORACLE's distance from a
    longdouble substitution, tools/measure_tri_edges.py); the guard passes, refuses (a component of 81 rows; diagonal tiles whose
    inverses grow) or meets a NaN, as the case says, and a refused plan gives the exact route's bytes."""
    import _csx
    import tol as TOL
    r = TC.ROUNDING_BY_ID[rid]
    T, B = TC.rounding_matrix(rid), TC.rounding_rhs(r)
    ref = TC.rounding_reference(rid)[0]
    lib, kind = _csx.lib(), TC.KIND_ID[r.kind]
    A = _pinned(cs, T)
    plan = cs._plan(A._dev, kind)
    _csx.check(lib.csx_tri_set_order(plan, 0))

    def run():
        X = cs.dvec(B)
        _csx.check(lib.csx_tri_solve(plan, X.handle, r.nrhs), "csx_tri_solve")
        return X.numpy().reshape(B.shape)

    got = run()
    want_info, want_launches, _ = TC.model(T, r.kind, r.nrhs, guard=r.guard)
    info, launches = _csx.tri_route_info(plan, r.nrhs), _csx.tri_launches(plan)
    for key in _csx.TRI_ROUTE_INFO:
        assert info[key] == want_info[key], (rid, key, info, want_info)
    assert launches == want_launches and info["route"] == r.route and info["guard"] == r.guard, (rid, info, launches)
    mc, growth = _csx.C.c_int32(-1), _csx.C.c_double(-1.0)
    _csx.check(lib.csx_tri_order_info(plan, mc, growth))
    assert bool(mc.value) is (r.guard == 1)
    if r.guard == 1:
        assert 1.0 <= growth.value <= 1e3
    elif r.guard == 3:
        assert np.isnan(growth.value)
    elif r.spoil == "growth":
        assert growth.value > 1e3
    if r.route == "Ragged":
        units = TC.eps_units(rid, got)
        print("%s: %.2f eps units of the terms (bound %.2f)" % (rid, units, TOL.TRI_EPS_UNITS))
        assert units <= TOL.TRI_EPS_UNITS, (rid, units)
        assert run().tobytes() == got.tobytes(), rid                      # the same bits every run
        return
    exact = _pinned(cs, T)                                                # a plan in the exact order
    X = cs.dvec(B)
    assert getattr(cs, "cs_" + r.kind)(exact, X) is True
    assert X.numpy().reshape(B.shape).tobytes() == got.tobytes(), rid
    assert np.array_equal(got, ref, equal_nan=True), rid
    if r.spoil != "nan":
        assert got.tobytes() == ref.tobytes(), rid


def pair_on_device(cs, name):
    """(the device's distance from the oracle in roundings of the terms, what was read back) of a case of tri_cases.PAIRS"""
    import _csx
    lib = _csx.lib()
    if name.startswith("lu_rag"):
        trans = name.endswith("trans")
        L, U, pinv, q, B = TC.lu_rag()
        n, nrhs = L[0], B.shape[1]
        ref, terms = np.empty_like(B), np.empty_like(B)
        if trans:                                           # y = b(q), U' y = y, L' y = y, x = y(pinv)
            X, _, T = TC.two_solves(U, "utsolve", L, "ltsolve", B[q])
            ref, terms = X[pinv], T[pinv]
        else:                                               # x(pinv) = b, L x = x, U x = x, b(q) = x
            Bp = np.empty_like(B)
            Bp[pinv] = B
            X, _, T = TC.two_solves(L, "lsolve", U, "usolve", Bp)
            ref[q], terms[q] = X, T
        AL, AU = _pinned(cs, L), _pinned(cs, U)
        kinds = (cs.TRI_UT, cs.TRI_LT) if trans else (cs.TRI_L, cs.TRI_U)
        first, second = (AU, AL) if trans else (AL, AU)
        plans = [cs._plan(first._dev, kinds[0]), cs._plan(second._dev, kinds[1])]
        for p in plans:
            _csx.check(lib.csx_tri_set_order(p, 0))
        hp, keep_p = cs._perm_handle(pinv.tolist(), n)
        hq, keep_q = cs._perm_handle(q.tolist(), n)
        try:
            D, W, flag = cs.dvec(B), cs.dvec(n, nrhs), _csx.C.c_int(-1)
            fn = lib.csx_lusol_solve_trans if trans else lib.csx_lusol_solve
            _csx.check(fn(plans[0], plans[1], hp, hq, D.handle, W.handle, nrhs, _csx.C.byref(flag)))
            got = D.numpy()
            seen = {"fused": flag.value, "launches": [_csx.tri_launches(p) for p in plans],
                    "info": [_csx.tri_route_info(p, nrhs) for p in plans]}
        finally:
            for h in (keep_p, keep_q):
                _csx.free(h)
        return TC.pair_units(got, ref, terms), seen
    (n, Ap, Ai, Ax), B = TC.chol_band()
    opts = {"tri.supernodes": 0, "tri.graph": 0}
    if name.endswith("levels"):
        opts["tri.columns"] = 0
    with _options(opts):
        F = cs.cholsol_factor(_pinned(cs, (n, Ap, Ai, Ax)), 0, exact=False)
        D = cs.dvec(B)
        assert F.solve(D) is True
        got = D.numpy()
        seen = {"launches": [_csx.tri_launches(F.plan_handle, cholsol=w) for w in (0, 1)],
                "info": [_csx.tri_route_info(F.plan_handle, B.shape[1], cholsol=w) for w in (0, 1)]}
    Lp = np.asarray(F.L.p, np.int32)
    Ld = (n, Lp, np.asarray(F.L.i[:Lp[n]], np.int32), np.asarray(F.L.x[:Lp[n]], np.float64))
    X, _, terms = TC.two_solves(Ld, "lsolve", Ld, "ltsolve", B)           # the oracle on the factor the device solved with
    return TC.pair_units(got, X, terms), seen


@pytest.mark.parametrize("name", TC.PAIRS)
def test_two_solves_in_a_rounding_equal_order(cs, name):
    """csx_lusol_solve and csx_lusol_solve_trans with both plans in the rounding-equal order fuse the two matrix-core sweeps and
    count them on both plans; cholsol_factor(exact=False) on a band runs L' on the rows of L (k_tri_wcolumns, mate), or with
    "tri.columns" = 0 both solves on a schedule taken from the elimination tree's hint with k_tri_chain in the relaxed order.
    Each within tol.TRI_EPS_UNITS of the oracle, in roundings of the terms of both substitutions (tri_cases.two_solves)."""
    import _csx
    import tol as TOL
    units, seen = pair_on_device(cs, name)
    print("%s: %.2f eps units of the terms (bound %.2f)" % (name, units, TOL.TRI_EPS_UNITS))
    fwd, bwd = seen["info"]
    if name.startswith("lu_rag"):
        assert seen["fused"] == 1
        assert seen["launches"] == [{"ragged": 1}, {"ragged": 1}]
        assert fwd["route"] == bwd["route"] == "Ragged" and fwd["guard"] == bwd["guard"] == 1
    elif name == "cholband-mate":
        assert (fwd["route"], fwd["mate"], fwd["schedule"]) == ("Columns", 0, 0)
        assert (bwd["route"], bwd["mate"], bwd["threads"], bwd["window"], bwd["schedule"]) == ("WColumns", 1, 256, 64, 0)
        assert bwd["band"] == TC.CHOL_BAND and fwd["col_state"] == 1
        assert seen["launches"] == [{"columns_l": 1}, {"wcolumns_256": 1}]
    else:
        for info in (fwd, bwd):
            assert (info["route"], info["schedule"], info["levels"], info["chain_ok"]) == ("Levels", 1, TC.CHOL_N, 0), info
        assert seen["launches"] == [{"chain": 1}, {"chain": 1}]           # the relaxed walker: the exact one needs chain_ok
    assert units <= TOL.TRI_EPS_UNITS, (name, units)
    lib, count = _csx.lib(), _csx.C.c_int32(-1)
    out = (_csx.C.c_int64 * 4)()
    assert lib.csx_cholsol_tri_launches(0, 0, out, 4, count) == _csx.EINVAL


def test_the_read_backs_refuse_what_is_no_plan(cs):
    import _csx
    case = TC.BY_ID["comps64-lsolve-1"]
    A = _pinned(cs, TC.matrix(case))
    _solve(cs, case, A, TC.rhs(case))
    plan, lib, count = A._dev.plans[cs.TRI_L], _csx.lib(), _csx.C.c_int32(-1)
    out = (_csx.C.c_int64 * 4)()
    assert lib.csx_tri_route_info(plan, 1, out, 4, count) == _csx.OK and count.value == len(_csx.TRI_ROUTE_INFO)
    assert lib.csx_tri_launches(plan, out, 4, count) == _csx.OK and count.value == len(_csx.TRI_LAUNCHES)
    assert lib.csx_tri_route_info(plan, 0, out, 4, count) == _csx.EINVAL
    assert lib.csx_tri_route_info(plan, 1, None, 4, count) == _csx.EINVAL
    assert lib.csx_tri_launches(plan, None, 4, count) == _csx.EINVAL
    assert lib.csx_tri_route_info(A._dev.handle, 1, out, 4, count) == _csx.EINVAL
    assert lib.csx_tri_launches(A._dev.handle, out, 4, count) == _csx.EINVAL
