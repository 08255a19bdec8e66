"""slusol_factor(...).batch() on the device on the cases of tests/slu_cases.py and the sizes of
tests/slu_batch_cases.py: every member's L.x / Ut.x and statistics byte-equal to the host rule (tests/slu_oracle.py); one walk of
the schedule whatever B is; a wide batch against the same values one by one, and twice; a member that breaks down (a zero or inf
pivot, a NaN) alone; the batched solves byte-equal to the single exact solver column by column, forward and transposed, on both
sides of every size limit; refactor of a batch; the factor it borrows left as it was; the ValueError / CSX_EINVAL cases.  The
rule of the sweeps is held to the reference's loops by tests/test_slu_batch_cpu.py."""
import numpy as np
import pytest

import slu_batch_cases as BC
import slu_cases as SC
import slu_oracle as SO
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

_SINGLES = {}   # (case, member) -> the single exact solver of that member: made once, only solved with


def _factor(cs, case, values=None, exact=None):
    return cs.slusol_factor(case.matrix(cs, case.x if values is None else values), case.order, case.perturb, case.match,
                            case.match_seed, exact)


def _single(cs, case, m):
    key = (case.name, m)
    if key not in _SINGLES:
        _SINGLES[key] = _factor(cs, case, BC.member(case, m), exact=True)
        assert _SINGLES[key] is not None
    return _SINGLES[key]


def _values_of(M):
    import _csx
    m, n, nnz, hv = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return x[:nnz]


def _member_is(batch, m, case, ref, info=None):
    """member m of the batch has the bytes (and the statistics) of ref = (Lx, Ux, (pos, neg, perturbed, breakdown))"""
    Lp = np.asarray(SO.pattern_of(case)[0])
    Lx, Ux, want = ref
    gl, gu = batch.member(m)
    assert gl.tobytes() == np.asarray(Lx).tobytes() and gu.tobytes() == np.asarray(Ux).tobytes(), m
    i = batch.info() if info is None else info
    assert (int(i["pos"][m]), int(i["neg"][m]), int(i["perturbed"][m]), int(i["breakdown"][m])) == tuple(want), m
    Lx, Ux = np.asarray(Lx), np.asarray(Ux)
    d = Ux[Lp[:-1]]
    off = np.ones(len(Lx), bool)
    off[Lp[:-1]] = False
    assert i["min_abs_d"][m] == np.min(np.abs(d)) and i["max_abs_d"][m] == np.max(np.abs(d))
    assert i["max_abs_l"][m] == (np.max(np.abs(Lx[off])) if off.any() else 0.0)
    assert i["max_abs_u"][m] == (np.max(np.abs(Ux[off])) if off.any() else 0.0)


def _host_rule(case, x):
    st, Lx, Ux, info = SO.host(case, x, SO.tau_of(case, x))
    assert st == 0
    return Lx, Ux, info


def _solves_are_the_single_solver(cs, case, batch, B, r, which=None):
    """every column of batch.solve, forward and transposed, has the bytes of the single exact solver of its member"""
    n, K = case.n, B * r
    R = SC.random_block(case, K)
    for trans in (False, True):
        dX = cs.dvec(R)
        assert batch.solve(dX, trans=trans) is True
        X = dX.numpy().reshape(n, K)
        for m in range(B) if which is None else which:
            S = _single(cs, case, m)
            for c in range(r):
                x = cs.dvec(np.ascontiguousarray(R[:, m * r + c]))
                assert S.solve(x, trans=trans) is True
                assert X[:, m * r + c].tobytes() == x.numpy().tobytes(), (trans, B, r, m, c)


@pytest.mark.parametrize("name", SC.NAMES)
def test_every_member_is_the_host_rule(cs, name):
    case = SC.BY_NAME[name]
    F = _factor(cs, case)
    batch = F.batch(BC.members(case, 3))
    assert batch.B == 3 and batch.ok.dtype == bool and batch.ok.tolist() == [True] * 3
    info, single = batch.info(), F.info()
    for m, which in enumerate(SC.VALUE_SETS):
        _member_is(batch, m, case, SO.reference(case, which), info)
    assert [info[k] for k in ("n", "lnz", "levels", "B")] == [single["n"], single["lnz"], single["levels"], 3]
    assert info["kernel_us"] > 0 and info["long_columns"].tolist() == [single["long_columns"]] * 3
    if case.perturb > 0.0:
        assert info["perturbed"].min() > 0        # per-member thresholds: tau[m] = perturb |A_m|_1


def test_the_three_forms_of_values(cs):
    case = SC.BY_NAME["west-nd"]
    F, V = _factor(cs, case), BC.members(case, 3)
    want = [SO.reference(case, which) for which in SC.VALUE_SETS]
    for values in (V, cs.dvec(V), [V[:, m].copy() for m in range(3)], [V[:, m].tolist() for m in range(3)]):
        batch = F.batch(values)
        for m in range(3):
            _member_is(batch, m, case, want[m])
    one = F.batch(cs.dvec(V[:, 1].copy()))         # a plain vector of nnz values: one member
    assert one.B == 1
    _member_is(one, 0, case, want[1])


@pytest.mark.parametrize("name", BC.LAUNCH_CASES)
def test_one_walk_whatever_b(cs, name):
    case = SC.BY_NAME[name]
    F = _factor(cs, case)
    single = F.info()
    assert single["launches"] == single["level_launches"] + single["run_launches"] >= 1
    for B in (1, 3, 65):
        batch = F.batch(BC.members(case, B))
        i = batch.info()
        assert batch.ok.all() and i["B"] == B
        assert (i["launches"], i["run_launches"], i["level_launches"]) == (single["launches"], single["run_launches"],
                                                                           single["level_launches"]), B
        _member_is(batch, B - 1, case, _host_rule(case, BC.member(case, B - 1)), i)
    assert F.info() == single                      # the factor's own counters are its own


def test_wide_batch(cs):
    case, B = SC.BY_NAME["grid24-shift"], 65
    F, V = _factor(cs, case), BC.members(case, B)
    batch = F.batch(V)
    assert batch.ok.all()
    info = batch.info()
    for m in (0, 63, 64):
        _member_is(batch, m, case, _host_rule(case, V[:, m]), info)
    first = [batch.member(m) for m in range(B)]
    for m in range(B):
        alone = F.batch(np.ascontiguousarray(V[:, m:m + 1]))
        gl, gu = alone.member(0)
        assert alone.ok.tolist() == [True] and gl.tobytes() == first[m][0].tobytes() and gu.tobytes() == first[m][1].tobytes(), m
    assert batch.refactor(V).all()                 # a second run: the same bytes
    again = F.batch(V)
    for m in range(B):
        for b2 in (batch, again):
            gl, gu = b2.member(m)
            assert gl.tobytes() == first[m][0].tobytes() and gu.tobytes() == first[m][1].tobytes(), m


@pytest.mark.parametrize("name", ["grid24-shift", "west", "saddle"])
def test_a_member_that_breaks_down_is_alone(cs, name):
    case = SC.BY_NAME[name]
    F = _factor(cs, case)
    r = 3
    R = SC.random_block(case, 3 * r)
    clean = F.batch(np.stack([case.x, case.A2[0]], axis=1))
    dC = cs.dvec(np.ascontiguousarray(R[:, list(range(r)) + list(range(2 * r, 3 * r))]))
    assert clean.solve(dC) is True
    C = dC.numpy().reshape(case.n, 2 * r)
    nan = case.x.copy()
    nan[len(nan) // 2] = np.nan
    for bad, at in ((case.breaking(*SO.first_pivot(case)), 0), (nan, None)):
        batch = F.batch(np.stack([case.x, bad, case.A2[0]], axis=1))
        assert batch.ok.tolist() == [True, False, True]
        i = batch.info()
        assert i["breakdown"][1] >= 0 and (at is None or i["breakdown"][1] == at)
        _member_is(batch, 0, case, SO.reference(case, "A"), i)
        _member_is(batch, 2, case, SO.reference(case, 0), i)
        dX = cs.dvec(R)
        assert batch.solve(dX) is True
        X = dX.numpy().reshape(case.n, 3 * r)
        assert np.isnan(X[:, r:2 * r]).all()
        assert X[:, :r].tobytes() == C[:, :r].tobytes() and X[:, 2 * r:].tobytes() == C[:, r:].tobytes()
    # a NaN or an inf in one member's right-hand side stays in that member's columns
    batch = F.batch(BC.members(case, 3))
    P = R.copy()
    P[0, r] = np.nan
    P[case.n - 1, r + 1] = np.inf
    for trans in (False, True):
        dX, dP = cs.dvec(R), cs.dvec(P)
        assert batch.solve(dX, trans=trans) is True and batch.solve(dP, trans=trans) is True
        X, Y = dX.numpy().reshape(case.n, 3 * r), dP.numpy().reshape(case.n, 3 * r)
        keep = [c for c in range(3 * r) if c not in (r, r + 1)]
        assert np.isfinite(X).all() and Y[:, keep].tobytes() == X[:, keep].tobytes()
        assert not np.isfinite(Y[:, r]).all() and not np.isfinite(Y[:, r + 1]).all()


@pytest.mark.parametrize("name", SC.NAMES)
def test_solves_are_the_single_exact_solver(cs, name):
    case = SC.BY_NAME[name]
    batch = _factor(cs, case).batch(BC.members(case, 3))
    assert batch.ok.all()
    for r in BC.R_SIZES:
        _solves_are_the_single_solver(cs, case, batch, 3, r)
    X = SC.random_block(case, 3)                   # a numpy block is overwritten too
    want = cs.dvec(X)
    assert batch.solve(want) is True and batch.solve(X) is True and X.tobytes() == want.numpy().tobytes()


def test_solves_of_wide_batches(cs):
    case = SC.BY_NAME["grid24"]
    F = _factor(cs, case)
    for B, r in ((65, 1),) + BC.WAVE_SHAPES:
        batch = F.batch(BC.members(case, B))
        assert batch.ok.all()
        _solves_are_the_single_solver(cs, case, batch, B, r)


def test_solves_at_the_workgroup_edges(cs):
    """a wide level on both sides of one solve workgroup; a walker level at exactly one pass of its waves and one more"""
    case = SC.BY_NAME["chains5"]
    F = _factor(cs, case)
    for B in BC.WIDE_EDGE_B:
        batch = F.batch(BC.members(case, B))
        assert batch.ok.all() and batch.info()["level_launches"] == 3
        _solves_are_the_single_solver(cs, case, batch, B, 1)
    case = SC.BY_NAME["chains4"]
    batch = _factor(cs, case).batch(BC.members(case, 2))
    assert batch.ok.all() and batch.info()["run_launches"] == 1
    for r in BC.RUN_EDGE_R:
        _solves_are_the_single_solver(cs, case, batch, 2, r)


@pytest.mark.parametrize("name", ["grid24-shift", "west-nd", "saddle"])
def test_refactor_of_a_batch(cs, name):
    case = SC.BY_NAME[name]
    F = _factor(cs, case)
    batch = F.batch(np.stack([case.x, case.breaking(*SO.first_pivot(case)), case.A2[0]], axis=1))
    assert batch.ok.tolist() == [True, False, True]
    ok = batch.refactor([case.A2[1], case.x, case.A2[0]])
    assert ok is batch.ok and ok.tolist() == [True] * 3          # the member that failed has recovered
    info = batch.info()
    for m, which in enumerate((1, "A", 0)):
        _member_is(batch, m, case, SO.reference(case, which), info)
    with pytest.raises(ValueError):
        batch.refactor(BC.members(case, 2))                       # B is fixed
    with pytest.raises(ValueError):
        batch.refactor(BC.members(case, 3)[:-1])
    for m, which in enumerate((1, "A", 0)):
        _member_is(batch, m, case, SO.reference(case, which))     # ... and a refused refactor changed nothing


def test_the_factor_is_not_disturbed(cs):
    case = SC.BY_NAME["grid24-shift"]
    F = _factor(cs, case)
    L0, U0, info0 = _values_of(F.factors.L).tobytes(), _values_of(F.factors.U).tobytes(), F.info()
    b = SC.rhs(case, 1)[0].tolist()
    x0 = list(b)
    assert F.solve(x0) is True
    batch = F.batch(np.stack([case.A2[0], case.breaking(*SO.first_pivot(case)), case.A2[1]], axis=1))
    assert batch.ok.tolist() == [True, False, True]
    assert _values_of(F.factors.L).tobytes() == L0 and _values_of(F.factors.U).tobytes() == U0 and F.info() == info0
    x1 = list(b)
    assert F.solve(x1) is True and x1 == x0
    assert F.refactor(case.A2[1]) is True
    assert _values_of(F.factors.L).tobytes() == SO.reference(case, 1)[0].tobytes()
    assert _values_of(F.factors.U).tobytes() == SO.reference(case, 1)[1].tobytes()
    _member_is(batch, 0, case, SO.reference(case, 0))
    _member_is(batch, 2, case, SO.reference(case, 1))
    assert F.refactor(case.breaking(*SO.first_pivot(case))) is False
    _member_is(batch, 0, case, SO.reference(case, 0))


def test_the_most_members(cs):
    case = SC.BY_NAME["one"]
    F = _factor(cs, case)
    V = (-3.0 * (1.0 + np.arange(BC.MAX_MEMBERS))).reshape(1, BC.MAX_MEMBERS)
    batch = F.batch(V)
    assert batch.B == BC.MAX_MEMBERS and batch.ok.all()
    for m in (0, 1, BC.MAX_MEMBERS - 1):
        Lx, Ux = batch.member(m)
        assert Lx.tolist() == [1.0] and Ux.tolist() == [V[0, m]]
    X = np.ones((1, BC.MAX_MEMBERS))
    assert batch.solve(X) is True and X.tobytes() == (1.0 / V).tobytes()
    with pytest.raises(ValueError):
        F.batch(np.ones((1, BC.MAX_MEMBERS + 1)))


def test_a_freed_factor_is_refused(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    case = SC.BY_NAME["one"]
    n, V = case.n, BC.members(case, 3)
    dV, out, ok = cs.dvec(V), _csx.new_handle(), (C.c_int * 3)()
    # a factor made and freed at the ABI (natural order: the one column a root), its batch outliving it
    hF, one = _csx.new_handle(), C.c_int(0)
    parent, cp = np.full(n, -1, np.int32), np.arange(n + 1, dtype=np.int32)
    with cs._Resident(case.matrix(cs)) as dA:
        _csx.check(lib.csx_slu_factor(dA.handle, _csx.pi(parent), _csx.pi(cp), None, None, 0.0, hF, one), "csx_slu_factor")
    assert one.value == 1
    assert lib.csx_slu_batch_factor(hF, dV.handle, 3, None, out, ok) == _csx.OK and out.value and list(ok) == [1, 1, 1]
    lx, ux = np.zeros(n), np.zeros(n)
    assert lib.csx_slu_batch_member(out, 2, _csx.pd(lx), _csx.pd(ux)) == _csx.OK
    assert lx.tolist() == [1.0] and ux.tobytes() == V[:, 2].tobytes()
    _csx.free(hF)
    shared, per = (C.c_int64 * 8)(), (C.c_int64 * 15)()
    dX = cs.dvec(np.zeros((n, 3)))
    for call in (lambda: lib.csx_slu_batch_refactor(out, dV.handle, None, ok), lambda: lib.csx_slu_batch_solve(out, dX.handle, 1, 0),
                 lambda: lib.csx_slu_batch_info(out, shared, per), lambda: lib.csx_slu_batch_stats(out, _csx.pd(np.zeros(12))),
                 lambda: lib.csx_slu_batch_member(out, 0, _csx.pd(lx), _csx.pd(ux))):
        assert call() == _csx.EINVAL and b"freed" in lib.csx_last_error()
    again = _csx.new_handle()
    assert lib.csx_slu_batch_factor(hF, dV.handle, 3, None, again, ok) == _csx.EINVAL and again.value == 0
    _csx.free(out)


def test_bad_arguments(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    case = SC.BY_NAME["grid24-shift"]
    nnz, n = len(case.x), case.n
    F = _factor(cs, case)
    V = BC.members(case, 3)
    for values in (V[:-1], np.zeros((nnz, 0)), [], V[:, 0].tolist(), cs.dvec(V[:-1]), np.zeros((nnz + 1, 2))):
        with pytest.raises(ValueError):
            F.batch(values)
    with pytest.raises(ValueError):
        F.batch(V, perturb=-1.0)
    batch = F.batch(V)
    for X in (cs.dvec(np.zeros((n, 2))), cs.dvec(np.zeros((n + 1, 3))), cs.dvec(np.zeros((n, 4))), [0.0] * (3 * n)):
        with pytest.raises(ValueError):
            batch.solve(X)
    for m in (-1, 3):
        with pytest.raises(ValueError):
            batch.member(m)
    # the C ABI
    assert lib.csx_slu_batch_limits(None) == _csx.EINVAL
    dV, small = cs.dvec(V), cs.dvec(V[:-1])
    hB, hF, ok, out = batch._h, batch._hF, (C.c_int * 3)(), _csx.new_handle()
    tau = np.zeros(3)
    assert lib.csx_slu_batch_factor(hF, dV.handle, 3, _csx.pd(tau), out, ok) == _csx.OK and out.value and list(ok) == [1, 1, 1]
    _csx.free(out)
    out = _csx.new_handle()
    for args in ((hB, dV.handle, 3, None, out, ok),                      # not a factor
                 (hF, hF, 3, None, out, ok),                             # not a vector
                 (hF, small.handle, 3, None, out, ok),                   # too short for nnz x B
                 (hF, dV.handle, 0, None, out, ok), (hF, dV.handle, -1, None, out, ok),
                 (hF, dV.handle, BC.MAX_MEMBERS + 1, None, out, ok),
                 (hF, dV.handle, 3, None, None, ok), (hF, dV.handle, 3, None, out, None),
                 (hF, dV.handle, 3, _csx.pd(np.array([0.0, -1.0, 0.0])), out, ok),
                 (hF, dV.handle, 3, _csx.pd(np.array([0.0, 0.0, np.nan])), out, ok)):
        assert lib.csx_slu_batch_factor(*args) == _csx.EINVAL, args[2:4]
        assert args[4] is None or out.value == 0
    assert lib.csx_slu_batch_factor(hF, dV.handle, BC.MAX_MEMBERS + 1, None, out, ok) == _csx.EINVAL
    assert b"members" in lib.csx_last_error()                             # refused with a text, not split
    assert lib.csx_slu_batch_refactor(hF, dV.handle, None, ok) == _csx.EINVAL
    assert lib.csx_slu_batch_refactor(hB, small.handle, None, ok) == _csx.EINVAL
    assert lib.csx_slu_batch_refactor(hB, dV.handle, None, None) == _csx.EINVAL
    norms = np.zeros(3)
    assert lib.csx_slu_batch_norm1(hB, dV.handle, 3, _csx.pd(norms)) == _csx.EINVAL
    assert lib.csx_slu_batch_norm1(hF, small.handle, 3, _csx.pd(norms)) == _csx.EINVAL
    assert lib.csx_slu_batch_norm1(hF, dV.handle, 0, _csx.pd(norms)) == _csx.EINVAL
    assert lib.csx_slu_batch_norm1(hF, dV.handle, 3, None) == _csx.EINVAL
    assert lib.csx_slu_batch_norm1(hF, dV.handle, 3, _csx.pd(norms)) == _csx.OK
    assert norms.tolist() == [SO.norm1(case, V[:, m]) for m in range(3)]
    dX = cs.dvec(np.zeros((n, 3)))
    assert lib.csx_slu_batch_solve(hF, dX.handle, 1, 0) == _csx.EINVAL
    assert lib.csx_slu_batch_solve(hB, dX.handle, 0, 0) == _csx.EINVAL
    assert lib.csx_slu_batch_solve(hB, dX.handle, 2, 0) == _csx.EINVAL      # n x 3 doubles are not n x 6
    assert lib.csx_slu_batch_solve(hB, hF, 1, 0) == _csx.EINVAL
    shared, per, st = (C.c_int64 * 8)(), (C.c_int64 * 15)(), np.zeros(12)
    assert lib.csx_slu_batch_info(hF, shared, per) == _csx.EINVAL and lib.csx_slu_batch_info(hB, None, per) == _csx.EINVAL
    assert lib.csx_slu_batch_info(hB, shared, None) == _csx.EINVAL
    assert lib.csx_slu_batch_stats(hF, _csx.pd(st)) == _csx.EINVAL and lib.csx_slu_batch_stats(hB, None) == _csx.EINVAL
    lx = np.zeros(batch.info()["lnz"])
    assert lib.csx_slu_batch_member(hB, 3, _csx.pd(lx), _csx.pd(lx)) == _csx.EINVAL
    assert lib.csx_slu_batch_member(hB, -1, _csx.pd(lx), _csx.pd(lx)) == _csx.EINVAL
    assert lib.csx_slu_batch_member(hB, 0, None, _csx.pd(lx)) == _csx.EINVAL
    assert lib.csx_slu_batch_member(hF, 0, _csx.pd(lx), _csx.pd(lx)) == _csx.EINVAL
    # none of it changed the batch
    for m, which in enumerate(SC.VALUE_SETS):
        _member_is(batch, m, case, SO.reference(case, which))
