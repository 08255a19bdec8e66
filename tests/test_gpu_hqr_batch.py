"""hqrsol_factor(...).batch() on the device on the cases of tests/hqr_cases.py and the sizes of
tests/hqr_batch_cases.py: every member's V.x / R.x / beta byte-equal to csx_hqr_host on the solver's own analysis and its
statistics equal to the single factor refactored to that member; the three forms of `values`, a wide A through the storage-order
map; one walk of the schedule whatever B is; a wide batch against the same values one by one, and twice; a member that breaks
down alone; the batched solves byte-equal to the single solver's list solves column by column, in both sequences and on both
sides of every size limit, and to the restated level solve; the factor it borrows left as it was; the ValueError / CSX_EINVAL
cases.  The rule of the level solve is held to the reference's loops by tests/test_hqr_batch_cpu.py."""
import math

import numpy as np
import pytest

import hqr_batch_cases as BC
import hqr_cases as HC
import hqr_oracle as HO
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

SOLVABLE = [c.name for c in HC.CASES if c.solvable]
_SINGLES = {}   # (case, member) -> hqrsol_factor of that member alone: made once, only solved with


def _factor(cs, case, values=None):
    return cs.hqrsol_factor(case.matrix(cs, case.x if values is None else values), case.order)


def _single(cs, case, m):
    key = (case.name, m)
    if key not in _SINGLES:
        _SINGLES[key] = _factor(cs, case, BC.member(case, m))
        assert _SINGLES[key] is not None
    return _SINGLES[key]


def _analysis(case, F):
    """the solver's own analysis in the shape of hqr_cases.Analysis (the factored matrix is the case's, the column order and the
    rest are the product's)"""
    S, mine = HC.Analysis(), case.analysis
    S.m, S.n, S.p, S.i, S.perm = mine.m, mine.n, mine.p, mine.i, mine.perm
    sym = F.symbolic
    S.q = None if sym.q is None else np.asarray(sym.q, np.int32)
    S.parent, S.pinv, S.leftmost = np.asarray(sym.parent, np.int32), np.asarray(sym.pinv[:S.m], np.int32), np.asarray(sym.leftmost, np.int32)
    S.m2, S.vnz, S.rnz = sym.m2, sym.lnz, sym.unz
    return S


def _host(case, F, x):
    out = HO.host(case, x, S=_analysis(case, F))
    assert out[0] == 0
    return out[1:]


def _download(M):
    import _csx
    m, n, nnz, hv = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return x[:nnz]


def _member_is(batch, m, ref):
    """member m of the batch has the bytes of ref = csx_hqr_host's (Vp, Vi, Vx, Rp, Ri, Rx, beta)"""
    Vx, Rx, beta = batch.member(m)
    assert Vx.tobytes() == ref[2].tobytes() and Rx.tobytes() == ref[5].tobytes() and beta.tobytes() == ref[6].tobytes(), m


def _shapes(case, trans):
    """(second, rows_in, rows_out) of A x = b (trans: A' x = b) on the case"""
    second = trans or case.m < case.n
    rows_in, rows_out = (case.n, case.m) if trans else (case.m, case.n)
    return second, rows_in, rows_out


def _block(case, K, rows):
    return np.ascontiguousarray(HC.rhs(case, K, rows).T)


def _list_solve(F, col, rows_out, trans):
    x = col.tolist() + [0.0] * max(rows_out - len(col), 0)
    assert F.solve(x, trans=trans) is True
    return np.asarray(x[:rows_out])


def _solves_are_the_single_solver(cs, case, batch, B, r, trans=False, single=None):
    """every column of batch.solve has the bytes of the single solver's list solve of its member.  single: None (a fresh
    hqrsol_factor per member, kept) or one factor of the case that is REFACTORED to each member in turn -- byte-equal to a fresh
    one (tests/test_gpu_hqr.py), and what keeps a wide batch to a few seconds"""
    _, rows_in, rows_out = _shapes(case, trans)
    K = B * r
    R = _block(case, K, rows_in)
    dX = cs.dvec(R)
    out = batch.solve(dX, trans=trans)
    assert isinstance(out, cs.dvec) and (out.n, out.k) == (rows_out, K)
    assert dX.numpy().reshape(R.shape).tobytes() == R.tobytes()          # X is left as it was
    X = out.numpy().reshape(rows_out, K)
    for m in range(B):
        if single is None:
            S = _single(cs, case, m)
        else:
            S = single
            assert S.refactor(BC.member(case, m)) is True
        for c in range(m * r, (m + 1) * r):
            assert X[:, c].tobytes() == _list_solve(S, R[:, c], rows_out, trans).tobytes(), (B, r, m, c)
    return R, X


@pytest.mark.parametrize("name", HC.NAMES)
def test_every_member_is_the_host_rule(cs, name):
    case = HC.BY_NAME[name]
    F = _factor(cs, case)
    V = BC.members(case, 3)
    batch = F.batch(V)
    assert batch.B == 3 and batch.ok.dtype == bool and batch.ok.tolist() == [True] * 3
    info, single = batch.info(), F.info()
    assert [info[k] for k in ("m", "n", "m2", "vnz", "rnz", "levels", "B")] == [single[k] for k in ("m", "n", "m2", "vnz", "rnz", "levels")] + [3]
    assert (info["launches"], info["level_launches"], info["run_launches"]) == (single["launches"], single["level_launches"],
                                                                              single["run_launches"])
    assert info["kernel_us"] > 0
    G = _factor(cs, case)                                    # the single factor, refactored to every member in turn
    for m in range(3):
        ref = _host(case, F, V[:, m])
        _member_is(batch, m, ref)
        assert G.refactor(V[:, m].copy()) is True
        g = G.info()
        for k in ("breakdown", "long_columns", "zero_diagonals", "min_abs_r", "max_abs_r"):
            assert info[k][m] == g[k], (k, m)
        d = np.abs(ref[5][ref[3][1:] - 1])
        assert info["zero_diagonals"][m] == int(np.sum(d == 0.0)) and info["min_abs_r"][m] == d.min() and info["max_abs_r"][m] == d.max()


@pytest.mark.parametrize("name", ["grid24-shift", "lp_afiro"])
def test_the_three_forms_of_values(cs, name):
    """lp_afiro is wide: the factored matrix is its transpose, and the rows of the block go through the storage-order map -- in
    numpy for an array or a list, on the device for a dvec"""
    case = HC.BY_NAME[name]
    F, V = _factor(cs, case), BC.members(case, 3)
    assert F.info()["transposed"] is (name == "lp_afiro")
    want = [_host(case, F, V[:, m]) for m in range(3)]
    for values in (V, cs.dvec(V), [V[:, m].copy() for m in range(3)], [V[:, m].tolist() for m in range(3)]):
        batch = F.batch(values)
        assert batch.ok.all()
        for m in range(3):
            _member_is(batch, m, want[m])
        assert batch.refactor(values).all()
        _member_is(batch, 2, want[2])
    one = F.batch(cs.dvec(V[:, 1].copy()))         # a plain vector of nnz values: one member
    assert one.B == 1
    _member_is(one, 0, want[1])


@pytest.mark.parametrize("name", BC.LAUNCH_CASES)
def test_one_walk_whatever_b(cs, name):
    case = HC.BY_NAME[name]
    F = _factor(cs, case)
    single = F.info()
    assert single["launches"] == single["level_launches"] + single["run_launches"] >= 1
    if name == "bidiagonal":
        assert (single["levels"], single["run_launches"], single["level_launches"]) == (257, 2, 0)      # the walker cut
    for B in (1, 3, 65):
        batch = F.batch(BC.members(case, B))
        i = batch.info()
        assert batch.ok.all() and i["B"] == B
        assert (i["launches"], i["run_launches"], i["level_launches"]) == (single["launches"], single["run_launches"],
                                                                           single["level_launches"]), B
        _member_is(batch, B - 1, _host(case, F, BC.member(case, B - 1)))
    assert F.info() == single                      # the factor's own counters are its own


def test_wide_batch(cs):
    case, B = HC.BY_NAME["grid24-shift"], 65
    F, V = _factor(cs, case), BC.members(case, B)
    batch = F.batch(V)
    assert batch.ok.all()
    for m in (0, 63, 64):
        _member_is(batch, m, _host(case, F, V[:, m]))
    first = [batch.member(m) for m in range(B)]
    for m in range(B):
        alone = F.batch(np.ascontiguousarray(V[:, m:m + 1]))
        got = alone.member(0)
        assert alone.ok.tolist() == [True] and all(a.tobytes() == b.tobytes() for a, b in zip(got, first[m])), m
    assert batch.refactor(V).all()                 # a second run: the same bytes
    again = F.batch(V)
    for m in range(B):
        for b2 in (batch, again):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(b2.member(m), first[m])), m


def test_a_member_that_breaks_down_is_alone(cs):
    case, r = HC.BY_NAME["grid24-shift"], 3
    F = _factor(cs, case)
    S = _analysis(case, F)
    bad = case.breaking(0 if S.q is None else int(S.q[0]))
    R = _block(case, 3 * r, case.m)
    clean = F.batch(np.stack([case.x, case.A2[0]], axis=1))
    assert clean.ok.all()
    C = clean.solve(np.ascontiguousarray(R[:, list(range(r)) + list(range(2 * r, 3 * r))]))
    batch = F.batch(np.stack([case.x, bad, case.A2[0]], axis=1))
    assert batch.ok.tolist() == [True, False, True]
    i = batch.info()
    assert i["breakdown"].tolist() == [-1, 0, -1]
    _member_is(batch, 0, _host(case, F, case.x))
    _member_is(batch, 2, _host(case, F, case.A2[0]))
    logs = batch.logabsdet()
    assert np.isnan(logs[1]) and np.isfinite(logs[[0, 2]]).all()
    assert logs[0] == F.logabsdet() and logs[2] == _single(cs, case, 1).logabsdet()
    for trans in (False, True):
        X = batch.solve(R, trans=trans)
        assert np.isnan(X[:, r:2 * r]).all()
        if not trans:
            assert X[:, :r].tobytes() == C[:, :r].tobytes() and X[:, 2 * r:].tobytes() == C[:, r:].tobytes()
        else:
            assert np.isfinite(X[:, :r]).all() and np.isfinite(X[:, 2 * r:]).all()
    # refactor with mended values: the member recovers
    ok = batch.refactor([case.A2[1], case.x, case.A2[0]])
    assert ok is batch.ok and ok.tolist() == [True] * 3
    for m, which in enumerate((1, "A", 0)):
        _member_is(batch, m, _host(case, F, case.values(which)))
    assert np.isfinite(batch.solve(R)).all() and np.isfinite(batch.logabsdet()).all()


def test_a_nan_in_a_right_hand_side_stays_in_its_column(cs):
    case, r = HC.BY_NAME["grid24-shift"], 3
    batch = _factor(cs, case).batch(BC.members(case, 3))
    R = _block(case, 3 * r, case.m)
    P = R.copy()
    P[0, r] = np.nan
    P[case.n - 1, r + 1] = np.inf
    keep = [c for c in range(3 * r) if c not in (r, r + 1)]
    for trans in (False, True):
        X, Y = batch.solve(R, trans=trans), batch.solve(P, trans=trans)
        assert np.isfinite(X).all() and Y[:, keep].tobytes() == X[:, keep].tobytes()
        assert not np.isfinite(Y[:, r]).all() and not np.isfinite(Y[:, r + 1]).all()


@pytest.mark.parametrize("name", SOLVABLE)
def test_solves_are_the_single_solver(cs, name):
    """first sequence on the tall and the square cases, second on lp_afiro and with trans=True on the square ones; r = 1 and 3;
    a numpy block and a dvec give the same bytes; and every column of r = 1 is the restated level solve"""
    case = HC.BY_NAME[name]
    F = _factor(cs, case)
    batch = F.batch(BC.members(case, 3))
    assert batch.ok.all()
    S = _analysis(case, F)
    for trans in ((False, True) if name in HC.SQUARE else (False,)):
        second, rows_in, rows_out = _shapes(case, trans)
        for r in BC.R_SIZES:
            R, X = _solves_are_the_single_solver(cs, case, batch, 3, r, trans)
            got = batch.solve(R.copy(), trans=trans)             # a numpy block: a new array, the same bytes
            assert isinstance(got, np.ndarray) and got.shape == (rows_out, 3 * r) and got.tobytes() == X.tobytes()
            if r == 1:
                for m in range(3):
                    ref = _host(case, F, BC.member(case, m))
                    assert X[:, m].tobytes() == BC.level_solve(S, ref, R[:, m], second).tobytes(), (trans, m)
    assert (case.m < case.n) == (name == "lp_afiro")


def test_a_sweep_is_the_schedule_for_any_b(cs):
    """the launches of a batched solve: two permutations, csx_happly's launches for one member, len(schedule) for the sweep"""
    for name in ("grid24-shift", "bidiagonal", "blocks"):
        case = HC.BY_NAME[name]
        F = _factor(cs, case)
        Vp, Vi, _, _ = HO.symbolic(_analysis(case, F))
        nlev = len(BC.house_levels(Vp, Vi, F.symbolic.m2))
        reflections = 1 if (nlev == case.analysis.n or nlev > BC.MAX_LEVELS) else nlev
        assert (reflections == 1) is (name == "bidiagonal")
        for B in (1, 3, 65):
            batch = F.batch(BC.members(case, B))
            for trans in ((False, True) if name in HC.SQUARE else (False,)):
                batch.solve(cs.dvec(_block(case, B, case.n if trans else case.m)), trans=trans)
                assert batch.info()["solve_launches"] == 2 + reflections + F.info()["launches"], (name, B, trans)


def test_solves_of_wide_batches(cs):
    """K = B r = 64 and 65, the reflection kernel's lane chunk, in both sequences"""
    case = HC.BY_NAME["west-nd"]
    F, G = _factor(cs, case), _factor(cs, case)
    for B, r in BC.WAVE_SHAPES:
        batch = F.batch(BC.members(case, B))
        assert batch.ok.all()
        for trans in (False, True):
            _solves_are_the_single_solver(cs, case, batch, B, r, trans, single=G)
    wide = HC.BY_NAME["lp_afiro"]
    F, G = _factor(cs, wide), _factor(cs, wide)
    batch = F.batch(BC.members(wide, BC.LANES + 1))
    _solves_are_the_single_solver(cs, wide, batch, BC.LANES + 1, 1, single=G)


@pytest.mark.parametrize("name", BC.EDGE_CASES)
def test_solves_at_the_workgroup_edges(cs, name):
    """K at SOLVE_THREADS - 1, SOLVE_THREADS, + 1 and (row, right-hand side) pairs at RUN_WAVES - 1, RUN_WAVES, + 1: on the two
    walker cases, and on chains5, whose levels go to the wide kernel that SOLVE_THREADS cuts"""
    case = HC.BY_NAME[name]
    F, G = _factor(cs, case), _factor(cs, case)
    shapes = BC.THREAD_SHAPES + BC.RUN_SHAPES + tuple((2, r) for r in BC.RUN_EDGE_R)
    for B, r in shapes:
        batch = F.batch(BC.members(case, B))
        i = batch.info()
        assert batch.ok.all() and (i["run_launches"], i["level_launches"]) == ((0, 3) if name == "chains5" else (1, 0))
        _solves_are_the_single_solver(cs, case, batch, B, r, single=G)


def test_a_zero_on_the_diagonal_of_r_is_no_breakdown(cs):
    case = HC.BY_NAME["diagonal"]
    F = _factor(cs, case)
    batch = F.batch(BC.members(case, 3))
    assert batch.ok.all() and batch.info()["zero_diagonals"].tolist() == [1, 1, 1]
    assert batch.logabsdet().tolist() == [-np.inf] * 3
    R = _block(case, 3, case.m)
    for trans in (False, True):                     # what the single solver gives: the reference's division by zero
        with pytest.raises(ZeroDivisionError):
            F.solve(R[:, 0].tolist(), trans=trans)
        with pytest.raises(ZeroDivisionError):
            batch.solve(R, trans=trans)
    import _csx
    assert b"member 0" in _csx.lib().csx_last_error()
    V = BC.members(case, 3)                         # one member still singular: the same; none: the single solver's bytes
    V[2, :2] = 1.0
    assert batch.refactor(V).all() and batch.info()["zero_diagonals"].tolist() == [0, 0, 1]
    with pytest.raises(ZeroDivisionError):
        batch.solve(R)
    V[2, 2] = -1.0
    assert batch.refactor(V).all() and batch.info()["zero_diagonals"].tolist() == [0, 0, 0]
    G = _factor(cs, case, V[:, 0].copy())
    for trans in (False, True):
        X = batch.solve(R, trans=trans)
        for m in range(3):
            assert G.refactor(V[:, m].copy()) is True
            assert X[:, m].tobytes() == _list_solve(G, R[:, m], case.n, trans).tobytes(), (trans, m)


def test_the_factor_is_not_disturbed(cs):
    case = HC.BY_NAME["grid24-shift"]
    F = _factor(cs, case)
    V0, R0, B0, info0 = _download(F.factors.L).tobytes(), _download(F.factors.U).tobytes(), list(F.factors.B), F.info()
    b = HC.rhs(case, 1)[0].tolist()
    x0 = list(b)
    assert F.solve(x0) is True
    S = _analysis(case, F)
    bad = case.breaking(0 if S.q is None else int(S.q[0]))
    batch = F.batch(np.stack([case.A2[0], bad, case.A2[1]], axis=1))
    assert batch.ok.tolist() == [True, False, True]
    assert batch.refactor(np.stack([case.A2[1], bad, case.A2[0]], axis=1)).tolist() == [True, False, True]
    for trans in (False, True):
        batch.solve(cs.dvec(_block(case, 3, case.m)), trans=trans)
    assert _download(F.factors.L).tobytes() == V0 and _download(F.factors.U).tobytes() == R0 and list(F.factors.B) == B0
    assert np.asarray(F.factors.B).tobytes() == _host(case, F, case.x)[6].tobytes() and F.info() == info0
    x1 = list(b)
    assert F.solve(x1) is True and x1 == x0
    assert F.refactor(case.A2[1]) is True          # ... and the batch is not disturbed by the factor's own work
    _member_is(batch, 0, _host(case, F, case.A2[1]))
    _member_is(batch, 2, _host(case, F, case.A2[0]))
    assert F.refactor(bad) is False
    _member_is(batch, 0, _host(case, F, case.A2[1]))


def test_the_most_members(cs):
    import _csx
    case = HC.BY_NAME["one"]
    F = _factor(cs, case)
    V = (-3.0 * (1.0 + np.arange(BC.MAX_MEMBERS))).reshape(1, BC.MAX_MEMBERS)
    batch = F.batch(V)
    assert BC.MAX_MEMBERS == 65535 and batch.B == BC.MAX_MEMBERS and batch.ok.all()
    for m in (0, 1, BC.MAX_MEMBERS - 1):
        Vx, Rx, beta = batch.member(m)
        assert Vx.tolist() == [1.0] and Rx.tolist() == [-V[0, m]] and beta.tolist() == [2.0]
    X = batch.solve(np.ones((1, BC.MAX_MEMBERS)))
    assert X.tobytes() == (1.0 / V).tobytes()
    more = np.ones((1, BC.MAX_MEMBERS + 1))
    with pytest.raises(ValueError):
        F.batch(more)
    lib, C = _csx.lib(), _csx.C
    out, ok, dM = _csx.new_handle(), (C.c_int * (BC.MAX_MEMBERS + 1))(), cs.dvec(more)
    assert lib.csx_hqr_batch_factor(F.factors.L._dev.handle, dM.handle, 3, out, ok) == _csx.EINVAL      # not a factor
    assert lib.csx_hqr_batch_factor(batch._hF, dM.handle, BC.MAX_MEMBERS + 1, out, ok) == _csx.EINVAL
    assert out.value == 0 and b"members" in lib.csx_last_error()          # refused with a text, not split


def test_a_freed_factor_is_refused(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    case = HC.BY_NAME["chains5"]
    S = _analysis(case, _factor(cs, case))
    V = BC.members(case, 3)
    dV, out, ok = cs.dvec(V), _csx.new_handle(), (C.c_int * 3)()
    # a factor made and freed at the ABI, its batch outliving it
    hF, one = _csx.new_handle(), C.c_int(0)
    with cs._Resident(case.matrix(cs)) as dA:
        _csx.check(lib.csx_hqr_factor(dA.handle, _csx.pi(S.q), _csx.pi(S.parent), _csx.pi(S.pinv), _csx.pi(S.leftmost), S.m2, hF, one),
                   "csx_hqr_factor")
    assert one.value == 1
    assert lib.csx_hqr_batch_factor(hF, dV.handle, 3, out, ok) == _csx.OK and out.value and list(ok) == [1, 1, 1]
    ref = HO.host(case, V[:, 2], S=S)
    vx, rx, beta = np.zeros(S.vnz), np.zeros(S.rnz), np.zeros(S.n)
    assert lib.csx_hqr_batch_member(out, 2, _csx.pd(vx), _csx.pd(rx), _csx.pd(beta)) == _csx.OK
    assert vx.tobytes() == ref[3].tobytes() and rx.tobytes() == ref[6].tobytes() and beta.tobytes() == ref[7].tobytes()
    _csx.free(hF)
    shared, per = (C.c_int64 * 12)(), (C.c_int64 * 9)()
    dX, dY = cs.dvec(np.zeros((case.m, 3))), cs.dvec(np.zeros((case.n, 3)))
    for call in (lambda: lib.csx_hqr_batch_info(out, shared, per), lambda: lib.csx_hqr_batch_solve(out, dX.handle, dY.handle, 1, 0),
                 lambda: lib.csx_hqr_batch_refactor(out, dV.handle, ok), lambda: lib.csx_hqr_batch_r_diag(out, _csx.pd(np.zeros(3 * case.n))),
                 lambda: lib.csx_hqr_batch_stats(out, _csx.pd(np.zeros(6))),
                 lambda: lib.csx_hqr_batch_member(out, 0, _csx.pd(vx), _csx.pd(rx), _csx.pd(beta))):
        assert call() == _csx.EINVAL and b"freed" in lib.csx_last_error()
    again = _csx.new_handle()
    assert lib.csx_hqr_batch_factor(hF, dV.handle, 3, again, ok) == _csx.EINVAL and again.value == 0
    assert b"freed" in lib.csx_last_error()
    _csx.free(out)


def test_bad_arguments(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    case = HC.BY_NAME["grid24-shift"]
    nnz, n = len(case.x), case.n
    F = _factor(cs, case)
    V = BC.members(case, 3)
    for values in (V[:-1], np.zeros((nnz, 0)), [], V[:, 0].tolist(), cs.dvec(V[:-1]), np.zeros((nnz + 1, 2))):    # the row count
        with pytest.raises(ValueError):
            F.batch(values)
    batch = F.batch(V)
    with pytest.raises(ValueError):
        batch.refactor(BC.members(case, 2))                       # B is fixed
    with pytest.raises(ValueError):
        batch.refactor(V[:-1])
    for X in (cs.dvec(np.zeros((n, 2))), cs.dvec(np.zeros((n + 1, 3))), cs.dvec(np.zeros((n, 4))), np.zeros((n, 2)), np.zeros(3 * n),
              [0.0] * (3 * n)):
        with pytest.raises(ValueError):
            batch.solve(X)
    for m in (-1, 3):
        with pytest.raises(ValueError):
            batch.member(m)
    for name in ("ash219", "lp_afiro"):                            # a rectangular A: the single solver's errors
        c = HC.BY_NAME[name]
        wide = _factor(cs, c).batch(BC.members(c, 2))
        with pytest.raises(ValueError, match="trans=True needs a square matrix"):
            wide.solve(np.zeros((c.n, 2)), trans=True)
        with pytest.raises(ValueError, match="square"):
            wide.logabsdet()
        with pytest.raises(ValueError):
            wide.solve(np.zeros((c.n if c.m > c.n else c.m + 1, 2)))   # the rows of the unknowns, not of the equations
    # the C ABI
    dV, small = cs.dvec(V), cs.dvec(V[:-1])
    hB, hF, ok, out = batch._h, batch._hF, (C.c_int * 3)(), _csx.new_handle()
    for args in ((hB, dV.handle, 3, out, ok),                            # not a factor
                 (hF, hF, 3, out, ok),                                   # not a vector
                 (hF, small.handle, 3, out, ok),                         # too short for nnz x B
                 (hF, dV.handle, 0, out, ok), (hF, dV.handle, -1, out, ok),
                 (hF, dV.handle, BC.MAX_MEMBERS + 1, out, ok),
                 (hF, dV.handle, 3, None, ok), (hF, dV.handle, 3, out, None)):
        assert lib.csx_hqr_batch_factor(*args) == _csx.EINVAL, args[2]
        assert args[3] is None or out.value == 0
    assert lib.csx_hqr_batch_refactor(hF, dV.handle, ok) == _csx.EINVAL
    assert lib.csx_hqr_batch_refactor(hB, small.handle, ok) == _csx.EINVAL
    assert lib.csx_hqr_batch_refactor(hB, dV.handle, None) == _csx.EINVAL
    dX, dY = cs.dvec(np.zeros((n, 3))), cs.dvec(np.zeros((n, 3)))
    assert lib.csx_hqr_batch_solve(hF, dX.handle, dY.handle, 1, 0) == _csx.EINVAL
    assert lib.csx_hqr_batch_solve(hB, dX.handle, dY.handle, 0, 0) == _csx.EINVAL
    assert lib.csx_hqr_batch_solve(hB, dX.handle, dY.handle, 2, 0) == _csx.EINVAL      # n x 3 doubles are not n x 6
    assert lib.csx_hqr_batch_solve(hB, dX.handle, dX.handle, 1, 0) == _csx.EINVAL      # in place
    assert lib.csx_hqr_batch_solve(hB, hF, dY.handle, 1, 1) == _csx.EINVAL
    shared, per, st = (C.c_int64 * 12)(), (C.c_int64 * 9)(), np.zeros(6)
    assert lib.csx_hqr_batch_info(hF, shared, per) == _csx.EINVAL and lib.csx_hqr_batch_info(hB, None, per) == _csx.EINVAL
    assert lib.csx_hqr_batch_info(hB, shared, None) == _csx.EINVAL
    assert lib.csx_hqr_batch_stats(hF, _csx.pd(st)) == _csx.EINVAL and lib.csx_hqr_batch_stats(hB, None) == _csx.EINVAL
    i = batch.info()
    vx, rx, beta = np.zeros(i["vnz"]), np.zeros(i["rnz"]), np.zeros(n)
    for args in ((hB, 3, vx, rx, beta), (hB, -1, vx, rx, beta), (hB, 0, None, rx, beta), (hB, 0, vx, None, beta), (hB, 0, vx, rx, None),
                 (hF, 0, vx, rx, beta)):
        assert lib.csx_hqr_batch_member(args[0], args[1], *(_csx.pd(a) for a in args[2:])) == _csx.EINVAL
    assert lib.csx_hqr_batch_r_diag(hF, _csx.pd(np.zeros(3 * n))) == _csx.EINVAL and lib.csx_hqr_batch_r_diag(hB, None) == _csx.EINVAL
    diag = np.zeros(3 * n)
    assert lib.csx_hqr_batch_r_diag(hB, _csx.pd(diag)) == _csx.OK
    refs = [_host(case, F, V[:, m]) for m in range(3)]
    assert diag.tobytes() == b"".join(r[5][r[3][1:] - 1].tobytes() for r in refs)
    assert batch.logabsdet().tolist() == [math.fsum(np.log(np.abs(r[5][r[3][1:] - 1])).tolist()) for r in refs]
    # none of it changed the batch
    for m in range(3):
        _member_is(batch, m, refs[m])
