"""csx_pattern_outer / outer_on_pattern and assembly_plan(T).pullback on the device: byte-equal to the host rule
csx_pattern_outer_host (which tests/test_outer_cases_cpu.py pins to the Python restatement) on every case of
tests/outer_cases.py in both modes, the same bytes on a second run, NaN and inf only where their rows reach, the symmetric
storages, the argument checks that leave `out` untouched, U the same block as V, the pull-back against its host rule, and the
Python conventions of outer_on_pattern.  NaNs compare by position, not by payload."""
import numpy as np
import pytest

import _csx
import outer_cases as OC
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()


def matrix(cs, case, values=None):
    """the case's pattern as a `cs`: pattern only unless it (or the caller) brings values"""
    values = case.values if values is None else values
    A = cs.cs_spalloc(case.m, case.n, max(case.nnz, 1), values is not None, False)
    A.p, A.i = case.p.tolist(), (case.i.tolist() or [0])
    if values is not None:
        A.x = np.asarray(values, np.float64).tolist() or [0.0]
    return A


def host(case, sym, alpha=-1.0, clean=False):
    U, V = case.data(clean)
    return _csx.pattern_outer_host(case.m, case.n, case.p, case.i, U, V, case.nrhs, alpha, sym)


def device(cs, case, sym, alpha=-1.0, clean=False):
    U, V = case.data(clean)
    out = cs.outer_on_pattern(matrix(cs, case), cs.dvec(U) if case.m else cs.dvec(0, case.nrhs),
                              cs.dvec(V) if case.n else cs.dvec(0, case.nrhs), alpha, sym)
    assert isinstance(out, cs.dvec) and out.n * out.k == case.nnz
    return out.numpy().reshape(-1)


@pytest.mark.parametrize("name", OC.NAMES)
def test_device_is_the_host_rule_and_runs_twice_alike(cs, name):
    case = OC.BY_NAME[name]
    for sym in OC.modes(case):
        for alpha in (-1.0, 0.75):
            got = device(cs, case, sym, alpha)
            assert same(got, host(case, sym, alpha)), (name, sym, alpha)
        assert same(device(cs, case, sym), device(cs, case, sym))


@pytest.mark.parametrize("name", [c.name for c in OC.CASES if c.special is not None])
def test_nan_and_inf_stay_in_the_entries_their_rows_reach(cs, name):
    case = OC.BY_NAME[name]
    for sym in OC.modes(case):
        got, clean, hit = device(cs, case, sym), device(cs, case, sym, clean=True), case.touched(sym)
        assert hit.any() and not np.isfinite(got[hit]).any() and np.isfinite(clean).all()
        assert got[~hit].tobytes() == clean[~hit].tobytes()


def test_symmetric_storages_give_the_same_bytes_above_and_zero_below(cs):
    cases = [OC.BY_NAME[name] for name in OC.SYM_SHARED]
    U, V = cases[0].data()
    slots = [OC.upper_slots(c) for c in cases]
    got = []
    for c in cases:
        g = cs.outer_on_pattern(matrix(cs, c), U, V, -1.0, True).numpy().reshape(-1)
        col = np.repeat(np.arange(c.n), c.column_lengths())
        low = c.i > col
        assert g[low].tobytes() == np.zeros(int(low.sum())).tobytes()
        got.append(g)
    keys = sorted(slots[0])
    ref = np.array([got[0][slots[0][k]] for k in keys])
    assert np.abs(ref).min() > 0
    for g, s in zip(got[1:], slots[1:]):
        assert np.array([g[s[k]] for k in keys]).tobytes() == ref.tobytes()
    # the values of A are never read: other values below the diagonal (or anywhere) change nothing
    c = OC.BY_NAME["sym_full_other_below"]
    again = cs.outer_on_pattern(matrix(cs, c, values=-3.0 * c.values), U, V, -1.0, True).numpy().reshape(-1)
    assert again.tobytes() == got[2].tobytes()
    low_only = OC.BY_NAME["sym_strictly_lower"]
    g = device(cs, low_only, True)
    assert g.tobytes() == np.zeros(low_only.nnz).tobytes()


def test_every_refusal_leaves_out_untouched(cs):
    lib = _csx.lib()
    case = OC.BY_NAME["5x300"]
    k = case.nrhs
    U, V = case.data()
    with cs._Resident(matrix(cs, case)) as dA:
        dU, dV, out = cs.dvec(U), cs.dvec(V), cs.dvec(case.nnz)
        out.fill(7.0)
        short_u, short_v, short_out = cs.dvec(case.m * k - 1), cs.dvec(case.n * k - 1), cs.dvec(case.nnz - 1)
        short_out.fill(7.0)

        def call(A=dA.handle, U=dU.handle, V=dV.handle, nrhs=k, mode=0, out=out.handle):
            return lib.csx_pattern_outer(A, U, V, nrhs, mode, -1.0, out)

        bad = [dict(A=0), dict(A=dU.handle), dict(U=0), dict(V=dA.handle), dict(out=0), dict(nrhs=0), dict(nrhs=-3),
               dict(mode=2), dict(mode=-1), dict(mode=1), dict(U=short_u.handle), dict(V=short_v.handle),
               dict(out=short_out.handle)]
        for kw in bad:
            assert call(**kw) == _csx.EINVAL, kw
        assert (out.numpy() == 7.0).all() and (short_out.numpy() == 7.0).all()
        # out overlapping U or V: views of one buffer through csx_vec_wrap
        big = cs.dvec(max(case.m, case.n) * k + case.nnz)
        big.fill(7.0)
        base = big.device_ptr()
        views = []
        for off, ln in ((0, case.m * k), (0, case.n * k), (8 * (case.m * k - 1), case.nnz), (8 * (case.n * k - 1), case.nnz)):
            h = _csx.new_handle()
            _csx.check(lib.csx_vec_wrap(_csx.C.c_void_p(base + off), ln, h), "csx_vec_wrap")
            views.append(h)
        try:
            assert call(U=views[0], out=views[2]) == _csx.EINVAL
            assert call(V=views[1], out=views[3]) == _csx.EINVAL
            assert call(U=views[0], out=views[0]) == _csx.EINVAL
            assert (big.numpy() == 7.0).all()
        finally:
            for h in views:
                _csx.free(h)
        assert call() == _csx.OK
        assert same(out.numpy(), host(case, False))


def test_u_may_be_v(cs):
    case = OC.BY_NAME["nrhs%d" % (OC.W + 1)]
    U, _ = case.data()
    dU = cs.dvec(U)
    for sym in (False, True):
        ref = _csx.pattern_outer_host(case.m, case.n, case.p, case.i, U, U, case.nrhs, 0.75, sym)
        assert same(cs.outer_on_pattern(matrix(cs, case), dU, dU, 0.75, sym).numpy(), ref)
        assert same(cs.outer_on_pattern(matrix(cs, case), U, U, 0.75, sym).numpy(), ref)


@pytest.mark.parametrize("plan", OC.PLANS, ids=[p.name for p in OC.PLANS])
def test_pullback_is_its_host_rule(cs, plan):
    T = cs.cs_spalloc(plan.m, plan.n, max(plan.nz, 1), True, True)
    for i, j in zip(plan.Ti.tolist(), plan.Tj.tolist()):
        assert cs.cs_entry(T, i, j, 1.0)
    T.m, T.n = plan.m, plan.n
    P = cs.assembly_plan(T)
    assert (P.nz, P.nnz) == (plan.nz, plan.nnz)
    ref = _csx.assemble_pullback_host(plan.sp, plan.src, plan.g)
    for g in (plan.g, plan.g.tolist(), cs.dvec(plan.g) if plan.nnz else cs.dvec(0)):
        got = P.pullback(g)
        assert isinstance(got, cs.dvec) and got.n * got.k == plan.nz
        assert got.numpy().reshape(-1).tobytes() == ref.tobytes()
    for wrong in (np.zeros(plan.nnz + 1), np.zeros(plan.nnz + 2).tolist()):
        with pytest.raises(ValueError):
            P.pullback(wrong)
    if plan.nnz:
        with pytest.raises(ValueError):
            P.pullback(plan.g[:-1])
        # the pull-back is the transpose of the fold: <assemble(v), g> = <v, pullback(g)> on integers, exactly
        v = np.arange(1.0, plan.nz + 1)
        g = np.arange(1.0, plan.nnz + 1)
        assert float(P.assemble(v).numpy() @ g) == float(v @ P.pullback(g).numpy())
        # refusals of the library call leave out untouched
        lib = _csx.lib()
        dg, out = cs.dvec(plan.g), cs.dvec(plan.nz)
        out.fill(7.0)
        short_g, short_out = cs.dvec(max(plan.nnz - 1, 0)), cs.dvec(plan.nz - 1)
        for args in ((0, dg.handle, out.handle), (dg.handle, dg.handle, out.handle), (P._handle, short_g.handle, out.handle),
                     (P._handle, dg.handle, short_out.handle), (P._handle, dg.handle, 0), (P._handle, out.handle, out.handle)):
            assert lib.csx_assemble_pullback(*args) == _csx.EINVAL
        assert (out.numpy() == 7.0).all()


def test_python_conventions(cs):
    case = OC.BY_NAME["5x300"]
    A = matrix(cs, case)
    U, V = case.data()
    T = cs.cs_spalloc(5, 300, 4, True, True)
    assert cs.outer_on_pattern(T, U, V) is False and cs.outer_on_pattern(None, U, V) is False
    assert cs.outer_on_pattern(A, None, V) is False and cs.outer_on_pattern(A, U, None) is False
    assert cs.outer_on_pattern(A, U, V[:, :-1]) is False
    assert cs.outer_on_pattern(A, U, V, sym=True) is False                        # not square
    with pytest.raises(IndexError):
        cs.outer_on_pattern(A, U[:-1], V)
    with pytest.raises(IndexError):
        cs.outer_on_pattern(A, cs.dvec(U), cs.dvec(V[:-1]))
    ref = host(case, False, 1.0)
    assert A.x is None                                                           # a pattern-only A is accepted
    assert same(cs.outer_on_pattern(A, U, V).numpy(), ref)                       # alpha defaults to 1
    assert same(cs.outer_on_pattern(A, cs.dvec(U), V).numpy(), ref)
    assert same(cs.outer_on_pattern(matrix(cs, case, values=np.ones(case.nnz)), U, V).numpy(), ref)
    taller = np.vstack([U, np.ones((2, case.nrhs))])
    assert same(cs.outer_on_pattern(A, taller, V).numpy(), ref)                  # more rows than needed are fine
    # 1-D vectors are one column
    one = OC.BY_NAME["nrhs1"]
    u, v = one.data()
    ref = host(one, False, 1.0)
    assert same(cs.outer_on_pattern(matrix(cs, one), u[:, 0], v[:, 0].tolist()).numpy(), ref)
    # the result is what refactor(values) and friends take: a dvec of nnz doubles in A's storage order
    out = cs.outer_on_pattern(matrix(cs, one), u, v)
    assert isinstance(out, cs.dvec) and (out.n, out.k) == (one.nnz, 1)
