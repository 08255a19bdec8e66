"""gmres() and the csx_gs_* kernels on the device.  The kernels are held byte for byte to csx_gs_host (which
tests/test_gmres_cpu.py holds to the restatement) on every case of tests/gmres_cases.py; gmres() to the conditions the CPU file
establishes on the systems of gmres_cases -- omega <= 2^-52 in every column within the inner-step bound, where refine() ends above
it -- and, with an exact solver, byte for byte to the restated loop of tests/gmres_oracle.py run on the device's own solve and
residual.  NaNs compare by position, not by payload."""
import numpy as np
import pytest

import gmres_cases as GC
import gmres_oracle as GO
import hqr_cases as HC
from test_gmres_cpu import counted, host_rule, same
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = GC.EPS


# ---- the four kernels ------------------------------------------------------------------------------------------------------------------

def device_rule(cs, case, data=None, mask=None):
    """the four operations on the device, laid out as test_gmres_cpu.host_rule's result"""
    import _csx
    lib = _csx.lib()
    V, W, h, s, y, length = case.data() if data is None else data
    m = _csx.i32(case.mask() if mask is None else mask)
    nv, (rows, k) = V.shape[0] - 1, W.shape
    work = cs.dvec(_csx.gs_work_len(rows, k, nv + 1))
    dV = cs.dvec(V.reshape(-1))
    out = {}
    for key, neg in (("h", 0), ("h-", 1)):
        dW, got = cs.dvec(W), np.full((nv, k), np.nan)
        _csx.check(lib.csx_gs_project(dV.handle, nv, dW.handle, work.handle, rows, k, _csx.pi(m), neg, _csx.pd(got)))
        assert dW.numpy().reshape(rows, k).tobytes() == W.tobytes()
        out[key] = got
    for key, neg in (("update", 0), ("update-", 1)):
        dW, nrm2 = cs.dvec(W), np.full(k, np.nan)
        _csx.check(lib.csx_gs_update(dV.handle, nv, dW.handle, work.handle, rows, k, _csx.pi(m), neg, _csx.pd(_csx.f64(h)),
                                     _csx.pd(nrm2)))
        out[key] = (dW.numpy().reshape(rows, k), nrm2)
    dW = cs.dvec(W)
    _csx.check(lib.csx_gs_scale(dW.handle, dV.handle, nv, work.handle, rows, k, _csx.pi(m), _csx.pd(_csx.f64(s))))
    after = dV.numpy().reshape(nv + 1, rows, k)
    assert same(after[:nv], V[:nv])                                                   # the other blocks of the basis: untouched
    out["scale"] = after[nv]
    dU = cs.dvec(np.full((rows, k), np.nan))
    _csx.check(lib.csx_gs_combine(dV.handle, nv, dU.handle, work.handle, rows, k, _csx.pi(m), _csx.pd(_csx.f64(y)),
                                  _csx.pi(_csx.i32(length))))
    out["combine"] = dU.numpy().reshape(rows, k)
    return out


def agree(got, ref):
    for key in ref:
        if isinstance(ref[key], tuple):
            assert same(got[key][0], ref[key][0]) and same(got[key][1], ref[key][1]), key
        else:
            assert same(got[key], ref[key]), key


@pytest.mark.parametrize("name", GC.KERNEL_NAMES)
def test_kernels_are_the_host_rule(cs, name):
    case = GC.KERNEL_BY_NAME[name]
    ref, got = host_rule(case), device_rule(cs, case)
    agree(got, ref)                                       # (masked columns: the NaN or the input both sides started from)
    agree(device_rule(cs, case), got)                     # a second run


def test_a_column_has_the_same_bytes_in_every_block(cs):
    rows, nv = GC.CHUNK * GC.FAN + 1, GC.GROUP + 1
    one = GC.KernelCase("column", rows, 1, nv, seed=77).data()
    alone = device_rule(cs, None, one, np.ones(1, np.int32))
    for k, at in ((3, 1), (64, 63), (64, 0), (65, 64), (130, 77)):
        V, W, h, s, y, length = GC.KernelCase("block", rows, k, nv, seed=78 + k).data()
        for big, small in zip((V, W, h, s, y, length), one):
            big[..., at] = small[..., 0]
        got = device_rule(cs, None, (V, W, h, s, y, length), np.ones(k, np.int32))
        for key in alone:
            if isinstance(alone[key], tuple):
                assert same(got[key][0][:, at], alone[key][0][:, 0]) and same(got[key][1][at], alone[key][1][0]), (k, key)
            else:
                assert same(got[key][..., at], alone[key][..., 0]), (k, key)


def test_every_bad_argument_is_refused(cs):
    import _csx
    lib = _csx.lib()
    rows, k, nv = 300, 3, 2
    V, W, U, small = cs.dvec(rows * k * nv), cs.dvec(rows, k), cs.dvec(rows, k), cs.dvec(rows * k - 1)
    work, short = cs.dvec(_csx.gs_work_len(rows, k, nv)), cs.dvec(_csx.gs_work_len(rows, k, nv) - 1)
    m, h, ln = _csx.i32([1, 1, 1]), np.zeros(nv * k), _csx.i32([2, 1, 0])
    pm, ph, pl = _csx.pi(m), _csx.pd(h), _csx.pi(ln)
    E = _csx.EINVAL

    def project(V=V, nv=nv, W=W, work=work, rows=rows, k=k, pm=pm, ph=ph):
        return lib.csx_gs_project(V.handle, nv, W.handle, work.handle, rows, k, pm, 0, ph)

    def update(V=V, nv=nv, W=W, work=work, rows=rows, k=k, pm=pm, ph=ph, pn=ph):
        return lib.csx_gs_update(V.handle, nv, W.handle, work.handle, rows, k, pm, 0, ph, pn)

    def scale(W=W, V=V, slot=1, work=work, rows=rows, k=k, pm=pm, ps=ph):
        return lib.csx_gs_scale(W.handle, V.handle, slot, work.handle, rows, k, pm, ps)

    def combine(V=V, nv=nv, U=U, work=work, rows=rows, k=k, pm=pm, py=ph, pl=pl):
        return lib.csx_gs_combine(V.handle, nv, U.handle, work.handle, rows, k, pm, py, pl)

    for call in (project, update, scale, combine):
        assert call() == _csx.OK
        assert call(k=0) == E and call(rows=-1) == E and call(pm=None) == E and call(work=short) == E
    assert project(work=W) == E and update(work=W) == E and scale(work=W) == E and combine(work=U) == E   # the block itself
    assert project(work=V) == E and combine(work=V) == E                                                 # ... the basis
    for call in (project, update, combine):
        assert call(nv=0) == E and call(nv=nv + 1) == E                           # nv < 1, nv above the basis
    assert project(W=small) == E and update(W=small) == E and scale(W=small) == E and combine(U=small) == E
    assert project(W=V) == E and combine(U=V) == E and scale(W=V) == E            # the block inside the basis
    assert project(ph=None) == E and update(ph=None) == E and update(pn=None) == E and scale(ps=None) == E
    assert combine(py=None) == E and combine(pl=None) == E
    assert scale(slot=-1) == E and scale(slot=nv) == E
    assert combine(pl=_csx.pi(_csx.i32([3, 0, 0]))) == E and combine(pl=_csx.pi(_csx.i32([-1, 0, 0]))) == E
    dead = _csx.i32([0, 1, 1])
    assert combine(pm=_csx.pi(dead), pl=_csx.pi(_csx.i32([9, 0, 0]))) == _csx.OK   # a masked column's length is not read
    A = cs.cs_spalloc(2, 2, 2, True, False)
    A.p, A.i, A.x = [0, 1, 2], [0, 1], [1.0, 2.0]
    with cs._Resident(A) as dA:                                                    # a handle that is no vector
        assert lib.csx_gs_project(dA.handle, nv, W.handle, work.handle, rows, k, pm, 0, ph) == E
    empty = np.full(nv * k, np.nan)
    assert project(rows=0, ph=_csx.pd(empty)) == _csx.OK and not empty.any()


def test_views_of_one_buffer_that_share_a_double_are_refused(cs):
    """basis, block and work vector as csx_vec_wrap views of one buffer: a view that reaches one double into another is
    CSX_EINVAL at every entry point and nothing is written; the same views laid end to end pass"""
    import _csx
    lib = _csx.lib()
    rows, k, nv = 8, 4, 2
    block, need = rows * k, _csx.gs_work_len(rows, k, nv)
    big = cs.dvec(np.full((nv + 1) * block + need, 7.0))
    views = []

    def view(offset, count):
        views.append(_csx.new_handle())
        _csx.check(lib.csx_vec_wrap(_csx.C.c_void_p(big.device_ptr() + 8 * offset), count, views[-1]), "csx_vec_wrap")
        return views[-1]

    V, W, work = view(0, nv * block), view(nv * block, block), view((nv + 1) * block, need)
    W_in_V, work_in_W, work_in_V = view(nv * block - 1, block), view((nv + 1) * block - 1, need), view(nv * block - 1, need)
    pm, ph, pl = _csx.pi(_csx.i32([1] * k)), _csx.pd(np.zeros(nv * k)), _csx.pi(_csx.i32([nv] * k))
    calls = (lambda V, W, work: lib.csx_gs_project(V, nv, W, work, rows, k, pm, 0, ph),
             lambda V, W, work: lib.csx_gs_update(V, nv, W, work, rows, k, pm, 0, ph, ph),
             lambda V, W, work: lib.csx_gs_scale(W, V, nv - 1, work, rows, k, pm, ph),
             lambda V, W, work: lib.csx_gs_combine(V, nv, W, work, rows, k, pm, ph, pl))
    try:
        for call in calls:
            assert call(V, W_in_V, work) == _csx.EINVAL
            assert call(V, W, work_in_W) == _csx.EINVAL
            assert call(V, W, work_in_V) == _csx.EINVAL
        assert (big.numpy() == 7.0).all()
        for call in calls:
            assert call(V, W, work) == _csx.OK
    finally:
        for h in views:
            _csx.free(h)


# ---- the systems ------------------------------------------------------------------------------------------------------------------------

def _exact(s):
    return None if s.name.startswith("stale-btf") else True


@pytest.mark.parametrize("name", GC.NAMES)
def test_gmres_ends_where_refine_stalls(cs, name):
    s = GC.BY_NAME[name]
    F, kw = s.device(cs, _exact(s)) if _exact(s) else s.device(cs)
    assert F is not None
    for k in ((1, 3, 65) if s in GC.CHOL else (3,)):
        B = s.B(k)
        dX = cs.dvec(B)
        out = F.gmres(dX, **kw)
        ref = F.refine(cs.dvec(B), **kw)
        print(name, k, "bound", GC.bound(s), "gmres omega / eps", out["omega"][:3] / EPS, "iters", out["iters"][:3], "cycles",
              out["cycles"][:3], "refine omega / eps", ref["omega"][:3] / EPS, "steps", ref["steps"][:3])
        assert sorted(out) == ["cycles", "iters", "omega", "omega0", "resid_est", "rnorm", "solves", "steps"]
        assert out["steps"] is out["cycles"] and out["omega"].shape == (k,)
        assert (out["omega"] <= EPS).all() and (out["iters"] <= GC.bound(s)).all() and (out["iters"] >= 1).all()
        assert (out["omega"] <= out["omega0"]).all() and out["omega0"].tobytes() == ref["omega0"].tobytes()
        assert F.backward_error(dX, cs.dvec(B), **kw).tobytes() == out["omega"].tobytes()
        if name != "saddle-perturb1e-10":                 # (there refinement mends it: tests/test_gmres_cpu.py says why it stays)
            assert (ref["omega"] > EPS).all()
        if s.refine_accepts_none:
            assert not ref["steps"].any()


def device_callables(cs, F, A, kw, sym=False):
    """solve(B) -> X by the solver's own block solve and residual(X, B) -> (R, omega) by residual_block, numpy in and out"""
    trans = bool(kw.get("trans", False))

    def solve(B):
        d = cs.dvec(np.ascontiguousarray(B, dtype=np.float64))
        r = F.solve(d, trans=trans) if "trans" in kw else F.solve(d)
        assert r is True or r is d
        return d.numpy().reshape(B.shape)

    def residual(X, B):
        R, w, _ = cs.residual_block(A, np.ascontiguousarray(X), np.ascontiguousarray(B), trans=trans, sym=sym)
        return R.numpy().reshape(np.shape(B)), w

    return solve, residual


def held_to_the_oracle(cs, F, A, B, kw, **args):
    solve, residual = device_callables(cs, F, A, kw)
    res, calls = counted(residual, B)
    ref = GO.gmres_loop(solve, res, B, **args)
    dX = cs.dvec(B)
    out = F.gmres(dX, **dict(kw, **args))
    print("omega / eps", out["omega"] / EPS, "iters", out["iters"], "cycles", out["cycles"], "resid_est", out["resid_est"])
    assert dX.numpy().tobytes() == ref["x"].tobytes()
    for key in ("omega0", "omega", "iters", "cycles", "resid_est"):
        assert same(out[key], ref[key]) and out[key].dtype == ref[key].dtype, key
    assert out["solves"] == ref["solves"]
    return out, calls[0] - 1


@pytest.mark.parametrize("perturb", [1e-10, GC.SADDLE_PERTURB])
def test_a_whole_run_is_the_restated_loop(cs, perturb):
    import slu_cases as SC
    s = GC.BY_NAME["saddle-perturb%g" % perturb]
    F, kw = s.device(cs, True)
    out, _ = held_to_the_oracle(cs, F, SC.BY_NAME["saddle"].matrix(cs), s.B(3), kw)
    assert (out["omega"] <= EPS).all()
    held_to_the_oracle(cs, F, SC.BY_NAME["saddle"].matrix(cs), s.B(3), kw, restart=1, maxit=5)
    held_to_the_oracle(cs, F, SC.BY_NAME["saddle"].matrix(cs), s.B(3), kw, restart=3, maxit=7, inner_tol=0.5)


def test_a_refused_cycle_leaves_the_column_as_it_was(cs):
    """tests/test_gmres_cpu.py: on REFUSED the model refuses the third cycle of column REFUSED_COLUMN.  The device's run is the
    restated loop's byte for byte, in which a refused candidate is never copied; that a cycle was refused here too shows in the
    count of candidates judged against the cycles kept."""
    import slu_cases as SC
    s = GC.REFUSED
    F, kw = s.device(cs, True)
    out, judged = held_to_the_oracle(cs, F, SC.BY_NAME["saddle"].matrix(cs), s.B(3), kw)
    c = GC.REFUSED_COLUMN
    assert out["omega"][c] > EPS and out["iters"][c] < GC.MAXIT and out["cycles"][c] < judged
    assert (out["omega"] <= out["omega0"]).all()
    # inner_tol close to 1 on columns already near eps: whatever is refused, nothing rises and the bytes are the oracle's
    B = s.B(3)
    dX = cs.dvec(B)
    F.gmres(dX, **kw)
    near, _ = held_to_the_oracle(cs, F, SC.BY_NAME["saddle"].matrix(cs), B, kw, inner_tol=0.999, maxit=4)
    assert (near["omega"] <= near["omega0"]).all()


def test_guarantees_with_an_exact_solver(cs):
    s = GC.BY_NAME["saddle-perturb%g" % GC.SADDLE_PERTURB]
    F, kw = s.device(cs, True)
    runs = {}
    for k in (1, 3, 64, 65):
        dX = cs.dvec(s.B(k))
        out = F.gmres(dX)
        runs[k] = (dX.numpy().reshape(s.n, k), out)
    dX = cs.dvec(s.B(65))
    again = F.gmres(dX)
    assert dX.numpy().tobytes() == runs[65][0].tobytes() and same(again["omega"], runs[65][1]["omega"])
    for k in (3, 64, 65):
        for c in range(min(k, 3) if k > 1 else 1):
            if c == 0:
                assert runs[k][0][:, 0].tobytes() == runs[1][0][:, 0].tobytes()
            assert runs[k][0][:, c].tobytes() == runs[3][0][:, c].tobytes(), (k, c)
            for key in ("omega0", "omega", "iters", "cycles", "resid_est"):
                assert runs[k][1][key][c] == runs[3][1][key][c], (k, c, key)
    # the scaled copies of a column take its steps (a power of two scales every operation exactly)
    assert (runs[65][1]["iters"] == np.resize(runs[3][1]["iters"], 65)).all()
    # maxit = 0 is solve() and the backward error
    B = s.B(3)
    plain = cs.dvec(B)
    assert F.solve(plain) is True
    dX = cs.dvec(B)
    none = F.gmres(dX, maxit=0)
    assert dX.numpy().tobytes() == plain.numpy().tobytes() and not none["iters"].any() and none["solves"] == 1
    assert none["omega"].tobytes() == F.backward_error(plain, cs.dvec(B)).tobytes() == none["omega0"].tobytes()
    # a NaN column reports NaN and leaves its neighbours as they are without it
    Bn = B.copy()
    Bn[5, 1] = np.nan
    dX = cs.dvec(Bn)
    out = F.gmres(dX)
    X = dX.numpy()
    assert np.isnan(out["omega"][1]) and out["iters"][1] == 0 and out["cycles"][1] == 0
    for c in (0, 2):
        assert X[:, c].tobytes() == runs[3][0][:, c].tobytes() and out["iters"][c] == runs[3][1]["iters"][c]
    # restart = 1
    dX = cs.dvec(B)
    one = F.gmres(dX, restart=1, maxit=6)
    assert (one["iters"] <= 6).all() and (one["omega"] <= one["omega0"]).all()


def test_nothing_to_do_is_the_plain_solve(cs):
    s = GC.DIAGONAL
    F, kw = s.device(cs, True)
    B = s.B(3)
    plain = cs.dvec(B)
    assert F.solve(plain) is True
    dX = cs.dvec(B)
    out = F.gmres(dX)
    assert (out["omega0"] <= EPS).all() and not out["iters"].any() and not out["cycles"].any() and out["solves"] == 1
    assert dX.numpy().tobytes() == plain.numpy().tobytes() and (out["resid_est"] == 1.0).all()


def test_a_restart_shorter_than_the_rank_goes_on_through_restarts(cs):
    s = GC.BY_NAME["chol-order1-r5-sigma50"]
    F, kw = s.device(cs, True)
    out = F.gmres(cs.dvec(s.B(3)), restart=4, **kw)
    print("restart 4: omega / eps", out["omega"] / EPS, "iters", out["iters"], "cycles", out["cycles"])
    assert (out["iters"] <= GC.MAXIT).all() and (out["omega"] <= out["omega0"]).all()
    assert ((out["omega"] <= EPS) | (out["iters"] == GC.MAXIT) | (out["cycles"] >= 1)).all()


# ---- interfaces ----------------------------------------------------------------------------------------------------------------------------

def test_lists_arrays_and_blocks(cs):
    s = GC.BY_NAME["ldl-grid24-shift-perturbed"]
    F, kw = s.device(cs, True)
    B = s.B(3)
    dX = cs.dvec(B)
    blk = F.gmres(dX)
    X = dX.numpy()
    arr = B.copy()
    out = F.gmres(arr)
    assert arr.tobytes() == X.tobytes() and same(out["omega"], blk["omega"])
    b = B[:, 0].tolist()
    one = F.gmres(b)
    assert isinstance(b, list) and len(b) == s.n and one["omega"].shape == (1,) and one["omega"][0] <= EPS
    assert F.backward_error(b, B[:, 0].tolist()) == one["omega"][0]
    vec = B[:, 0].copy()
    assert F.gmres(vec)["omega"][0] <= EPS and vec.tolist() == b
    with pytest.raises(IndexError):
        F.gmres([1.0] * (s.n - 1))


def test_the_operator_of_the_symmetric_solvers(cs):
    s = GC.BY_NAME["chol-order0-r1-sigma50"]
    F, kw = s.device(cs)
    B = s.B(3)
    out = F.gmres(cs.dvec(B))                                         # A=None: the factored matrix itself
    assert (out["omega"] <= 4.0 * EPS).all() and F.operator_info()["source"] == "factored"
    assert (F.gmres(cs.dvec(B), **kw)["omega"] <= EPS).all() and F.operator_info()["source"] == "given"
    n = s.n
    with pytest.raises(ValueError):
        F.gmres(cs.dvec(B), A=cs.cs_spalloc(n + 1, n + 1, 1, True, False))
    Cm = cs.cs_spalloc(n, 1, 1, True, False)
    Cm.p, Cm.i, Cm.x = [0, 1], [n - 1], [0.5]
    assert F.update(Cm) is True
    b = B[:, 0].tolist()
    with pytest.raises(RuntimeError, match="A="):
        F.gmres(b)
    assert b == B[:, 0].tolist()
    out = F.gmres(cs.dvec(B), **kw)                                   # the updated factor still preconditions
    assert (out["omega"] <= out["omega0"]).all() and (out["cycles"] >= 1).all()


def test_square_householder_factors_take_it_and_tall_ones_do_not(cs):
    case = HC.BY_NAME["grid24-shift"]
    F = cs.hqrsol_factor(cs.cs_pin(case.matrix(cs)), case.order)
    B = np.ascontiguousarray(HC.rhs(case, 3).T)
    for trans in (False, True):
        dX = cs.dvec(B)
        out = F.gmres(dX, trans=trans)
        print("hqr", trans, "omega0 / eps", out["omega0"] / EPS, "omega / eps", out["omega"] / EPS, "iters", out["iters"])
        assert (out["omega"] <= out["omega0"]).all() and ((out["omega"] <= EPS) | (out["iters"] >= 1)).all()
        assert F.backward_error(dX, cs.dvec(B), trans=trans).tobytes() == out["omega"].tobytes()
    tall = HC.BY_NAME["ash219"]
    T = cs.hqrsol_factor(cs.cs_pin(tall.matrix(cs)), tall.order)
    with pytest.raises(ValueError, match="square"):
        T.gmres(HC.rhs(tall, 1)[0].tolist())


def test_bad_arguments(cs):
    s = GC.DIAGONAL
    F, kw = s.device(cs)
    b = s.B(1)[:, 0].tolist()
    for bad in ({"restart": 0}, {"restart": -3}, {"maxit": -1}, {"inner_tol": 0.0}, {"inner_tol": 1.0}, {"inner_tol": -0.5},
                {"inner_tol": float("nan")}, {"inner_tol": 2.0}):
        x = list(b)
        with pytest.raises(ValueError, match="gmres"):
            F.gmres(x, **bad)
        assert x == b
    sym, kws = GC.BY_NAME["chol-order0-r1-sigma50"].device(cs)
    with pytest.raises(ValueError, match="gmres"):
        sym.gmres(list(GC.BY_NAME["chol-order0-r1-sigma50"].B(1)[:, 0]), restart=0, **kws)


def test_a_basis_that_cannot_be_had_is_a_memory_error(cs):
    s = GC.BY_NAME["saddle-perturb%g" % GC.SADDLE_PERTURB]
    F, kw = s.device(cs)
    with pytest.raises(MemoryError, match="bytes"):
        F.gmres(cs.dvec(s.B(3)), restart=2 ** 30)                    # 7e12 bytes of basis
