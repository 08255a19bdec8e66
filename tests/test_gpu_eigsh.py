"""eigsh() and the csx_bgs_* kernels on the device.  The kernels are held byte for byte to csx_bgs_host (which
tests/test_eig_cpu.py holds to the restatement) on every case of tests/eig_cases.py; eigsh() on cholsol_factor(exact=True) and
ldlsol_factor(exact=True) byte for byte to the restated loop of tests/eig_oracle.py run on the device's own solve and residual
calls, and to the conditions the CPU file puts on the pencils.  NaNs compare by position, not by payload."""
import numpy as np
import pytest

import eig_cases as EC
import eig_oracle as EO
from test_eig_cpu import holds, host_rule, same
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = EC.TOL


# ---- the three kernels -----------------------------------------------------------------------------------------------------------------

def device_rule(cs, case, data=None):
    """the three operations on the device, laid out as test_eig_cpu.host_rule's result"""
    import _csx
    lib = _csx.lib()
    V, W, H = case.data() if data is None else data
    nv, rows, b = V.shape
    q = W.shape[1]
    work = cs.dvec(_csx.bgs_work_len(rows, b, q, nv))
    dV = cs.dvec(V.reshape(-1))
    out = {}
    for key, neg in (("gram", 0), ("gram-", 1)):
        dW, got = cs.dvec(W), np.full((nv, b, q), np.nan)
        _csx.check(lib.csx_bgs_gram(dV.handle, nv, b, dW.handle, q, work.handle, rows, neg, _csx.pd(got)))
        assert same(dW.numpy().reshape(rows, q), W)                                  # W is read only
        out[key] = got
    dW = cs.dvec(W)
    _csx.check(lib.csx_bgs_update(dV.handle, nv, b, dW.handle, q, work.handle, rows, _csx.pd(_csx.f64(H))))
    out["update"] = dW.numpy().reshape(rows, q)
    dU = cs.dvec(np.full((rows, q), np.nan))
    _csx.check(lib.csx_bgs_combine(dV.handle, nv, b, dU.handle, q, work.handle, rows, _csx.pd(_csx.f64(H))))
    out["combine"] = dU.numpy().reshape(rows, q)
    assert same(dV.numpy().reshape(V.shape), V)                                      # the basis: untouched
    return out


@pytest.mark.parametrize("name", EC.KERNEL_NAMES)
def test_kernels_are_the_host_rule(cs, name):
    case = EC.KERNEL_BY_NAME[name]
    ref, got = host_rule(case), device_rule(cs, case)
    for key in ref:
        assert same(got[key], ref[key]), key
    again = device_rule(cs, case)                                                    # a second run
    for key in ref:
        assert same(again[key], got[key]), key


def test_a_column_has_the_same_bytes_in_every_block(cs):
    rows, b, nv = EC.CHUNK * EC.FAN + 1, 8, EC.GROUP + 1
    V, w, h = EC.KernelCase("column", rows, b, 1, nv, seed=77).data()
    alone = device_rule(cs, None, (V, w, h))
    for q, at in ((3, 1), (8, 7), (9, 0), (EC.MAXW, EC.MAXW - 1), (EC.MAXW, 13)):
        _, W, H = EC.KernelCase("block", rows, b, q, nv, seed=78 + q).data()
        W[:, at], H[:, :, at] = w[:, 0], h[:, :, 0]
        got = device_rule(cs, None, (V, W, H))
        for key in alone:
            assert same(got[key][..., at], alone[key][..., 0]), (q, at, key)


def test_nv_0_and_rows_0(cs):
    import _csx
    lib = _csx.lib()
    rows, b, q = 300, 3, 2
    V, W, U = cs.dvec(rows * b), cs.dvec(np.arange(rows * q, dtype=np.float64)), cs.dvec(np.full((rows, q), np.nan))
    work, none = cs.dvec(_csx.bgs_work_len(rows, b, q, 1)), np.zeros(1)
    assert lib.csx_bgs_combine(V.handle, 0, b, U.handle, q, work.handle, rows, _csx.pd(none)) == _csx.OK
    assert U.numpy().tobytes() == np.zeros(rows * q).tobytes()                       # +0.0
    assert lib.csx_bgs_update(V.handle, 0, b, W.handle, q, work.handle, rows, _csx.pd(none)) == _csx.OK
    assert W.numpy().tobytes() == np.arange(rows * q, dtype=np.float64).tobytes()
    sums = np.full(b * q, np.nan)
    assert lib.csx_bgs_gram(V.handle, 1, b, W.handle, q, work.handle, 0, 0, _csx.pd(sums)) == _csx.OK and not sums.any()


def test_every_bad_argument_is_refused(cs):
    import _csx
    lib = _csx.lib()
    rows, b, q, nv = 300, 3, 2, 2
    V, W, U, small = cs.dvec(rows * b * nv), cs.dvec(rows, q), cs.dvec(rows, q), cs.dvec(rows * q - 1)
    need = _csx.bgs_work_len(rows, b, q, nv)
    work, short = cs.dvec(need), cs.dvec(need - 1)
    h = np.zeros(nv * b * q)
    ph, E, wide = _csx.pd(h), _csx.EINVAL, EC.MAXW + 1

    def gram(V=V, nv=nv, b=b, W=W, q=q, work=work, rows=rows, ph=ph):
        return lib.csx_bgs_gram(V.handle, nv, b, W.handle, q, work.handle, rows, 0, ph)

    def update(V=V, nv=nv, b=b, W=W, q=q, work=work, rows=rows, ph=ph):
        return lib.csx_bgs_update(V.handle, nv, b, W.handle, q, work.handle, rows, ph)

    def combine(V=V, nv=nv, b=b, W=U, q=q, work=work, rows=rows, ph=ph):
        return lib.csx_bgs_combine(V.handle, nv, b, W.handle, q, work.handle, rows, ph)

    for call in (gram, update, combine):
        assert call() == _csx.OK
        assert call(b=0) == E and call(q=0) == E and call(b=wide) == E and call(q=wide) == E            # every bad width
        assert call(rows=-1) == E and call(nv=-1) == E                                                  # negative counts
        assert call(nv=nv + 1) == E and call(W=small) == E and call(work=short) == E                    # short vectors
        assert call(ph=None) == E                                                                       # a null host array
        assert call(work=V) == E                                                                        # the work vector in the basis
    assert gram(work=W) == E and update(work=W) == E and combine(work=U) == E                            # ... in the block
    assert update(W=V) == E and combine(W=V) == E                                   # a written block inside the basis
    assert gram(W=V, b=q, nv=1) == _csx.OK                                           # ... a read one may be: the Gram matrix of a block
    A = cs.cs_spalloc(2, 2, 2, True, False)
    A.p, A.i, A.x = [0, 1, 2], [0, 1], [1.0, 2.0]
    with cs._Resident(A) as dA:                                                      # a handle that is no vector
        assert lib.csx_bgs_gram(dA.handle, nv, b, W.handle, q, work.handle, rows, 0, ph) == E


def test_views_of_one_buffer_that_share_a_double_are_refused(cs):
    """basis, block and work vector as csx_vec_wrap views of one buffer: a work vector that reaches one double into the
    block or the basis, and a written block that reaches one into the basis, are CSX_EINVAL and nothing is written; the
    same views laid end to end pass"""
    import _csx
    lib = _csx.lib()
    rows, b, q, nv = 8, 3, 2, 2
    vlen, xlen, need = nv * rows * b, rows * q, _csx.bgs_work_len(rows, b, q, nv)
    big = cs.dvec(np.full(vlen + xlen + need, 7.0))
    views = []

    def view(offset, count):
        views.append(_csx.new_handle())
        _csx.check(lib.csx_vec_wrap(_csx.C.c_void_p(big.device_ptr() + 8 * offset), count, views[-1]), "csx_vec_wrap")
        return views[-1]

    V, W, work = view(0, vlen), view(vlen, xlen), view(vlen + xlen, need)
    W_in_V, work_in_W, work_in_V = view(vlen - 1, xlen), view(vlen + xlen - 1, need), view(vlen - 1, need)
    ph = _csx.pd(np.zeros(nv * b * q))
    gram, update, combine = (lambda V, W, work: lib.csx_bgs_gram(V, nv, b, W, q, work, rows, 0, ph),
                             lambda V, W, work: lib.csx_bgs_update(V, nv, b, W, q, work, rows, ph),
                             lambda V, W, work: lib.csx_bgs_combine(V, nv, b, W, q, work, rows, ph))
    try:
        for call in (gram, update, combine):
            assert call(V, W, work_in_W) == _csx.EINVAL
            assert call(V, W, work_in_V) == _csx.EINVAL
        assert update(V, W_in_V, work) == _csx.EINVAL and combine(V, W_in_V, work) == _csx.EINVAL
        assert (big.numpy() == 7.0).all()
        for call in (gram, update, combine):
            assert call(V, W, work) == _csx.OK
    finally:
        for h in views:
            _csx.free(h)


# ---- eigsh -------------------------------------------------------------------------------------------------------------------------------

_DEVICE = {}


def device(cs, p, kind):
    """(F, A, M) of the pencil on the device, built once: A = K - sigma M and M as pinned upper triangles"""
    if (p.name, kind) not in _DEVICE:
        if p.name not in _DEVICE:
            M = p.M()
            _DEVICE[p.name] = (cs.cs_pin(EC.upper_csc(cs, p.A())), None if M is None else cs.cs_pin(EC.upper_csc(cs, M)))
        A, M = _DEVICE[p.name]
        F = cs.cholsol_factor(A, 1, exact=True) if kind == "chol" else cs.ldlsol_factor(A, 1, exact=True)
        assert F is not None
        _DEVICE[(p.name, kind)] = (F, A, M)
    return _DEVICE[(p.name, kind)]


def device_callables(cs, F, A, M):
    """solve, product and residual of the restated loop by the solver's own block solve and residual_block, numpy in and out"""
    def solve(B):
        d = cs.dvec(np.ascontiguousarray(B, dtype=np.float64))
        assert F.solve(d) is True
        return d.numpy().reshape(B.shape)

    def residual(X, B, S=A):
        R, w, _ = cs.residual_block(S, np.ascontiguousarray(X), np.ascontiguousarray(B), sym=True)
        return R.numpy().reshape(np.shape(B)), w

    def product(X):
        return residual(X, np.zeros(np.shape(X)), M)[0]

    return solve, (product if M is not None else None), residual


def as_arrays(out):
    return dict(out, vectors=out["vectors"].numpy().reshape(out["vectors"].n, -1))


SOLVERS = [(name, "ldl") for name in EC.PENCIL_NAMES] + [("grid17x13-mass-0", "chol")]


@pytest.mark.parametrize("name,kind", SOLVERS)
def test_eigsh_is_the_restated_loop_and_finds_the_pairs(cs, name, kind):
    p = EC.PENCIL_BY_NAME[name]
    F, A, M = device(cs, p, kind)
    out = F.eigsh(p.nev, M=M, sigma=p.sigma, block=p.block, tol=TOL)
    got = as_arrays(out)
    assert isinstance(out["vectors"], cs.dvec) and (out["vectors"].n, out["vectors"].k) == (p.n, p.nev)
    ref = EO.eig_loop(*device_callables(cs, F, A, M), p.n, p.nev, sigma=p.sigma, block=p.block, tol=TOL)
    for key in ("values", "vectors", "resid", "omega", "estimate"):
        assert same(got[key], ref[key]), key
    for key in ("blocks", "solves", "products", "breakdown"):
        assert got[key] == ref[key], key
    assert (got["converged"] == ref["converged"]).all()
    holds(p, got)
    if kind == "ldl":
        assert out["below"] == F.inertia()[1] == p.below()
    else:
        assert "below" not in out
    again = as_arrays(F.eigsh(p.nev, M=M, sigma=p.sigma, block=p.block, tol=TOL))    # a second run
    assert same(again["vectors"], got["vectors"]) and same(again["values"], got["values"])


def test_defaults_a_starting_block_and_more_pairs_than_a_chunk(cs):
    p = EC.PENCIL_BY_NAME["grid17x13-mass-3.7"]
    F, A, M = device(cs, p, "ldl")
    out = as_arrays(F.eigsh(3, M=M, sigma=p.sigma))                                   # block = 8
    ref = EO.eig_loop(*device_callables(cs, F, A, M), p.n, 3, sigma=p.sigma)
    assert same(out["vectors"], ref["vectors"]) and same(out["values"], ref["values"]) and out["converged"].all()
    v0 = np.random.default_rng(3).standard_normal((p.n, 4))
    out = as_arrays(F.eigsh(2, M=M, sigma=p.sigma, block=4, v0=v0, A=A))
    ref = EO.eig_loop(*device_callables(cs, F, A, M), p.n, 2, sigma=p.sigma, block=4, v0=v0)
    assert same(out["vectors"], ref["vectors"]) and out["converged"].all() and F.operator_info()["source"] == "given"
    nev = EC.MAXW + 3                                                                 # two column chunks of the Ritz vectors
    out = as_arrays(F.eigsh(nev, M=M, sigma=p.sigma, block=16, maxblocks=12))
    ref = EO.eig_loop(*device_callables(cs, F, A, M), p.n, nev, sigma=p.sigma, block=16, maxblocks=12)
    assert out["vectors"].shape == (p.n, nev) and same(out["vectors"], ref["vectors"]) and same(out["resid"], ref["resid"])
    assert out["blocks"] == ref["blocks"]


def test_breakdown_and_running_out_of_blocks(cs):
    Ad, v0 = EC.breakdown_pencil()
    A = cs.cs_pin(EC.upper_csc(cs, Ad))
    F = cs.cholsol_factor(A, 0, exact=True)
    out = as_arrays(F.eigsh(4, block=8, v0=v0))
    ref = np.sort(np.linalg.eigvalsh(Ad[:8, :8]))[:4]
    assert out["breakdown"] and out["blocks"] == 1 and out["converged"].all() and (out["estimate"] == 0.0).all()
    assert np.abs(out["values"] - ref).max() <= 1e-13 * ref.max() and not out["vectors"][8:].any()
    p = EC.PENCIL_BY_NAME["grid17x13-mass-3.7"]
    F, A, M = device(cs, p, "ldl")
    out = F.eigsh(p.nev, M=M, sigma=p.sigma, block=8, maxblocks=4)                    # three blocks in the Ritz space: too few
    assert not out["converged"].all() and not out["breakdown"] and out["blocks"] == 3 and out["solves"] == 3


def test_bad_arguments(cs):
    p = EC.PENCIL_BY_NAME["grid17x13-mass-0"]
    F, A, M = device(cs, p, "chol")
    n = p.n
    other = cs.cs_spalloc(n + 1, n + 1, 1, True, False)
    for bad in ({"nev": 0}, {"nev": -2}, {"nev": 9, "block": 8, "maxblocks": 2}, {"nev": 1, "maxblocks": 1}, {"block": 0},
                {"block": EC.MAXW + 1}, {"tol": 0.0}, {"tol": 1.0}, {"tol": float("nan")}, {"tol": -0.5}, {"M": other},
                {"v0": np.zeros((n, 7))}, {"v0": np.zeros((n - 1, 8))}, {"v0": np.ones((n, 8))}, {"A": other}):
        kw = dict({"nev": 4, "M": M, "block": 8}, **bad)
        with pytest.raises(ValueError):
            F.eigsh(kw.pop("nev"), **kw)
    pattern = cs.cs_spalloc(n, n, 1, False, False)
    with pytest.raises(TypeError):
        F.eigsh(4, M=pattern)
    with pytest.raises(MemoryError, match="bytes"):
        cs._EigSpace(10 ** 9, EC.MAXW, 2 ** 20, EC.MAXW, True)                         # 5e17 bytes of bases
    Cm = cs.cs_spalloc(n, 1, 1, True, False)
    Cm.p, Cm.i, Cm.x = [0, 1], [n - 1], [0.5]
    G = cs.cholsol_factor(A, 1, exact=True)
    assert G.update(Cm) is True
    with pytest.raises(RuntimeError, match="A="):
        G.eigsh(4, M=M)
