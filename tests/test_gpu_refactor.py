"""refactor() of btf_factor and lusol_factor on the device: new values with the pivots kept give L, U, F
byte-equal to a fresh factor of the new values wherever it pivots the same, solves byte-equal to the CPU restatements on
the new factors, a failed refactor changes nothing, and another pattern is refused."""
import numpy as np
import pytest
import scipy.sparse as sp

import btf_oracle
import synth
import trans_oracle as T
from conftest import golden

pytestmark = pytest.mark.gpu


def cs():
    import csparse
    return csparse


def _fixture(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])
    p = g["C_p"].astype(np.int64)
    S = sp.coo_matrix(sp.csc_matrix((g["C_x"][:p[n]], g["C_i"][:p[n]], p), shape=(m, n))).tocsc()
    S.sum_duplicates()
    return S


def _cs(S):
    S = sp.csc_matrix(S)
    A = cs().cs_spalloc(S.shape[0], S.shape[1], max(S.nnz, 1), True, False)
    A.p, A.i, A.x = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    return A


def _device(S):
    import _csx
    S = sp.csc_matrix(S)
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(S.shape[0], S.shape[1], _csx.pi(_csx.i32(S.indptr)), _csx.pi(_csx.i32(S.indices)),
                                         _csx.pd(_csx.f64(S.data)), h), "upload")
    return cs()._from_device(h, lambda nnz: max(nnz, 1))


def _with(S, x):
    return sp.csc_matrix((x, S.indices.copy(), S.indptr.copy()), shape=S.shape)


def _entrywise(S, seed):
    return _with(S, S.data * (1.0 + 1e-3 * np.random.default_rng(seed).uniform(-1, 1, S.nnz)))


def _columnwise(S, seed):
    u = np.random.default_rng(seed).uniform(-1, 1, S.shape[1])
    return _with(S, S.data * (1.0 + 1e-3 * u)[np.repeat(np.arange(S.shape[1]), np.diff(S.indptr))])


def _arr(M, n):
    nnz = M.p[n]
    return np.asarray(M.p[:n + 1], np.int64), np.asarray(M.i[:nnz], np.int64), np.asarray(M.x[:nnz], np.float64)


def _same_factors(fa, fb, n):
    assert np.array_equal(fa.pinv, fb.pinv), "a fresh factor of the new values pivots differently: pick another case"
    for name in ("L", "U", "F", "D"):
        a, b = _arr(getattr(fa, name), n), _arr(getattr(fb, name), n)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes(), name


def _btf_solves(sol, S, widths, seed):
    """forward and transposed solves byte-equal to the CPU restatements on the solver's factors; blocks equal to lists"""
    c = cs()
    n = S.shape[0]
    f = sol.factors
    rng = np.random.default_rng(seed)
    for trans in (False, True):
        b = rng.uniform(-1, 1, n)
        x = b.tolist()
        assert sol.solve(x, trans=trans) is True
        if trans:
            want = T.btf_solve_trans(f.L, f.U, f.F, f.pinv, f.p, f.q, f.r, list(b))
        else:
            want = btf_oracle.solve(f.L, f.U, f.F, f.pinv, f.p, f.q, f.r, list(b))
        assert np.asarray(x).tobytes() == np.asarray(want).tobytes(), trans
        for k in widths:
            B = rng.uniform(-1, 1, (n, k))
            dB = c.dvec(B)
            sol.solve(dB, trans=trans)
            X = dB.numpy().reshape(n, k)
            for col in (0, k - 1):
                xc = B[:, col].tolist()
                sol.solve(xc, trans=trans)
                assert np.asarray(xc).tobytes() == X[:, col].tobytes(), (trans, k, col)


def _generated(n, seed, depth, big=()):
    S, _, _ = btf_oracle.reducible(btf_oracle.block_sizes(n, seed, big=big), depth, seed)
    return S


BTF_CASES = [  # (matrix, perturbation, tol): the generated matrices at tol 1, the fixtures at tol 0.001
    ("west0067", _columnwise, 0.001),
    ("fs_183_1", _entrywise, 0.001),
    ("gen20k", _entrywise, 1.0),
    ("large300", _entrywise, 1.0),
]


def _btf_matrix(name):
    if name == "gen20k":
        return _generated(20000, 4, 6)
    if name == "large300":
        return _generated(4000, 7, 6, big=(300,))
    return _fixture(name)


@pytest.mark.parametrize("name,perturb,tol", BTF_CASES)
def test_btf_refactor_equals_a_fresh_factor(name, perturb, tol):
    c = cs()
    S = _btf_matrix(name)
    n = S.shape[0]
    S2 = perturb(S, 21)
    sol = c.btf_factor(_cs(S), tol)
    assert sol is not None
    _btf_solves(sol, S, (1,), 1)                  # the transposed programs exist before the refactor
    assert sol.refactor(_cs(S2)) is True
    info = sol.refactor_info()
    assert info["device_columns"] + info["host_columns"] == n and 0.0 < info["pivot_ratio"] <= 1.0
    sizes = np.diff(sol.factors.r)
    assert info["host_columns"] == int(sizes[sizes > 96].sum())      # blocks over 96 rows take the host loop
    if name == "large300":
        assert info["host_columns"] == 300 and sol.info()["large_blocks"] == 1
    fresh = c.btf_factor(_cs(S2), tol)
    _same_factors(sol.factors, fresh.factors, n)
    _btf_solves(sol, S2, (1, 64, 65), 2)
    assert sol.condest() == fresh.condest()


def test_btf_refactor_there_and_back():
    c = cs()
    S = _generated(3000, 9, 5)
    n = S.shape[0]
    sol = c.btf_factor(_cs(S))
    b = np.random.default_rng(4).uniform(-1, 1, (n, 65))
    outs = []
    for M in (S, _entrywise(S, 5), S):
        if outs:
            assert sol.refactor(_cs(M)) is True
        for trans in (False, True):
            dB = c.dvec(b)
            sol.solve(dB, trans=trans)
            outs.append(dB.numpy().tobytes())
    assert outs[0] == outs[4] and outs[1] == outs[5] and outs[0] != outs[2]


def test_btf_refactor_inputs():
    """a device-resident A2, its values as numpy, list and dvec: the same factors"""
    c = cs()
    S = _generated(3000, 10, 4)
    n = S.shape[0]
    S2 = _entrywise(S, 6)
    ref = c.btf_factor(_cs(S))
    assert ref.refactor(_cs(S2)) is True
    for a2 in (_device(S2), S2.data.copy(), S2.data.tolist(), c.dvec(S2.data)):
        sol = c.btf_factor(_device(S))
        assert sol.refactor(a2) is True
        _same_factors(sol.factors, ref.factors, n)
        b = np.linspace(-1, 1, n)
        x, y = b.tolist(), b.tolist()
        sol.solve(x)
        ref.solve(y)
        assert x == y
        assert sol.condest() == ref.condest()


def test_btf_failed_refactor_changes_nothing():
    c = cs()
    S = _generated(3000, 11, 4)
    n = S.shape[0]
    sol = c.btf_factor(_cs(S))
    f = sol.factors
    Lx_read = list(f.L.x)                          # host lists read before: they stay what they were
    one = next(b for b in range(len(f.r) - 1) if f.r[b + 1] - f.r[b] == 1)
    row, col = int(f.p[f.r[one]]), int(f.q[f.r[one]])
    t = S.indptr[col] + int(np.flatnonzero(S.indices[S.indptr[col]:S.indptr[col + 1]] == row)[0])
    x2 = _entrywise(S, 8).data
    x2[t] = 0.0                                    # the 1-by-1 block's only entry: its pivot
    b = np.random.default_rng(2).uniform(-1, 1, (n, 64))
    before = []
    for trans in (False, True):
        dB = c.dvec(b)
        sol.solve(dB, trans=trans)
        before.append(dB.numpy().tobytes())
    assert sol.refactor(x2) is False
    assert sol.refactor_info()["ok"] is False
    assert list(f.L.x) == Lx_read
    after = []
    for trans in (False, True):
        dB = c.dvec(b)
        sol.solve(dB, trans=trans)
        after.append(dB.numpy().tobytes())
    assert before == after


def test_btf_refactor_other_pattern_raises():
    c = cs()
    S = _generated(2000, 12, 3)
    sol = c.btf_factor(_cs(S))
    with pytest.raises(ValueError):
        sol.refactor(S.data[:-1])
    R = S.tolil()
    j = 5
    i = next(r for r in range(S.shape[0]) if R[r, j] == 0)
    R[i, j] = 1.0
    with pytest.raises(ValueError):
        sol.refactor(_cs(R.tocsc()))
    Q = _with(S, S.data)
    Q.indices = Q.indices.copy()
    a, e = Q.indptr[3], Q.indptr[4]
    assert e - a >= 2
    Q.indices[a:e] = Q.indices[a:e][::-1].copy()   # same entries, another storage order
    with pytest.raises(ValueError):
        sol.refactor(_cs(Q))
    assert sol.refactor(_cs(_entrywise(S, 1))) is True


def test_btf_refactor_scale_1m_128_rhs():
    import c_oracle as CO
    c = cs()
    sizes = btf_oracle.block_sizes(1_000_000, 11)
    S, blocks, depth = btf_oracle.reducible(sizes, 8, 11)
    n = S.shape[0]
    sol = c.btf_factor(_device(S))
    S2 = _entrywise(S, 31)
    assert sol.refactor(_device(S2)) is True
    assert sol.refactor_info()["host_columns"] == 0
    k = 128
    B = np.random.default_rng(3).uniform(-1, 1, (n, k))
    dB = c.dvec(B)
    assert sol.solve(dB)
    X = dB.numpy().reshape(n, k)
    f = sol.factors
    F, L, U = f.F, f.L, f.U
    Fp, Fi, Fx = (np.asarray(F.p), np.asarray(F.i[:F.p[n]]), -np.asarray(F.x[:F.p[n]]))
    Lp, Li, Lx = np.asarray(L.p), np.asarray(L.i[:L.p[n]]), np.asarray(L.x[:L.p[n]])
    Up, Ui, Ux = np.asarray(U.p), np.asarray(U.i[:U.p[n]]), np.asarray(U.x[:U.p[n]])
    nA = abs(S2).sum(axis=1).max()
    for col in range(0, k, 9):
        x = X[:, col]
        z = x[f.q]
        rr = CO.gaxpy(n, n, Fp, Fi, Fx, z, B[f.p, col])
        w = CO.usolve(n, Up, Ui, Ux, CO.lsolve(n, Lp, Li, Lx, CO.ipvec(f.pinv, rr)))
        assert w.tobytes() == z.tobytes(), col
        res = np.max(np.abs(S2 @ x - B[:, col]))
        assert res / (nA * np.max(np.abs(x)) + np.max(np.abs(B[:, col]))) < 1e-13, col


# ---------------------------------------------------------------------------------------------------- lusol --

def _w_matrix(nb, seed):
    """W of test_gpu_configs (nb copies of west0067's pattern on the diagonal), block b scaled by 1 + 1e-3 u_b"""
    g = golden("west0067")
    bp, bi, bx = g["C_p"].astype(np.int64), g["C_i"].astype(np.int64), g["C_x"]
    bs = 67
    u = synth.vec(nb, seed, 0.0, 1.0)
    Ai = (bi[None, :] + (np.arange(nb) * bs)[:, None]).reshape(-1).astype(np.int32)
    Ax = (bx[None, :] * (1.0 + 1e-3 * u)[:, None]).reshape(-1)
    Ap = np.concatenate([[0], np.cumsum(np.tile(np.diff(bp), nb))]).astype(np.int32)
    return sp.csc_matrix((Ax, Ai, Ap), shape=(nb * bs, nb * bs))


def _same_lu(fa, fb, n):
    assert list(fa.factors.pinv) == list(fb.factors.pinv), "a fresh factor pivots differently: pick another case"
    for name in ("L", "U"):
        for u, v in zip(_arr(getattr(fa.factors, name), n), _arr(getattr(fb.factors, name), n)):
            assert u.tobytes() == v.tobytes(), name


def test_lusol_refactor_on_W():
    c = cs()
    W, W2 = _w_matrix(1493, 20240604), _w_matrix(1493, 77)
    n = W.shape[0]
    for exact in (True, None):
        sol = c.lusol_factor(_cs(W), 0, 0.1, exact=exact)
        rng = np.random.default_rng(5)
        B = rng.uniform(-1, 1, (n, 64))
        sol.solve(c.dvec(B))                          # plans exist before the refactor: they must be rebuilt
        assert sol.refactor(_cs(W2)) is True
        info = sol.refactor_info()
        assert info["device_columns"] == n and info["host_columns"] == 0
        fresh = c.lusol_factor(_cs(W2), 0, 0.1, exact=exact)
        _same_lu(sol, fresh, n)
        for trans in (False, True):
            d1, d2 = c.dvec(B), c.dvec(B)
            sol.solve(d1, trans=trans)
            fresh.solve(d2, trans=trans)
            if exact:
                assert d1.numpy().tobytes() == d2.numpy().tobytes()
            else:
                got, want = d1.numpy(), d2.numpy()
                assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)) <= 1e-10
            b = B[:, 0].tolist()
            x1, x2 = list(b), list(b)
            sol.solve(x1, trans=trans)
            fresh.solve(x2, trans=trans)
            assert x1 == x2


def _uniform(S, seed):
    return _with(S, S.data * (1.0 + 1e-3 * np.random.default_rng(seed).uniform(0, 1)))


@pytest.mark.parametrize("name,order,host,perturb,tol", [("bcsstk16", 0, True, _columnwise, 0.001),
                                                         ("west0067", 0, False, _columnwise, 0.001),
                                                         ("west0067", 3, False, _uniform, 0.1)])
def test_lusol_refactor_paths(name, order, host, perturb, tol):
    c = cs()
    S = _fixture(name)
    n = S.shape[0]
    S2 = perturb(S, 3)
    sol = c.lusol_factor(_cs(S), order, tol, exact=True)
    L_read = list(sol.factors.L.x)
    b = np.linspace(-1, 1, n)
    sol.solve(list(b))
    assert sol.refactor(_cs(S2)) is True
    info = sol.refactor_info()
    assert info["device_columns"] + info["host_columns"] == n
    if host:
        assert info["host_columns"] > 96       # a component over 96 rows: the host loop (small ones beside it: the device)
    else:
        assert info["device_columns"] == n
    assert list(sol.factors.L.x) != L_read
    fresh = c.lusol_factor(_cs(S2), order, tol, exact=True)
    _same_lu(sol, fresh, n)
    for trans in (False, True):
        x1, x2 = b.tolist(), b.tolist()
        sol.solve(x1, trans=trans)
        fresh.solve(x2, trans=trans)
        assert x1 == x2
    assert sol.condest() == fresh.condest()
    bad = S2.data.copy()
    bad[:] = 0.0
    assert sol.refactor(bad) is False
    x3 = b.tolist()
    sol.solve(x3)
    x4 = b.tolist()
    fresh.solve(x4)
    assert x3 == x4
    with pytest.raises(ValueError):
        sol.refactor(np.zeros(S.nnz + 1))


def test_lusol_refactor_mixed_groups_with_duplicates():
    """one refactor, two groups: west0067 on the device, and a copy with duplicate entries (cs_spsolve assigns, the later
    entry of a row counts) on the host loop; L and U byte-equal to the rule on the factor's own pattern"""
    import refactor_oracle as R
    c = cs()
    S = _fixture("west0067")
    m = S.shape[0]
    p, i, x = [0], [], []
    for blk in range(2):
        for j in range(m):
            a, e = S.indptr[j], S.indptr[j + 1]
            i += (S.indices[a:e] + blk * m).tolist()
            x += S.data[a:e].tolist()
            if blk == 1 and j % 3 == 0 and e > a:
                i.append(int(S.indices[a]) + m)
                x.append(float(S.data[a]) * 2.0)
            p.append(len(i))
    n = 2 * m
    A = c.cs_spalloc(n, n, len(i), True, False)
    A.p, A.i, A.x = list(p), list(i), list(x)
    sol = c.lusol_factor(A, 0, 0.001, exact=True)
    N = sol.factors
    L0, U0 = (list(N.L.p), list(N.L.i), list(N.L.x)), (list(N.U.p), list(N.U.i), list(N.U.x))
    u = np.random.default_rng(9).uniform(-1, 1, n)
    x2 = np.asarray(x) * (1.0 + 1e-3 * u)[np.repeat(np.arange(n), np.diff(p))]
    assert sol.refactor(x2) is True
    info = sol.refactor_info()
    assert info["device_columns"] >= m and info["host_columns"] > 0 and info["device_columns"] + info["host_columns"] == n
    Lx, Ux, ok, ratio = R.refactor(L0, U0, N.pinv, (p, i, x2.tolist()))
    assert ok and ratio == info["pivot_ratio"]
    assert np.asarray(N.L.x[:len(Lx)]).tobytes() == np.asarray(Lx).tobytes()      # lists read before: updated in place
    assert np.asarray(N.U.x[:len(Ux)]).tobytes() == np.asarray(Ux).tobytes()
