"""btf_factor on the device: x byte-equal to btf_oracle run on the factor's own factors, for lists and dvec blocks of
every width; the structure of the factors; the cases that give None; a 1M-row matrix by a fixed-point check against the
C oracle and the backward error of every column."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

import btf_oracle
from conftest import golden

pytestmark = pytest.mark.gpu


def cs():
    import csparse
    return csparse


def _fixture(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])      # the reference test file's C (dm_oracle.KNOWN)
    p = g["C_p"].astype(np.int64)
    S = sp.coo_matrix(sp.csc_matrix((g["C_x"][:p[n]], g["C_i"][:p[n]], p), shape=(m, n))).tocsc()
    S.sum_duplicates()
    return S


def _cs(S):
    """A host-list `cs` of a scipy matrix."""
    S = S.tocsc()
    A = cs().cs_spalloc(S.shape[0], S.shape[1], max(S.nnz, 1), True, False)
    A.p, A.i, A.x = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    return A


def _device(S):
    """A device-resident `cs` of a scipy matrix (no host lists)."""
    import _csx
    S = S.tocsc()
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(S.shape[0], S.shape[1], _csx.pi(_csx.i32(S.indptr)), _csx.pi(_csx.i32(S.indices)),
                                         _csx.pd(_csx.f64(S.data)), h), "upload")
    return cs()._from_device(h, lambda nnz: max(nnz, 1))


def _sp(M, n):
    nnz = M.p[n]
    return sp.csc_matrix((np.asarray(M.x[:nnz], float), np.asarray(M.i[:nnz]), np.asarray(M.p[:n + 1])), shape=(n, n))


def _oracle(sol, b):
    f = sol.factors
    return np.asarray(btf_oracle.solve(f.L, f.U, f.F, f.pinv, f.p, f.q, f.r, list(b)))


def check_structure(S, sol, seed=0):
    """C = A(p, q) block upper triangular; blocks = dmperm's fine blocks; D + F = C; F reaches only earlier-solved blocks."""
    c = cs()
    f = sol.factors
    n = S.shape[0]
    p, q, r, lev = f.p.astype(np.int64), f.q.astype(np.int64), f.r.astype(np.int64), f.levels
    assert np.array_equal(np.sort(p), np.arange(n)) and np.array_equal(np.sort(q), np.arange(n))
    nb = len(r) - 1
    assert r[0] == 0 and r[nb] == n and np.all(np.diff(r) > 0) and len(lev) == nb
    C = S.tocsc()[p][:, q].tocoo()
    blk = np.repeat(np.arange(nb), np.diff(r))
    assert np.all(blk[C.row] <= blk[C.col])
    d = c.dmperm_arrays(_cs(S), seed)
    want = set((frozenset(d["p"][d["r"][k]:d["r"][k + 1]].tolist()), frozenset(d["q"][d["s"][k]:d["s"][k + 1]].tolist()))
               for k in range(d["nb"]))
    got = set((frozenset(p[r[k]:r[k + 1]].tolist()), frozenset(q[r[k]:r[k + 1]].tolist())) for k in range(nb))
    assert got == want
    D, F = _sp(f.D, n).tocoo(), _sp(f.F, n).tocoo()
    assert np.all(blk[D.row] == blk[D.col])
    assert np.all(blk[F.row] < blk[F.col])
    diff = (_sp(f.D, n) + _sp(f.F, n) - S.tocsc()[p][:, q]).tocsc()
    diff.eliminate_zeros()
    assert diff.nnz == 0
    assert D.nnz + F.nnz == C.nnz
    assert np.all(np.diff(lev) <= 0)
    assert np.all(lev[blk[F.row]] > lev[blk[F.col]])        # solved before: a lower level
    has_f = np.zeros(nb, bool)
    has_f[blk[F.row]] = True
    assert np.all((lev == 0) == ~has_f)


def check_exact(S, widths=(1, 2, 7, 64, 65, 130), seed=1):
    """x byte-equal to the oracle; every column of a block byte-equal to the list solve of that column; reruns equal."""
    c = cs()
    n = S.shape[0]
    sol = c.btf_factor(_cs(S))
    assert sol is not None
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1, 1, n)
    x = b.tolist()
    assert sol.solve(x) is True
    x = np.asarray(x)
    assert x.tobytes() == _oracle(sol, b).tobytes()
    for k in widths:
        B = rng.uniform(-1, 1, (n, k))
        dB = c.dvec(B)
        assert sol.solve(dB) is True
        X = dB.numpy().reshape(n, k)
        for col in range(k):
            xc = B[:, col].tolist()
            sol.solve(xc)
            assert np.asarray(xc).tobytes() == X[:, col].tobytes(), (k, col)
        dB2 = c.dvec(B)
        sol.solve(dB2)
        assert dB2.numpy().reshape(n, k).tobytes() == X.tobytes()
    return sol


@pytest.mark.parametrize("name", ["fs_183_1", "west0067", "bcsstk16"])
def test_fixture_exact(name):
    S = _fixture(name)
    sol = check_exact(S, widths=(1, 2, 7, 64, 65, 130) if name != "bcsstk16" else (1, 7, 65))
    check_structure(S, sol)
    nb = {"fs_183_1": 38, "west0067": 2, "bcsstk16": 75}[name]
    assert sol.info()["blocks"] == nb


def _generated_20k():
    sizes = btf_oracle.block_sizes(20000, 7, big=(500,))
    return btf_oracle.reducible(sizes, 30, 7)


def test_generated_20k_exact_and_structure():
    S, blocks, depth = _generated_20k()
    sol = check_exact(S)
    check_structure(S, sol)
    info = sol.info()
    assert info["levels"] == depth == 30
    assert info["large_blocks"] == 1 and info["max_block"] == 500
    assert info["blocks"] == len(blocks)
    f = sol.factors
    p, q, r = f.p, f.q, f.r
    got = set((frozenset(p[r[k]:r[k + 1]].tolist()), frozenset(q[r[k]:r[k + 1]].tolist())) for k in range(len(r) - 1))
    assert got == blocks
    b = np.linspace(-1, 1, S.shape[0])
    x = b.tolist()
    sol.solve(x)
    want = spsolve(S.tocsc(), b)
    assert np.linalg.norm(np.asarray(x) - want) <= 1e-10 * np.linalg.norm(want)


def test_device_resident_input():
    S, _, _ = btf_oracle.reducible(btf_oracle.block_sizes(3000, 3), 5, 3)
    c = cs()
    a, b = c.btf_factor(_cs(S)), c.btf_factor(_device(S))
    v = np.linspace(0, 1, S.shape[0])
    x1, x2 = v.tolist(), v.tolist()
    a.solve(x1)
    b.solve(x2)
    assert np.asarray(x1).tobytes() == np.asarray(x2).tobytes()


# ------------------------------------------------------------------------------------------------------- edges --

def test_none_for_non_square():
    c = cs()
    assert c.btf_factor(_cs(_fixture("mbeacxc"))) is None      # 492 x 490
    assert c.btf_factor(_cs(sp.random(30, 40, 0.2, random_state=1, format="csc") + sp.eye(30, 40))) is None


def test_none_for_structurally_singular():
    """Square and structurally singular, as the rank-loss variant of the dmperm tests: columns that repeat one pattern."""
    n = 200
    S = (sp.eye(n) * 4 + sp.random(n, n, 0.01, random_state=5)).tolil()
    for j in (3, 4, 5):            # three columns with the single row 7: rank falls by two
        S[:, j] = 0
        S[7, j] = 1.0 + j
    S = S.tocsc()
    from scipy.sparse import csgraph
    assert csgraph.structural_rank(S) < n
    assert cs().btf_factor(_cs(S)) is None


def test_none_for_numerically_singular_block():
    S = sp.csc_matrix(np.array([[1.0, 1.0, 0.5], [1.0, 1.0, 0.0], [0.0, 0.0, 2.0]]))
    assert cs().btf_factor(_cs(S)) is None


def test_none_for_non_csc():
    c = cs()
    T = c.cs_spalloc(3, 3, 3, True, True)
    for k in range(3):
        c.cs_entry(T, k, k, 1.0)
    assert c.btf_factor(T) is None
    assert c.btf_factor(None) is None


def test_diagonal():
    c = cs()
    n = 1000
    d = np.linspace(1, 3, n)
    S = sp.diags(d).tocsc()
    sol = c.btf_factor(_cs(S))
    info = sol.info()
    assert info["blocks"] == n and info["fnz"] == 0 and info["levels"] == 1
    b = np.linspace(-2, 2, n)
    x = b.tolist()
    sol.solve(x)
    assert np.asarray(x).tobytes() == _oracle(sol, b).tobytes()
    assert np.allclose(x, b / d, rtol=1e-15)


def test_irreducible_agrees_with_lusol():
    c = cs()
    n = 300
    rng = np.random.default_rng(2)
    S = (sp.random(n, n, 0.02, random_state=2) + sp.diags(np.full(n, 3.0)) + sp.diags(np.ones(n - 1), 1)
         + sp.diags(np.ones(1), -(n - 1))).tocsc()
    sol = c.btf_factor(_cs(S))
    assert sol.info()["blocks"] == 1 and sol.info()["fnz"] == 0
    b = rng.uniform(-1, 1, n)
    x1, x2 = b.tolist(), b.tolist()
    sol.solve(x1)
    c.lusol_factor(_cs(S)).solve(x2)
    assert np.max(np.abs(np.asarray(x1) - x2)) <= 1e-10 * np.max(np.abs(x2))
    assert np.asarray(x1).tobytes() == _oracle(sol, b).tobytes()


def test_chain_of_2x2_blocks_natural_order():
    """Block lower bidiagonal, 2 000 blocks of 2 x 2 in natural order: one level per block."""
    c = cs()
    nbk = 2000
    n = 2 * nbk
    rows, cols, vals = [], [], []
    for k in range(nbk):
        a = 2 * k
        rows += [a, a + 1, a, a + 1]
        cols += [a, a, a + 1, a + 1]
        vals += [4.0, 1.0, 1.0, 5.0]
        if k:
            rows.append(a)
            cols.append(a - 1)
            vals.append(-1.0)
    S = sp.csc_matrix((vals, (rows, cols)), shape=(n, n))
    sol = check_exact(S, widths=(1, 3, 64))
    check_structure(S, sol)
    info = sol.info()
    assert info["blocks"] == nbk and info["levels"] == nbk and info["large_blocks"] == 0


# ------------------------------------------------------------------------------------------------------- scale --

def test_scale_1m_128_rhs():
    import c_oracle as CO
    c = cs()
    sizes = btf_oracle.block_sizes(1_000_000, 11)
    assert len(sizes) > 100_000
    S, blocks, depth = btf_oracle.reducible(sizes, 8, 11)
    n = S.shape[0]
    sol = c.btf_factor(_device(S))
    assert sol is not None
    info = sol.info()
    assert info["blocks"] == len(sizes) and info["levels"] == depth and info["large_blocks"] == 0
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
    nA = abs(S).sum(axis=1).max()
    for col in range(k):
        x = X[:, col]
        z = x[f.q]
        rr = CO.gaxpy(n, n, Fp, Fi, Fx, z, B[f.p, col])
        w = CO.usolve(n, Up, Ui, Ux, CO.lsolve(n, Lp, Li, Lx, CO.ipvec(f.pinv, rr)))
        assert w.tobytes() == z.tobytes(), col
        res = np.max(np.abs(S @ x - B[:, col]))
        assert res / (nA * np.max(np.abs(x)) + np.max(np.abs(B[:, col]))) < 1e-13, col
