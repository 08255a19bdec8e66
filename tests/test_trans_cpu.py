"""trans_oracle on the CPU: the two transposed-solve restatements solve A' x = b (backward error, and forward error against
scipy within the conditioning), and condest_dense is exact on diagonal matrices and never above the dense cond_1."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

import btf_oracle
import csparse_oracle as O
import trans_oracle as T
from conftest import golden


def _fixture(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])
    p = g["C_p"].astype(np.int64)
    S = sp.coo_matrix(sp.csc_matrix((g["C_x"][:p[n]], g["C_i"][:p[n]], p), shape=(m, n))).tocsc()
    S.sum_duplicates()
    return S


def _oracle_cs(S):
    S = sp.csc_matrix(S)
    A = O.cs_spalloc(S.shape[0], S.shape[1], max(S.nnz, 1), True, False)
    A.p, A.i, A.x = S.indptr.tolist(), S.indices.tolist() or [0], S.data.tolist() or [0.0]
    return A


def _random_dupl(n, seed):
    """A random sparse matrix with repeated (row, column) pairs summed by cs_dupl, a strong diagonal."""
    rng = np.random.default_rng(seed)
    nz = 6 * n
    rows = np.concatenate([rng.integers(0, n, nz), np.arange(n)])
    cols = np.concatenate([rng.integers(0, n, nz), np.arange(n)])
    vals = np.concatenate([rng.uniform(-1, 1, nz), np.full(n, 4.0)])
    A = O.cs_spalloc(n, n, len(rows), True, True)
    for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):
        O.cs_entry(A, r, c, v)
    C = O.cs_compress(A)
    O.cs_dupl(C)
    nnz = C.p[n]
    return sp.csc_matrix((np.asarray(C.x[:nnz]), np.asarray(C.i[:nnz]), np.asarray(C.p)), shape=(n, n))


def _cond1(S):
    D = S.toarray()
    return float(np.linalg.norm(D, 1) * np.linalg.norm(np.linalg.inv(D), 1))


def _check(S, x, b):
    """backward error of A' x = b at rounding level; forward error against scipy within the conditioning"""
    AT = sp.csc_matrix(S).T.tocsc()
    x = np.asarray(x)
    res = np.max(np.abs(AT @ x - b))
    berr = res / (abs(AT).sum(axis=1).max() * np.max(np.abs(x)) + np.max(np.abs(b)))
    assert berr <= 1e-12, berr
    want = spsolve(AT, b)
    ferr = np.max(np.abs(x - want)) / np.max(np.abs(want))
    assert ferr <= 1e-12 * max(1.0, _cond1(S)), ferr


def _lusol_check(S, permute, seed=0):
    """L U = A(p, q) from the oracle's cs_lu (natural order) of A(:, q): q None, or a random column permutation"""
    n = S.shape[0]
    A = _oracle_cs(S)
    q = np.random.default_rng(seed + 100).permutation(n).tolist() if permute else None
    Aq = O.cs_permute(A, None, q, True) if permute else A
    N = O.cs_lu(Aq, O.cs_sqr(0, Aq, False), 1.0)
    assert N is not None
    b = np.random.default_rng(seed).uniform(-1, 1, n)
    x = T.lusol_trans(N.L, N.U, N.pinv, q, b.tolist())
    _check(S, x, b)


@pytest.mark.parametrize("name", ["west0067", "fs_183_1"])
@pytest.mark.parametrize("permute", [False, True])
def test_lusol_trans_fixtures(name, permute):
    _lusol_check(_fixture(name), permute)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_lusol_trans_random_dupl(seed):
    _lusol_check(_random_dupl(40 + 20 * seed, seed), seed % 2 == 1, seed)


def _btf_factor(S):
    """btf_factor's factors from the CPU restatements (as test_btf_cpu does)."""
    n = S.shape[0]
    Ap, Ai, Ax = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    p, q, r, levels = btf_oracle.btf_order(n, Ap, Ai)
    D, F = btf_oracle.split(n, Ap, Ai, Ax, p, q, r)
    Dc = O.cs_spalloc(n, n, max(len(D[1]), 1), True, False)
    Dc.p, Dc.i, Dc.x = D[0], D[1] or [0], D[2] or [0.0]
    N = O.cs_lu(Dc, O.cs_sqr(0, Dc, False), 1.0)
    assert N is not None
    return N, F, p, q, r


def _btf_check(S, seed=0):
    S = sp.csc_matrix(S)
    S.sort_indices()
    n = S.shape[0]
    N, F, p, q, r = _btf_factor(S)
    b = np.random.default_rng(seed).uniform(-1, 1, n)
    x = T.btf_solve_trans(N.L, N.U, F, N.pinv, p, q, r, b.tolist())
    _check(S, x, b)
    return len(r) - 1


@pytest.mark.parametrize("name", ["fs_183_1", "west0067"])
def test_btf_trans_fixtures(name):
    assert _btf_check(_fixture(name)) > 1


@pytest.mark.parametrize("seed", [4, 5])
def test_btf_trans_reducible(seed):
    S, blocks, depth = btf_oracle.reducible(btf_oracle.block_sizes(300, seed), 6, seed)
    assert _btf_check(S, seed) == len(blocks)


def test_btf_trans_random_dupl():
    _btf_check(_random_dupl(80, 9), 9)


def test_btf_and_lusol_trans_agree():
    S, _, _ = btf_oracle.reducible(btf_oracle.block_sizes(200, 6), 4, 6)
    S = sp.csc_matrix(S)
    n = S.shape[0]
    b = np.linspace(-1, 1, n)
    N, F, p, q, r = _btf_factor(S)
    x1 = np.asarray(T.btf_solve_trans(N.L, N.U, F, N.pinv, p, q, r, b.tolist()))
    A = _oracle_cs(S)
    Sy = O.cs_sqr(0, A, False)
    N2 = O.cs_lu(A, Sy, 1.0)
    x2 = np.asarray(T.lusol_trans(N2.L, N2.U, N2.pinv, Sy.q, b.tolist()))
    assert np.max(np.abs(x1 - x2)) <= 1e-12 * _cond1(S) * np.max(np.abs(x2))


# ------------------------------------------------------------------------------------------------------ condest --

def test_condest_dense_exact_on_diagonal():
    for d in (np.array([2.0]), np.linspace(1, 7, 9), np.array([-3.0, 0.5, 8.0, -0.25, 1.0])):
        want = np.max(np.abs(d)) / np.min(np.abs(d))
        assert T.condest_dense(np.diag(d)) == pytest.approx(want, rel=1e-15)
    assert T.condest_dense(np.zeros((0, 0))) == 0.0


@pytest.mark.parametrize("seed", range(6))
def test_condest_dense_never_above_cond1(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 60))
    A = rng.uniform(-1, 1, (n, n)) + np.diag(rng.uniform(0, 3, n))
    est = T.condest_dense(A)
    c = np.linalg.norm(A, 1) * np.linalg.norm(np.linalg.inv(A), 1)
    assert 0.0 < est <= c * (1 + 1e-12)


def test_condest_dense_on_fixture():
    S = _fixture("west0067")
    est = T.condest_dense(S)
    assert est <= _cond1(S) * (1 + 1e-12)
    assert est >= 0.1 * _cond1(S)
