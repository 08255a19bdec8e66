"""btf_oracle on the CPU: its solve sequence against scipy's solvers, its generator against scipy's strong components."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph
from scipy.sparse.linalg import spsolve

import btf_oracle
import csparse_oracle as O
from conftest import golden


def _fixture(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])      # the reference test file's C (dm_oracle.KNOWN)
    p = g["C_p"].astype(np.int64)
    S = sp.coo_matrix(sp.csc_matrix((g["C_x"][:p[n]], g["C_i"][:p[n]], p), shape=(m, n))).tocsc()
    S.sum_duplicates()      # (cs_lu's scatter assigns: a matrix with duplicates would be factored without them)
    return S


def _factor(S):
    """The factors btf_factor defines, from the CPU restatements: order, split, the oracle's cs_lu of D."""
    n = S.shape[0]
    Ap, Ai, Ax = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    p, q, r, levels = btf_oracle.btf_order(n, Ap, Ai)
    D, F = btf_oracle.split(n, Ap, Ai, Ax, p, q, r)
    Dc = O.cs_spalloc(n, n, max(len(D[1]), 1), True, False)
    Dc.p, Dc.i, Dc.x = D[0], D[1] or [0], D[2] or [0.0]
    N = O.cs_lu(Dc, O.cs_sqr(0, Dc, False), 1.0)
    assert N is not None
    return N, F, p, q, r, levels


def _check_structure(S, F, p, q, r, levels):
    n = S.shape[0]
    C = S[p][:, q].tocsc()
    blk = np.repeat(np.arange(len(r) - 1), np.diff(r))
    Cc = C.tocoo()
    assert np.all(blk[Cc.row] <= blk[Cc.col])            # block upper triangular
    Fm = sp.csc_matrix((F[2], F[1], F[0]), shape=(n, n)).tocoo()
    assert np.all(blk[Fm.row] < blk[Fm.col])
    lev = np.asarray(levels)
    assert np.all(lev[blk[Fm.row]] > lev[blk[Fm.col]])    # F reaches lower levels only
    assert np.all(np.diff(lev) <= 0)


def _solve(S, b):
    N, F, p, q, r, levels = _factor(S)
    _check_structure(S, F, p, q, r, levels)
    return np.asarray(btf_oracle.solve(N.L, N.U, F, N.pinv, p, q, r, b.tolist()))


@pytest.mark.parametrize("seed,depth", [(1, 1), (2, 3), (3, 6)])
def test_oracle_generated(seed, depth):
    sizes = btf_oracle.block_sizes(300, seed)
    S, blocks, nlev = btf_oracle.reducible(sizes, depth, seed)
    assert nlev == depth
    b = np.random.default_rng(seed).uniform(-1, 1, S.shape[0])
    x = _solve(S, b)
    want = spsolve(S.tocsc(), b)
    assert np.linalg.norm(x - want) <= 1e-10 * np.linalg.norm(want)


def test_oracle_west0067():
    S = _fixture("west0067")
    b = np.linspace(1.0, 2.0, S.shape[0])
    x = _solve(S, b)
    want = spsolve(S, b)
    assert np.linalg.norm(x - want) <= 1e-10 * np.linalg.norm(want)


def test_oracle_fs_183_1_backward_error():
    S = _fixture("fs_183_1")          # condition number about 2e13: judged by the backward error
    b = np.linspace(1.0, 2.0, S.shape[0])
    x = _solve(S, b)
    res = np.linalg.norm(S @ x - b, np.inf)
    nA = abs(S).sum(axis=1).max()
    assert res / (nA * np.linalg.norm(x, np.inf) + np.linalg.norm(b, np.inf)) < 1e-14


@pytest.mark.parametrize("seed,depth", [(4, 1), (5, 4), (6, 9)])
def test_generator_blocks_are_strong_components(seed, depth):
    sizes = btf_oracle.block_sizes(2000, seed, big=(120,))
    S, blocks, nlev = btf_oracle.reducible(sizes, depth, seed)
    n = S.shape[0]
    assert nlev == depth and len(blocks) == len(sizes)
    # a maximum matching puts a zero-free diagonal in place; the strong components of that matrix's graph are the blocks
    match = csgraph.maximum_bipartite_matching(S.tocsr(), perm_type="row")     # match[j] = row matched to column j
    assert np.all(match >= 0)
    S2 = S[match].tocsc()
    ncomp, lab = csgraph.connected_components(S2, directed=True, connection="strong")
    assert ncomp == len(blocks)
    got = {}
    for j in range(n):
        got.setdefault(lab[j], set()).add(j)
    assert set((frozenset(match[list(c)].tolist()), frozenset(c)) for c in got.values()) == blocks
    # diagonally dominant rows
    A = abs(S).tocsr()
    d = np.asarray(A.max(axis=1).todense()).ravel()
    off = np.asarray(A.sum(axis=1)).ravel() - d
    assert np.all(d > off)
