"""cs_dmperm / cs_maxtrans / cs_scc on the device: the reference test file's known answers, the canonical parts
against the CPU oracle (dm_oracle.py), the invariants of every result, determinism, edge cases and scale."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import dm_oracle
from conftest import golden

pytestmark = pytest.mark.gpu

NAMES = sorted(dm_oracle.KNOWN)


def cs():
    import csparse
    return csparse


def _mat(m, n, p, i, values=True):
    c = cs()
    p = np.asarray(p, dtype=np.int64)
    i = np.asarray(i, dtype=np.int64)[:p[n]]
    A = c.cs_spalloc(m, n, max(len(i), 1), values, False)
    A.p, A.i = p.tolist(), i.tolist()
    A.x = np.linspace(1.0, 2.0, len(i)).tolist() if values else None
    return A


def _fixture(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])
    p, i = g["C_p"].astype(np.int64), g["C_i"].astype(np.int64)
    return m, n, p, i[:p[n]]


def _pinned(m, n, p, i):
    """A device-resident matrix from numpy arrays (no host lists)."""
    c = cs()
    import _csx
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(m, n, _csx.pi(_csx.i32(p)), _csx.pi(_csx.i32(i)), None, h), "upload")
    return c._from_device(h, lambda nnz: max(nnz, 1))


def check_dm(m, n, p, i, d, known=None):
    """The invariants of a cs_dmperm result (numpy form); returns the fine blocks as (rows, cols) frozensets."""
    p = np.asarray(p, dtype=np.int64)
    i = np.asarray(i, dtype=np.int64)[:p[n]]
    P, Q, r, s, rr, cc, nb = (d["p"].astype(np.int64), d["q"].astype(np.int64), d["r"], d["s"], d["rr"], d["cc"],
                              d["nb"])
    assert np.array_equal(np.sort(P), np.arange(m)) and np.array_equal(np.sort(Q), np.arange(n))
    assert len(r) == nb + 1 and len(s) == nb + 1 and r[0] == 0 and s[0] == 0 and r[nb] == m and s[nb] == n
    assert np.all(np.diff(r) >= 0) and np.all(np.diff(s) >= 0)
    assert cc[0] == 0 and cc[4] == n and rr[0] == 0 and rr[4] == m
    assert np.all(np.diff(cc) >= 0) and np.all(np.diff(rr) >= 0)
    assert rr[1] == cc[2] - cc[1] and rr[2] - rr[1] == cc[3] - cc[2] and rr[3] - rr[2] == cc[4] - cc[3]
    # entries in the permuted positions
    col = np.repeat(np.arange(n), np.diff(p))
    pinv, qinv = np.empty(m, np.int64), np.empty(n, np.int64)
    pinv[P], qinv[Q] = np.arange(m), np.arange(n)
    pr, pc = pinv[i], qinv[col]
    # matched pairs on the three shifted diagonals are entries
    keys = np.unique(pr * max(n, 1) + pc)
    rr64, cc64 = rr.astype(np.int64), cc.astype(np.int64)
    for a, b, c0 in ((rr64[0], rr64[1], cc64[1]), (rr64[1], rr64[2], cc64[2]), (rr64[2], rr64[3], cc64[3])):
        k = np.arange(b - a, dtype=np.int64)
        want = (a + k) * max(n, 1) + (c0 + k)
        assert np.all(np.isin(want, keys, assume_unique=False))
    # block upper triangular: block of the row <= block of the column
    rb = np.searchsorted(r, pr, side="right") - 1
    cb = np.searchsorted(s, pc, side="right") - 1
    assert np.all(rb <= cb)
    blocks = set()
    for k in range(nb):
        blocks.add((frozenset(P[r[k]:r[k + 1]].tolist()), frozenset(Q[s[k]:s[k + 1]].tolist())))
    if known is not None:
        ns = int(np.sum((np.diff(r) == 1) & (np.diff(s) == 1)))
        assert (nb, ns, int(rr[3])) == known
    return blocks


def check_scc_blocks(m, n, p, i, d):
    """Every fine block of A(R2, C2) strongly connected (scipy), column identified with its matched row."""
    P, Q, r, s, rr, cc = d["p"], d["q"], d["r"], d["s"], d["rr"], d["cc"]
    S = sp.csc_matrix((np.ones(len(i)), np.asarray(i)[:p[n]], p), shape=(m, n))
    for k in range(d["nb"]):
        if s[k] < cc[2] or s[k] >= cc[3]:
            continue
        rows, cols = P[r[k]:r[k + 1]], Q[s[k]:s[k + 1]]
        assert len(rows) == len(cols)
        B = S[rows][:, cols]
        nc, _ = csgraph.connected_components(B, directed=True, connection="strong")
        assert nc == 1


@pytest.mark.parametrize("seed", [0, -1, 1])
@pytest.mark.parametrize("name", NAMES)
def test_dmperm_known_answers(name, seed):
    c = cs()
    m, n, p, i = _fixture(name)
    A = _mat(m, n, p, i)
    D = c.cs_dmperm(A, seed)
    assert isinstance(D, c.csd)
    assert len(D.p) == m and len(D.q) == n and len(D.r) == m + 6 and len(D.s) == n + 6
    assert len(D.rr) == 5 and len(D.cc) == 5
    d = dict(p=np.array(D.p), q=np.array(D.q), r=np.array(D.r[:D.nb + 1]), s=np.array(D.s[:D.nb + 1]),
             rr=np.array(D.rr), cc=np.array(D.cc), nb=D.nb)
    assert all(v == 0 for v in D.r[D.nb + 1:]) and all(v == 0 for v in D.s[D.nb + 1:])
    blocks = check_dm(m, n, p, i, d, dm_oracle.KNOWN[name])
    check_scc_blocks(m, n, p, i, d)
    o = dm_oracle.dm(m, n, p, i)
    P, Q, rr, cc = d["p"], d["q"], d["rr"], d["cc"]
    assert set(Q[:cc[2]].tolist()) == o["C01"] and set(Q[cc[2]:cc[3]].tolist()) == o["C2"]
    assert set(Q[cc[3]:].tolist()) == o["C3"]
    assert set(P[:rr[1]].tolist()) == o["R1"] and set(P[rr[1]:rr[2]].tolist()) == o["R2"]
    assert set(P[rr[2]:].tolist()) == o["R30"]
    assert blocks == o["blocks"]


@pytest.mark.parametrize("name", NAMES)
def test_maxtrans_is_maximum(name):
    c = cs()
    m, n, p, i = _fixture(name)
    A = _mat(m, n, p, i)
    S = sp.csc_matrix((np.ones(len(i)), i, p), shape=(m, n))
    for seed in (0, -1, 5):
        jm = np.array(c.cs_maxtrans(A, seed))
        assert len(jm) == m + n
        rm, cm = jm[:m], jm[m:]
        assert int(np.sum(cm >= 0)) == int(np.sum(rm >= 0)) == csgraph.structural_rank(S)
        for j in np.flatnonzero(cm >= 0):
            assert rm[cm[j]] == j and cm[j] in set(i[p[j]:p[j + 1]].tolist())


@pytest.mark.parametrize("name", ["west0067", "fs_183_1", "bcsstk16", "t1"])
def test_scc_block_upper_triangular(name):
    c = cs()
    m, n, p, i = _fixture(name)
    A = _mat(m, n, p, i)
    D = c.cs_scc(A)
    P, r, nb = np.array(D.p), np.array(D.r[:D.nb + 1]), D.nb
    assert np.array_equal(np.sort(P), np.arange(n)) and r[0] == 0 and r[nb] == n and np.all(np.diff(r) > 0)
    pinv = np.empty(n, np.int64)
    pinv[P] = np.arange(n)
    col = np.repeat(np.arange(n), np.diff(p))
    blk = np.searchsorted(r, pinv, side="right") - 1
    assert np.all(blk[i] <= blk[col])
    S = sp.csr_matrix((np.ones(len(i)), (i, col)), shape=(n, n))
    ncomp, lab = csgraph.connected_components(S, directed=True, connection="strong")
    assert ncomp == nb
    for k in range(nb):
        assert len(set(lab[P[r[k]:r[k + 1]]].tolist())) == 1


def test_determinism():
    c = cs()
    m, n, p, i = _fixture("mbeacxc")
    A = _mat(m, n, p, i)
    for seed in (0, 1, -1):
        a, b = c.dmperm_arrays(A, seed), c.dmperm_arrays(A, seed)
        for k in ("p", "q", "r", "s", "rr", "cc"):
            assert np.array_equal(a[k], b[k])
        assert c.cs_maxtrans(A, seed) == c.cs_maxtrans(A, seed)


def test_edge_cases():
    c = cs()
    for m, n in ((0, 0), (0, 3), (4, 0)):
        A = _mat(m, n, [0] * (n + 1), [])
        D = c.cs_dmperm(A, 0)
        d = c.dmperm_arrays(A, 0)
        check_dm(m, n, [0] * (n + 1), [], d)
        assert D.rr[3] == 0
        assert c.cs_maxtrans(A, 0) == [-1] * (m + n)
    # all-empty matrix
    d = c.dmperm_arrays(_mat(5, 4, [0] * 5, []), 1)
    check_dm(5, 4, [0] * 5, [], d)
    assert list(d["cc"]) == [0, 4, 4, 4, 4] and list(d["rr"]) == [0, 0, 0, 0, 5] and d["nb"] == 2
    # empty rows and columns, explicit zeros, pattern only, wide and tall
    rng = np.random.default_rng(3)
    for (m, n) in ((30, 30), (20, 45), (45, 20)):
        dense = rng.random((m, n)) < 0.08
        dense[:, 3] = False
        dense[5, :] = False
        S = sp.csc_matrix(dense.astype(float))
        p, i = S.indptr, S.indices
        o = dm_oracle.dm(m, n, p, i)
        for values in (True, False):
            A = _mat(m, n, p, i, values)
            if values:
                A.x = [0.0] * len(i)             # stored zeros are entries
            d = c.dmperm_arrays(A, 2)
            assert check_dm(m, n, p, i, d) == o["blocks"]
            check_scc_blocks(m, n, p, i, d)
    # not CSC
    T = c.cs_spalloc(3, 3, 3, True, True)
    assert c.cs_dmperm(T, 0) is None and c.cs_maxtrans(T, 0) is None and c.cs_scc(T) is None
    # cs_scc needs a square matrix
    assert c.cs_scc(_mat(3, 2, [0, 1, 2], [0, 1])) is None


def test_pinned_matrix_stays_on_the_device():
    c = cs()
    m, n, p, i = _fixture("west0067")
    A = _pinned(m, n, p, i)
    d = c.dmperm_arrays(A, 0)
    assert A._lazy                               # the host lists were never materialised
    assert check_dm(m, n, p, i, d) == dm_oracle.dm(m, n, p, i)["blocks"]


# ------------------------------------------------------------------ scale --

def planted(nblk_cols, seed, rank_loss=False):
    """Block upper triangular matrix with known fine blocks, rows and columns permuted at random.

    Returns m, n, S (scipy CSC, rows sorted) and the expected result: dict(blocks, sprank, C01, C3, R1, R30) --
    every fine block as (frozenset rows, frozenset cols), the structural rank and the coarse sets.  Blocks have 1 to
    1000 columns; a block of two or more is strongly connected (a cycle plus random entries inside it).

    rank_loss: the first block (37 columns) gains 5 empty columns and 6 columns that repeat the pattern of its own
    columns, the last block (23 rows) gains 3 empty rows and 4 rows that repeat its rows.  Columns of the first block
    hold rows of the first block only and rows of the last block hold columns of the last block only, so the
    alternating searches stop there: C0 u C1 = first block's columns + the 11 new ones, R1 = its rows, C3 = the last
    block's columns, R3 u R0 = its rows + the 7 new ones; the rank stays that of the square part."""
    rng = np.random.default_rng(seed)
    sizes = [37] if rank_loss else []
    tot = sum(sizes)
    while tot < nblk_cols:
        b = int(min(rng.integers(1, 1001) if rng.random() < 0.05 else rng.integers(1, 8), nblk_cols - tot))
        sizes.append(b)
        tot += b
    if rank_loss:
        sizes.append(23)
        tot += 23
    n0 = tot
    starts = np.concatenate([[0], np.cumsum(sizes)])
    blk = np.repeat(np.arange(len(sizes)), sizes)
    rows, cols = [np.arange(n0)], [np.arange(n0)]               # diagonal
    # a cycle inside every block of >= 2 columns: column j holds the row before it, plus random entries
    big = np.array(sizes) >= 2
    for b in np.flatnonzero(big):
        a, e = starts[b], starts[b + 1]
        k = np.arange(a, e)
        rows.append(np.roll(k, 1))
        cols.append(k)
        extra = int(sizes[b])
        rows.append(rng.integers(a, e, extra))
        cols.append(rng.integers(a, e, extra))
    # entries above the blocks: row block < column block
    jj = rng.integers(0, n0, n0)
    ii = (rng.random(n0) * starts[blk[jj]]).astype(np.int64)
    keep = starts[blk[jj]] > 0
    rows.append(ii[keep])
    cols.append(jj[keep])
    r = np.concatenate(rows)
    cl = np.concatenate(cols)
    m, n = n0, n0
    if rank_loss:
        lr, lc = [r], [cl]
        for t in range(6):                    # columns n0+5 .. n0+10 repeat columns 0..5 (first block)
            sel = cl == t
            lr.append(r[sel])
            lc.append(np.full(int(sel.sum()), n0 + 5 + t))
        last = starts[-2]
        for t in range(4):                    # rows n0+3 .. n0+6 repeat the first rows of the last block
            sel = r == last + t
            lr.append(np.full(int(sel.sum()), n0 + 3 + t))
            lc.append(cl[sel])
        r, cl = np.concatenate(lr), np.concatenate(lc)
        m, n = n0 + 7, n0 + 11
    S = sp.csc_matrix((np.ones(len(r)), (r, cl)), shape=(m, n))
    S.sum_duplicates()
    pr, pc = rng.permutation(m), rng.permutation(n)
    S = S[pr][:, pc].tocsc()
    S.sort_indices()
    rinv, cinv = np.empty(m, np.int64), np.empty(n, np.int64)
    rinv[pr], cinv[pc] = np.arange(m), np.arange(n)
    blocks = set()
    for b in range(len(sizes)):
        a, e = starts[b], starts[b + 1]
        R, Cc = rinv[a:e].tolist(), cinv[a:e].tolist()
        if rank_loss and b == 0:
            Cc += cinv[n0:n].tolist()
        if rank_loss and b == len(sizes) - 1:
            R += rinv[n0:m].tolist()
        blocks.add((frozenset(R), frozenset(Cc)))
    exp = dict(blocks=blocks, sprank=n0, nb=len(sizes))
    if rank_loss:
        a0, aL = starts[1], starts[-2]
        exp.update(C01=frozenset(cinv[:a0].tolist() + cinv[n0:n].tolist()), R1=frozenset(rinv[:a0].tolist()),
                   C3=frozenset(cinv[aL:n0].tolist()), R30=frozenset(rinv[aL:n0].tolist() + rinv[n0:m].tolist()))
    return m, n, S, exp


def test_planted_structure_1m():
    c = cs()
    m, n, S, exp = planted(1_000_000, 11)
    p, i = S.indptr.astype(np.int64), S.indices.astype(np.int64)
    A = _pinned(m, n, p, i)
    d = c.dmperm_arrays(A, 0)
    got = check_dm(m, n, p, i, d)
    assert int(d["rr"][3]) == n and d["nb"] == exp["nb"]
    assert got == exp["blocks"]


def test_planted_rank_loss_1m():
    """Empty and repeated columns and rows at scale: C0, C1, C3 and R0 non-empty, the exact sets known from the plant."""
    c = cs()
    m, n, S, exp = planted(1_000_000, 13, rank_loss=True)
    p, i = S.indptr.astype(np.int64), S.indices.astype(np.int64)
    A = _pinned(m, n, p, i)
    for seed in (0, 3):
        d = c.dmperm_arrays(A, seed)
        got = check_dm(m, n, p, i, d)
        P, Q, rr, cc = d["p"], d["q"], d["rr"], d["cc"]
        assert int(rr[3]) == exp["sprank"] and d["nb"] == exp["nb"]
        assert cc[1] > 0 and cc[2] > cc[1] and rr[3] < m and cc[3] < n
        assert frozenset(Q[:cc[2]].tolist()) == exp["C01"] and frozenset(P[:rr[1]].tolist()) == exp["R1"]
        assert frozenset(Q[cc[3]:].tolist()) == exp["C3"] and frozenset(P[rr[2]:].tolist()) == exp["R30"]
        assert got == exp["blocks"]


def test_planted_rank_loss():
    """Empty columns and duplicate-pattern columns lose rank: the sets come from the CPU oracle at this size."""
    c = cs()
    _, n, S, _ = planted(3000, 12)
    S = S.tolil()
    S[:, 7] = 0
    S[:, 11] = S[:, 13]
    S[:, 17] = S[:, 13]
    S[40, :] = 0
    S = S.tocsc()
    S.eliminate_zeros()
    S.sort_indices()
    p, i = S.indptr, S.indices
    o = dm_oracle.dm(n, n, p, i)
    assert o["sprank"] == csgraph.structural_rank(S) < n
    for seed in (0, 7):
        d = c.dmperm_arrays(_pinned(n, n, p, i), seed)
        assert check_dm(n, n, p, i, d) == o["blocks"] and int(d["rr"][3]) == o["sprank"]


def _gen(fn, *args):
    c = cs()
    import _csx
    h = _csx.new_handle()
    _csx.check(getattr(_csx.lib(), fn)(*args, h), fn)
    return c._from_device(h, lambda nnz: max(nnz, 1))


def test_grand_against_scipy():
    c = cs()
    n = 1_000_000
    A = _gen("csx_gen_grand_uniform", n, 3, 99)
    d = c.dmperm_arrays(A, 0)
    m2, n2, nnz, _ = A._dev.info()
    p, i = np.array(A.p, dtype=np.int64), np.array(A.i[:nnz], dtype=np.int64)
    S = sp.csc_matrix((np.ones(len(i)), i, p), shape=(n, n))
    check_dm(n, n, p, i, d)
    assert int(d["rr"][3]) == csgraph.structural_rank(S)
    jm = np.array(c.maxtrans_array(A, 3))
    assert int(np.sum(jm[:n] >= 0)) == int(d["rr"][3])
    # the fine blocks of A(R2, C2) are exactly scipy's strong components of that square part (matched pairs on its
    # diagonal): as many blocks as components, and every block strongly connected
    P, Q, r, s, rr, cc = d["p"], d["q"], d["r"], d["s"], d["rr"], d["cc"]
    B = S[P[rr[1]:rr[2]]][:, Q[cc[2]:cc[3]]]
    ncomp, lab = csgraph.connected_components(B, directed=True, connection="strong")
    fine = [k for k in range(d["nb"]) if cc[2] <= s[k] < cc[3]]
    assert len(fine) == ncomp
    for k in fine:
        assert len(np.unique(lab[s[k] - cc[2]:s[k + 1] - cc[2]])) == 1


def test_gspd_symmetric():
    c = cs()
    A = _gen("csx_gen_gspd", 4000, 16, 5)
    n = A.n
    d = c.dmperm_arrays(A, 0)
    m2, n2, nnz, _ = A._dev.info()
    p, i = np.array(A.p, dtype=np.int64), np.array(A.i[:nnz], dtype=np.int64)
    check_dm(n, n, p, i, d)
    S = sp.csc_matrix((np.ones(len(i)), i, p), shape=(n, n))
    ncomp, _ = csgraph.connected_components(S, directed=True, connection="strong")
    assert d["nb"] == ncomp and int(d["rr"][3]) == n


def test_deep_bidiagonal_chain():
    c = cs()
    n = 200_000
    rng = np.random.default_rng(5)
    r = np.concatenate([np.arange(n), np.arange(n - 1)])
    cl = np.concatenate([np.arange(n), np.arange(1, n)])
    pr, pc = rng.permutation(n), rng.permutation(n)
    rinv, cinv = np.empty(n, np.int64), np.empty(n, np.int64)
    rinv[pr], cinv[pc] = np.arange(n), np.arange(n)
    S = sp.csc_matrix((np.ones(len(r)), (rinv[r], cinv[cl])), shape=(n, n))
    S.sort_indices()
    p, i = S.indptr.astype(np.int64), S.indices.astype(np.int64)
    d = c.dmperm_arrays(_pinned(n, n, p, i), 0)
    check_dm(n, n, p, i, d)
    assert d["nb"] == n and int(d["rr"][3]) == n


def _block_lower_bidiagonal(k):
    """k full 2 x 2 diagonal blocks in natural order, block b + 1 holding an entry in column 2b (below the diagonal):
    the components form one chain whose edges run from high indices to low ones (a 1D upwind transport operator with
    two unknowns per cell).  Its diagonal is zero-free and the trim peels nothing."""
    b = np.arange(k)
    r = np.concatenate([2 * b, 2 * b + 1, 2 * b, 2 * b + 1, 2 * b[1:]])
    c = np.concatenate([2 * b, 2 * b, 2 * b + 1, 2 * b + 1, 2 * b[:-1]])
    n = 2 * k
    S = sp.csc_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    S.sort_indices()
    return n, S.indptr.astype(np.int64), S.indices.astype(np.int64)


def test_block_lower_bidiagonal_natural_order():
    """A chain of 20 000 strongly connected 2 x 2 blocks whose order is the reverse of index order: the colouring
    must not lose one component per round of colouring (that is a quadratic number of rounds)."""
    c = cs()
    k = 20_000
    n, p, i = _block_lower_bidiagonal(k)
    want = set((frozenset((2 * b, 2 * b + 1)), frozenset((2 * b, 2 * b + 1))) for b in range(k))
    A = _pinned(n, n, p, i)
    D = c.cs_scc(A)
    assert D.nb == k
    rounds = c.dmperm_rounds()
    assert rounds["colour"] <= 2 * (n + n + 1)
    P, r = np.array(D.p), np.array(D.r[:k + 1])
    pinv = np.empty(n, np.int64)
    pinv[P] = np.arange(n)
    col = np.repeat(np.arange(n), np.diff(p))
    blk = np.searchsorted(r, pinv, side="right") - 1
    assert np.all(blk[i] <= blk[col])
    assert set(frozenset(P[r[b]:r[b + 1]].tolist()) for b in range(k)) == set(x for x, _ in want)
    for seed in (0, 1):
        d = c.dmperm_arrays(A, seed)
        assert check_dm(n, n, p, i, d) == want and d["nb"] == k
        assert c.dmperm_rounds()["colour"] <= 2 * (n + n + 1)

