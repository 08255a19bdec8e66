"""csx_residual_sym_block / residual_block(sym=True) and csx_norm1_sym: R = B - S X for the symmetric matrix in
A's upper triangle, byte-equal to the host rule csx_residual_sym_host (which tests/test_residual_sym_cpu.py pins to the Python
restatement) for column counts on both sides of every template choice, at shapes around the 64-row tile and the U = 8 entries
in flight of either phase; the storages of one operator; the placement of the maxima, R == 0 and R aliasing B, the argument
checks; csx_norm1_sym against the restatement."""
import ctypes as C

import numpy as np
import pytest

import residual_sym_cases as SC
import residual_sym_oracle as RSO
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

KS = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 66, 67, 130)


def _random(n, seed, per_col=6):
    """unsorted columns with duplicates, explicit (signed) zeros, empty columns and rows, entries on both sides of the diagonal"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 2 * per_col, n)
    if n > 8:
        counts[rng.choice(n, n // 8, replace=False)] = 0
    live = rng.choice(n, max(1, (4 * n) // 5), replace=False)
    nnz = int(counts.sum())
    Ai = rng.choice(live, nnz)
    Ax = rng.standard_normal(nnz)
    Ax[rng.random(nnz) < 0.05] = 0.0
    Ax[rng.random(nnz) < 0.02] = -0.0
    Ap = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return n, Ap, Ai.astype(np.int32), Ax


SHAPES = {
    "1": lambda: (1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-1.5])),
    "63": lambda: _random(63, 1),
    "64": lambda: _random(64, 2),
    "65": lambda: _random(65, 3),
    "edges200": lambda: SC.edge_matrix(),
}


def _host_cs(cs, n, Ap, Ai, Ax):
    A = cs.cs_spalloc(n, n, max(len(Ai), 1), True, False)
    A.p, A.i, A.x = np.asarray(Ap).tolist(), np.asarray(Ai).tolist() or [0], np.asarray(Ax).tolist() or [0.0]
    return A


def _rule(n, Ap, Ai, Ax, k, X, B):
    """the host rule: (R, omega, rnorm)"""
    import _csx
    X, B = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    R, omega, rnorm = np.empty(n * k), np.empty(k), np.empty(k)
    Ap, Ai, Ax = np.ascontiguousarray(Ap, np.int32), np.ascontiguousarray(Ai, np.int32), np.ascontiguousarray(Ax, np.float64)
    _csx.check(_csx.load().csx_residual_sym_host(n, _csx.pi(Ap), _csx.pi(Ai), _csx.pd(Ax), k, _csx.pd(X), _csx.pd(B), _csx.pd(R),
                                                 _csx.pd(omega), _csx.pd(rnorm)), "csx_residual_sym_host")
    return R.reshape(n, k), omega, rnorm


def _blocks(n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k)) * 4.0, rng.standard_normal((n, k))


def _view(cs, lib, block, offset, count):
    """a handle to count doubles of a dvec from `offset` doubles on"""
    import _csx
    h = _csx.new_handle()
    _csx.check(lib.csx_vec_wrap(C.c_void_p(block.device_ptr() + 8 * offset), count, h))
    return h


def _check_the_edge_matrix(n, Ap, Ai, Ax):
    """the 200-row matrix has what the tests count on"""
    assert n == 200
    first = [sum(1 for q in range(Ap[r], Ap[r + 1]) if Ai[q] <= r) for r in range(n)]
    rows = RSO.rows_of(n, Ap, Ai, Ax)
    pairs = {(first[r], len(rows[r]) - first[r]) for r in range(40, 65)}
    assert pairs == {(a, b) for a in (0, 1, 7, 8, 9) for b in (0, 1, 7, 8, 9)}
    cols = np.repeat(np.arange(n), np.diff(Ap))
    assert all(not rows[r] and Ap[r] == Ap[r + 1] and not (Ai == r).any() for r in range(100, 110))    # empty rows and columns
    assert not ((Ai == 70) & (cols == 70)).any() and rows[70]                                            # a missing diagonal
    assert any((np.diff(Ai[Ap[j]:Ap[j + 1]]) < 0).any() for j in range(n))                               # unsorted
    keys = (cols * n + Ai).tolist()
    dup = {t for t in keys if keys.count(t) > 1}
    assert any(t // n > t % n for t in dup) and any(t // n == t % n for t in dup) and any(t // n < t % n for t in dup)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_byte_equal_to_the_host_rule(cs, shape):
    n, Ap, Ai, Ax = SHAPES[shape]()
    if shape == "edges200":
        _check_the_edge_matrix(n, Ap, Ai, Ax)
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    for k in KS:
        X, B = _blocks(n, k, 10 * k)
        ref, wr, ar = _rule(n, Ap, Ai, Ax, k, X, B)
        R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), sym=True)
        assert (R.n, R.k) == (n, k)
        assert R.numpy().tobytes() == ref.tobytes(), (shape, k)
        assert omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes(), (shape, k)
        assert rnorm.tobytes() == np.max(np.abs(ref), axis=0).tobytes()


def test_an_unaligned_block_takes_the_single_column_route(cs):
    """k = 66 and 130 from a block that starts 8 bytes off a 16-byte boundary: the 16-byte loads are refused, the bytes stay"""
    import _csx
    lib = _csx.lib()
    n, Ap, Ai, Ax = SHAPES["edges200"]()
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    for k in (66, 130):
        X, B = _blocks(n, k, k)
        ref, wr, ar = _rule(n, Ap, Ai, Ax, k, X, B)
        for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            blocks = []
            for v, o in zip((X, B, np.zeros((n, k))), off):
                h = np.zeros(n * k + 1)
                h[o:o + n * k] = v.reshape(-1)
                blocks.append(cs.dvec(h))
            assert all(blk.device_ptr() % 16 == 0 for blk in blocks)
            hs = [_view(cs, lib, blk, o, n * k) for blk, o in zip(blocks, off)]
            omega, rnorm = np.empty(k), np.empty(k)
            _csx.check(lib.csx_residual_sym_block(A._dev.handle, hs[0], hs[1], hs[2], k, _csx.pd(omega), _csx.pd(rnorm)))
            got = blocks[2].numpy().reshape(-1)[off[2]:off[2] + n * k]
            assert got.tobytes() == ref.tobytes() and omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes(), (k, off)
            for h in hs:
                _csx.free(h)


@pytest.mark.parametrize("source", ["edges200", "64", "grid"])
def test_the_storages_of_one_operator(cs, source):
    import _csx
    if source == "grid":
        from chol_refactor_cases import with_dups_and_lower
        n, p, i, x = with_dups_and_lower(12, 3)
        stored = (n, np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x))
    else:
        stored = SHAPES[source]()
    n = stored[0]
    for k in (3, 66):
        X, B = _blocks(n, k, k + 1)
        dX, dB = cs.dvec(X), cs.dvec(B)
        want = _rule(*stored, k, X, B)
        for other in (stored, SC.upper_only(*stored), SC.with_lower(*stored, 1, False), SC.with_lower(*stored, 2, True)):
            R, omega, rnorm = cs.residual_block(_host_cs(cs, *other), dX, dB, sym=True)
            assert R.numpy().tobytes() == want[0].tobytes() and omega.tobytes() == want[1].tobytes()
            assert rnorm.tobytes() == want[2].tobytes()
        full = _host_cs(cs, *SC.full_sorted(*stored))
        R, omega, rnorm = cs.residual_block(full, dX, dB, sym=True)
        G, wg, ag = cs.residual_block(full, dX, dB)
        assert R.numpy().tobytes() == G.numpy().tobytes() and omega.tobytes() == wg.tobytes() and rnorm.tobytes() == ag.tobytes()
        omega2, rnorm2 = np.empty(k), np.empty(k)
        with cs._Resident(full) as d:
            _csx.check(_csx.lib().csx_residual_block(d.handle, dX.handle, dB.handle, 0, k, 0, _csx.pd(omega2), _csx.pd(rnorm2)))
        assert omega2.tobytes() == omega.tobytes() and rnorm2.tobytes() == rnorm.tobytes()


def test_maximum_in_the_last_row_of_the_last_tile_and_the_last_column(cs):
    """65 rows: the last tile holds row 64 alone.  A huge b there makes that row's |r| and its ratio (about 1, the bound of
    every ratio) the column's maxima; with it in the last column only, that column alone reports it."""
    n, Ap, Ai, Ax = SHAPES["65"]()
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    for k in (1, 5, 64, 66, 130):
        X, B = _blocks(n, k, k)
        B[n - 1, k - 1] = 1e30
        ref, wr, ar = _rule(n, Ap, Ai, Ax, k, X, B)
        R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), sym=True)
        assert R.numpy().tobytes() == ref.tobytes()
        assert omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
        assert rnorm[k - 1] == abs(ref[n - 1, k - 1]) and rnorm[k - 1] > 1e29 and omega[k - 1] > 0.99
        assert (rnorm[:k - 1] < 1e29).all()


def test_a_nan_stays_in_its_column(cs):
    n, Ap, Ai, Ax = SHAPES["65"]()
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    k = 66
    X, B = _blocks(n, k, 5)
    cols = np.repeat(np.arange(n), np.diff(Ap))
    X[int(Ai[np.flatnonzero(Ai <= cols)[0]]), 64] = np.nan                        # a row of X that some term reads
    ref, wr, ar = _rule(n, Ap, Ai, Ax, k, X, B)
    R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), sym=True)
    assert np.isnan(omega[64]) and np.isnan(rnorm[64]) and np.isnan(wr[64])
    keep = np.arange(k) != 64
    assert omega[keep].tobytes() == wr[keep].tobytes() and rnorm[keep].tobytes() == ar[keep].tobytes()
    got = R.numpy()
    assert np.ascontiguousarray(got[:, keep]).tobytes() == np.ascontiguousarray(ref[:, keep]).tobytes()
    assert np.array_equal(np.isnan(got[:, 64]), np.isnan(ref[:, 64]))


@pytest.mark.parametrize("n", [0, 6])
def test_operators_without_rows_or_entries(cs, n):
    import _csx
    A = cs.cs_spalloc(n, n, 1, True, False)
    A.p = [0] * (n + 1)
    k = 3
    X, B = _blocks(n + 1, k, 9)
    B[:, 1] = 0.0
    R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), sym=True)
    assert (R.n, R.k) == (n, k) and R.numpy().tobytes() == B[:n].tobytes()
    if n == 0:
        assert omega.tolist() == [0.0] * k and rnorm.tolist() == [0.0] * k
    else:
        assert omega.tolist() == [1.0, 0.0, 1.0] and rnorm.tobytes() == np.max(np.abs(B[:n]), axis=0).tobytes()
    out = C.c_double(-1.0)
    with cs._Resident(A) as d:
        _csx.check(_csx.lib().csx_norm1_sym(d.handle, out))
    assert out.value == 0.0


def test_no_residual_and_in_place(cs):
    import _csx
    lib = _csx.lib()
    n, Ap, Ai, Ax = SHAPES["edges200"]()
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    for k in (3, 16, 66):
        X, B = _blocks(n, k, k)
        ref, wr, ar = _rule(n, Ap, Ai, Ax, k, X, B)
        dX, dB = cs.dvec(X), cs.dvec(B)
        omega, rnorm = np.empty(k), np.empty(k)
        _csx.check(lib.csx_residual_sym_block(A._dev.handle, dX.handle, dB.handle, 0, k, _csx.pd(omega), _csx.pd(rnorm)))
        assert omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
        assert dB.numpy().tobytes() == B.tobytes() and dX.numpy().tobytes() == X.tobytes()
        omega2 = np.empty(k)
        _csx.check(lib.csx_residual_sym_block(A._dev.handle, dX.handle, dB.handle, dB.handle, k, _csx.pd(omega2), None))
        assert dB.numpy().tobytes() == ref.tobytes() and omega2.tobytes() == wr.tobytes()
        _csx.check(lib.csx_residual_sym_block(A._dev.handle, dX.handle, dB.handle, 0, k, None, None))   # nothing asked


def test_c_abi_rejects_bad_arguments(cs):
    import _csx
    lib = _csx.lib()
    n, Ap, Ai, Ax = _random(40, 5)
    A = cs.cs_pin(_host_cs(cs, n, Ap, Ai, Ax))
    hA, k, E = A._dev.handle, 4, _csx.EINVAL
    X, B, R = cs.dvec(np.ones((n, k))), cs.dvec(np.zeros((n, k))), cs.dvec(n, k)
    w = np.empty(k + 1)

    def call(hX, hB, hR, kk=k, hM=hA):
        return lib.csx_residual_sym_block(hM, hX, hB, hR, kk, _csx.pd(w), None)

    assert call(X.handle, B.handle, R.handle) == _csx.OK
    for bad in (0, -1):
        assert call(X.handle, B.handle, R.handle, bad) == E
    assert call(X.handle, B.handle, R.handle, k + 1) == E                       # every block too short for k + 1
    Xs, Bs = cs.dvec(np.ones(n * k - 1)), cs.dvec(np.zeros(n * k - 1))
    assert call(Xs.handle, B.handle, R.handle) == E
    assert call(X.handle, Bs.handle, R.handle) == E
    assert call(X.handle, B.handle, Bs.handle) == E
    assert call(X.handle, B.handle, 0) == _csx.OK and call(X.handle, Bs.handle, 0) == E
    # R or B aliasing X
    assert call(X.handle, X.handle, 0) == E
    assert call(X.handle, B.handle, X.handle) == E
    assert call(X.handle, X.handle, R.handle) == E
    # wrapped views of one buffer: X over B, X over R, R over half of B; disjoint views pass
    big = cs.dvec(np.zeros(3 * n * k))
    vX, vB, vR = _view(cs, lib, big, 0, n * k), _view(cs, lib, big, n * k, n * k), _view(cs, lib, big, 2 * n * k, n * k)
    vB_over_X, vR_over_X = _view(cs, lib, big, n * k - 1, n * k), _view(cs, lib, big, 1, n * k)
    vR_over_B, vB_same = _view(cs, lib, big, n * k + (n * k) // 2, n * k), _view(cs, lib, big, n * k, n * k)
    assert call(vX, vB, vR) == _csx.OK
    assert call(vX, vB, vB_same) == _csx.OK                                   # the same range under another handle: in place
    assert call(vX, vB_over_X, vR) == E
    assert call(vX, vB, vR_over_X) == E
    assert call(vX, vB, vR_over_B) == E
    for h in (vX, vB, vR, vB_over_X, vR_over_X, vR_over_B, vB_same):
        _csx.free(h)
    # a pattern-only matrix, a handle that is no matrix, a matrix that is not square
    hP = _csx.new_handle()
    _csx.check(lib.csx_csc_upload(n, n, _csx.pi(Ap), _csx.pi(Ai), None, hP))
    assert call(X.handle, B.handle, R.handle, hM=hP) == E
    out = C.c_double(0.0)
    assert lib.csx_norm1_sym(hP, out) == E
    _csx.free(hP)
    assert call(X.handle, B.handle, R.handle, hM=X.handle) == E
    for m2, n2 in ((n + 1, n), (n, n - 1)):
        hN = _csx.new_handle()
        p2 = np.ascontiguousarray(Ap[:n2 + 1])
        _csx.check(lib.csx_csc_upload(m2, n2, _csx.pi(p2), _csx.pi(Ai), _csx.pd(Ax), hN))
        big_blocks = cs.dvec(np.ones(((n + 1), k)))
        assert call(big_blocks.handle, B.handle, 0, hM=hN) == E
        assert lib.csx_norm1_sym(hN, out) == E
        _csx.free(hN)
    assert lib.csx_norm1_sym(X.handle, out) == E


@pytest.mark.parametrize("shape", list(SHAPES) + ["grid"])
def test_norm1_sym_is_the_restatement(cs, shape):
    import _csx
    if shape == "grid":
        from chol_refactor_cases import with_dups_and_lower
        n, Ap, Ai, Ax = with_dups_and_lower(24, 14)
    else:
        n, Ap, Ai, Ax = SHAPES[shape]()
    stored = (n, np.asarray(Ap, np.int32), np.asarray(Ai, np.int32), np.asarray(Ax, np.float64))
    want = RSO.norm1(*stored)
    # (the restatement against the dense column sums of |entries|, which agree with it to rounding)
    dense = float(np.max(np.sum(SC.dense(stored[0], stored[1], stored[2], np.abs(stored[3])), axis=0)))
    assert abs(want - dense) <= 1e-13 * dense
    for other in (stored, SC.upper_only(*stored), SC.with_lower(*stored, 2, True)):
        out = C.c_double(-1.0)
        with cs._Resident(_host_cs(cs, *other)) as d:
            _csx.check(_csx.lib().csx_norm1_sym(d.handle, out))
        assert np.float64(out.value).tobytes() == np.float64(want).tobytes(), shape


def test_norm1_sym_over_many_blocks(cs):
    """70 000 rows: 274 blocks of 256 rows, so the partial maxima take two reduction passes; the largest row is the last one"""
    import _csx
    n = 70000
    Ap = np.arange(n + 1, dtype=np.int32)
    Ax = 1.0 + (np.arange(n) % 977) / 1000.0
    Ax[n - 1] = 5.0
    A = cs.cs_pin(_host_cs(cs, n, Ap, np.arange(n, dtype=np.int32), Ax))
    out = C.c_double(-1.0)
    _csx.check(_csx.lib().csx_norm1_sym(A._dev.handle, out))
    assert out.value == 5.0
    # a strictly lower entry is not counted, a strictly upper one counts in both rows
    small = (2, [0, 2, 3], [0, 1, 0], [1.0, 100.0, -3.0])
    with cs._Resident(_host_cs(cs, *small)) as d:
        _csx.check(_csx.lib().csx_norm1_sym(d.handle, out))
    assert out.value == 4.0 == RSO.norm1(*small)
    # and the residual of the same matrix: 1094 tiles, x = b / a gives r = 0 up to rounding, a huge b in the last row shows
    X, B = np.ones((n, 2)), np.stack([Ax, Ax], axis=1)
    B[n - 1, 1] = 1e30
    R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), sym=True)
    assert rnorm.tolist() == [0.0, 1e30 - 5.0] and omega[0] == 0.0 and omega[1] > 0.99


def test_residual_block_sym_and_its_arguments(cs):
    n, Ap, Ai, Ax = SHAPES["edges200"]()
    A = _host_cs(cs, n, Ap, Ai, Ax)                                              # not pinned: uploaded for the call
    X, B = _blocks(n, 7, 3)
    ref, wr, ar = _rule(n, Ap, Ai, Ax, 7, X, B)
    R, omega, rnorm = cs.residual_block(A, X, B, sym=True)
    assert R.numpy().tobytes() == ref.tobytes() and omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
    R, omega, rnorm = cs.residual_block(A, X, B, trans=True, sym=True)          # trans has no effect
    assert R.numpy().tobytes() == ref.tobytes() and omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
    none, omega, rnorm = cs.residual_block(A, X, B, residual=False, sym=True)
    assert none is None and omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
    ref1, w1, a1 = _rule(n, Ap, Ai, Ax, 1, X[:, 0], B[:, 0])
    R, omega, rnorm = cs.residual_block(A, X[:, 0].tolist(), B[:, 0].tolist(), sym=True)
    assert (R.n, R.k) == (n, 1) and R.numpy().tobytes() == ref1.tobytes() and omega.tobytes() == w1.tobytes()
    # blocks with more rows than the matrix needs: the rows beyond are not read
    Xl, Bl = np.vstack([X, np.full((2, 7), np.nan)]), np.vstack([B, np.full((3, 7), np.nan)])
    R, omega, rnorm = cs.residual_block(A, cs.dvec(Xl), cs.dvec(Bl), sym=True)
    assert (R.n, R.k) == (n, 7) and R.numpy().tobytes() == ref.tobytes() and omega.tobytes() == wr.tobytes()
    # the general call on the same matrix is another operator: other bytes
    G, wg, ag = cs.residual_block(A, X, B)
    assert G.numpy().tobytes() != ref.tobytes()
    # a matrix that is not square
    W = cs.cs_spalloc(n + 1, n, 1, True, False)
    W.p = [0] * (n + 1)
    assert cs.residual_block(W, np.ones((n + 1, 2)), np.ones((n + 1, 2)), sym=True) is False
    assert cs.residual_block(None, X, B, sym=True) is False and cs.residual_block(A, X, np.ones((n, 6)), sym=True) is False
