"""csx_residual_block / residual_block: R = B - op(A) X with the componentwise backward error of every column,
byte-equal to the host rule csx_residual_host (which tests/test_residual_cpu.py pins to the Python restatement) for column
counts on both sides of every template choice, at shapes around the 64-row tile and the U = 8 entries in flight, in both
directions; the placement of the maxima, R == 0 and R aliasing B, the argument checks, what each direction builds on the
matrix, and the two mask kernels of the refinement loop against numpy."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 66, 130)


def _random(m, n, seed, per_col=6):
    """unsorted columns with duplicates inside a column, explicit (signed) zeros, empty columns and empty rows"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 2 * per_col, n)
    counts[rng.choice(n, max(n // 8, 1), replace=False)] = 0
    live = rng.choice(m, max(1, (4 * m) // 5), replace=False)
    nnz = int(counts.sum())
    Ai = rng.choice(live, nnz)
    Ax = rng.standard_normal(nnz)
    Ax[rng.random(nnz) < 0.05] = 0.0
    Ax[rng.random(nnz) < 0.02] = -0.0
    Ap = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return m, n, Ap, Ai.astype(np.int32), Ax


def _row_lengths(seed, transpose):
    """rows of 0, 1, 7, 8 and 9 entries, ten of each (or columns, transposed): around the 8 entries in flight"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 7, 8, 9] * 10
    m, n = len(lens), 30
    r = np.repeat(np.arange(m), lens)
    c = np.concatenate([rng.choice(n, ln, replace=False) for ln in lens]).astype(np.int64)
    v = rng.standard_normal(len(r))
    if transpose:
        r, c, m, n = c, r, n, m
    order = np.lexsort((rng.random(len(r)), c))                 # by column, rows in random order inside one
    Ap = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.int32)
    return m, n, Ap, r[order].astype(np.int32), v[order]


SHAPES = {
    "1x1": lambda: (1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([-1.5])),
    "63x40": lambda: _random(63, 40, 1),
    "64x64": lambda: _random(64, 64, 2),
    "65x65": lambda: _random(65, 65, 3),
    "200x150": lambda: _random(200, 150, 4),
    "150x200": lambda: _random(150, 200, 5),
    "row_lengths": lambda: _row_lengths(6, False),
    "column_lengths": lambda: _row_lengths(7, True),
}


def _host_cs(cs, m, n, Ap, Ai, Ax):
    A = cs.cs_spalloc(m, n, max(len(Ai), 1), True, False)
    A.p, A.i, A.x = np.asarray(Ap).tolist(), np.asarray(Ai).tolist() or [0], np.asarray(Ax).tolist() or [0.0]
    return A


def _rule(m, n, Ap, Ai, Ax, k, trans, X, B):
    """the host rule: (R, omega, rnorm)"""
    import _csx
    rows = n if trans else m
    X, B = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    R, omega, rnorm = np.empty(rows * k), np.empty(k), np.empty(k)
    Ai, Ax = np.ascontiguousarray(Ai, np.int32), np.ascontiguousarray(Ax, np.float64)
    _csx.check(_csx.load().csx_residual_host(m, n, _csx.pi(Ap), _csx.pi(Ai), _csx.pd(Ax), k, 1 if trans else 0, _csx.pd(X),
                                             _csx.pd(B), _csx.pd(R), _csx.pd(omega), _csx.pd(rnorm)), "csx_residual_host")
    return R.reshape(rows, k), omega, rnorm


def _blocks(rows, cols, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((cols, k)) * 4.0, rng.standard_normal((rows, k))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_byte_equal_to_the_host_rule(cs, shape):
    m, n, Ap, Ai, Ax = SHAPES[shape]()
    A = cs.cs_pin(_host_cs(cs, m, n, Ap, Ai, Ax))
    for trans in (False, True):
        rows, cols = (n, m) if trans else (m, n)
        for k in KS:
            X, B = _blocks(rows, cols, k, 10 * k + trans)
            ref, wr, ar = _rule(m, n, Ap, Ai, Ax, k, trans, X, B)
            R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), trans=trans)
            assert (R.n, R.k) == (rows, k)
            assert R.numpy().tobytes() == ref.tobytes(), (shape, trans, k)
            assert omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes(), (shape, trans, k)
            assert rnorm.tobytes() == np.max(np.abs(ref), axis=0).tobytes()


@pytest.mark.parametrize("trans", [False, True])
def test_maximum_in_the_last_row_of_the_last_tile_and_the_last_column(cs, trans):
    """65 rows: the last tile holds row 64 alone.  A huge b there makes that row's |r| and its ratio (about 1, the
    bound of every ratio) the column's maxima; with it in the last column only, that column alone reports it."""
    m, n, Ap, Ai, Ax = SHAPES["65x65"]()
    A = cs.cs_pin(_host_cs(cs, m, n, Ap, Ai, Ax))
    for k in (1, 5, 64, 66, 130):
        X, B = _blocks(m, n, k, k)
        B[m - 1, k - 1] = 1e30
        ref, wr, ar = _rule(m, n, Ap, Ai, Ax, k, trans, X, B)
        R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), trans=trans)
        assert R.numpy().tobytes() == ref.tobytes()
        assert omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
        assert rnorm[k - 1] == abs(ref[m - 1, k - 1]) and rnorm[k - 1] > 1e29 and omega[k - 1] > 0.99
        assert (rnorm[:k - 1] < 1e29).all()


def test_hosts_blocks_lists_and_omega_alone(cs):
    m, n, Ap, Ai, Ax = SHAPES["200x150"]()
    A = _host_cs(cs, m, n, Ap, Ai, Ax)                          # not pinned: uploaded for the call
    X, B = _blocks(m, n, 7, 3)
    ref, wr, ar = _rule(m, n, Ap, Ai, Ax, 7, False, X, B)
    R, omega, rnorm = cs.residual_block(A, X, B)
    assert R.numpy().tobytes() == ref.tobytes() and omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
    assert X.shape == (n, 7) and B.shape == (m, 7)
    none, omega, rnorm = cs.residual_block(A, X, B, residual=False)
    assert none is None and omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
    ref1, w1, a1 = _rule(m, n, Ap, Ai, Ax, 1, True, B[:, 0], X[:, 0])
    R, omega, rnorm = cs.residual_block(A, B[:, 0].tolist(), X[:, 0].tolist(), trans=True)
    assert (R.n, R.k) == (n, 1) and R.numpy().tobytes() == ref1.tobytes() and omega.tobytes() == w1.tobytes()
    # blocks with more rows than the matrix needs: the rows beyond are not read
    Xl, Bl = np.vstack([X, np.full((2, 7), np.nan)]), np.vstack([B, np.full((3, 7), np.nan)])
    R, omega, rnorm = cs.residual_block(A, cs.dvec(Xl), cs.dvec(Bl))
    assert (R.n, R.k) == (m, 7) and R.numpy().tobytes() == ref.tobytes() and omega.tobytes() == wr.tobytes()


@pytest.mark.parametrize("trans", [False, True])
def test_a_nan_stays_in_its_column(cs, trans):
    m, n, Ap, Ai, Ax = SHAPES["65x65"]()
    A = cs.cs_pin(_host_cs(cs, m, n, Ap, Ai, Ax))
    k = 66
    X, B = _blocks(m, n, k, 5)
    col = int(np.flatnonzero(np.diff(Ap) > 0)[0]) if not trans else int(Ai[0])     # a row of X that some term reads
    X[col, 64] = np.nan
    ref, wr, ar = _rule(m, n, Ap, Ai, Ax, k, trans, X, B)
    R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), trans=trans)
    assert np.isnan(omega[64]) and np.isnan(rnorm[64]) and np.isnan(wr[64])
    keep = np.arange(k) != 64
    assert omega[keep].tobytes() == wr[keep].tobytes() and rnorm[keep].tobytes() == ar[keep].tobytes()
    got = R.numpy()
    assert np.ascontiguousarray(got[:, keep]).tobytes() == np.ascontiguousarray(ref[:, keep]).tobytes()
    assert np.array_equal(np.isnan(got[:, 64]), np.isnan(ref[:, 64]))


@pytest.mark.parametrize("shape", [(0, 5), (6, 0), (6, 5)])
@pytest.mark.parametrize("trans", [False, True])
def test_operators_without_rows_or_entries(cs, shape, trans):
    m, n = shape
    A = cs.cs_spalloc(m, n, 1, True, False)
    A.p = [0] * (n + 1)
    rows, cols = (n, m) if trans else (m, n)
    k = 3
    X, B = _blocks(rows + 1, cols + 1, k, 9)
    B[:, 1] = 0.0
    R, omega, rnorm = cs.residual_block(A, cs.dvec(X), cs.dvec(B), trans=trans)
    assert (R.n, R.k) == (rows, k) and R.numpy().tobytes() == B[:rows].tobytes()
    if rows == 0:
        assert omega.tolist() == [0.0] * k and rnorm.tolist() == [0.0] * k
    else:
        assert omega.tolist() == [1.0, 0.0, 1.0] and rnorm.tobytes() == np.max(np.abs(B[:rows]), axis=0).tobytes()
    ref, wr, ar = _rule(m, n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0), k, trans, X, B[:rows])
    assert omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()


def test_no_residual_and_in_place(cs):
    import _csx
    lib = _csx.lib()
    m, n, Ap, Ai, Ax = SHAPES["200x150"]()
    A = cs.cs_pin(_host_cs(cs, m, n, Ap, Ai, Ax))
    for trans in (0, 1):
        rows, cols = (n, m) if trans else (m, n)
        for k in (3, 16, 66):
            X, B = _blocks(rows, cols, k, k)
            ref, wr, ar = _rule(m, n, Ap, Ai, Ax, k, trans, X, B)
            dX, dB = cs.dvec(X), cs.dvec(B)
            omega, rnorm = np.empty(k), np.empty(k)
            _csx.check(lib.csx_residual_block(A._dev.handle, dX.handle, dB.handle, 0, k, trans, _csx.pd(omega), _csx.pd(rnorm)))
            assert omega.tobytes() == wr.tobytes() and rnorm.tobytes() == ar.tobytes()
            assert dB.numpy().tobytes() == B.tobytes() and dX.numpy().tobytes() == X.tobytes()
            omega2 = np.empty(k)
            _csx.check(lib.csx_residual_block(A._dev.handle, dX.handle, dB.handle, dB.handle, k, trans, _csx.pd(omega2), None))
            assert dB.numpy().tobytes() == ref.tobytes() and omega2.tobytes() == wr.tobytes()
            _csx.check(lib.csx_residual_block(A._dev.handle, dX.handle, dB.handle, 0, k, trans, None, None))   # nothing asked


def test_c_abi_rejects_bad_arguments(cs):
    import _csx
    lib = _csx.lib()
    m, n, Ap, Ai, Ax = _random(40, 30, 5)
    A = cs.cs_pin(_host_cs(cs, m, n, Ap, Ai, Ax))
    hA, k, E = A._dev.handle, 4, _csx.EINVAL
    X, B, R = cs.dvec(np.ones((n, k))), cs.dvec(np.zeros((m, k))), cs.dvec(m, k)
    w = np.empty(k + 1)

    def call(hX, hB, hR, kk=k, trans=0, hM=hA):
        return lib.csx_residual_block(hM, hX, hB, hR, kk, trans, _csx.pd(w), None)

    assert call(X.handle, B.handle, R.handle) == _csx.OK
    for bad in (0, -1):
        assert call(X.handle, B.handle, R.handle, bad) == E
    assert call(X.handle, B.handle, R.handle, k + 1) == E                       # every block too short for k + 1
    Xs, Bs = cs.dvec(np.ones(n * k - 1)), cs.dvec(np.zeros(m * k - 1))
    assert call(Xs.handle, B.handle, R.handle) == E
    assert call(X.handle, Bs.handle, R.handle) == E
    assert call(X.handle, B.handle, Bs.handle) == E
    assert call(X.handle, B.handle, 0) == _csx.OK and call(X.handle, Bs.handle, 0) == E
    # transposed: X needs m k, B and R n k entries
    assert call(B.handle, X.handle, 0, k, 1) == _csx.OK
    assert call(X.handle, B.handle, 0, k, 1) == E
    # R or B aliasing X
    Q = cs.dvec(np.ones((max(m, n), k)))
    assert call(Q.handle, Q.handle, 0) == E
    assert call(Q.handle, B.handle, Q.handle) == E
    assert call(X.handle, X.handle, R.handle) == E
    # wrapped views of one buffer: X over B, X over R, R over half of B; disjoint views pass
    big = cs.dvec(np.zeros((n + 2 * m) * k))
    base = big.device_ptr()

    def view(offset, count):
        h = _csx.new_handle()
        _csx.check(lib.csx_vec_wrap(C.c_void_p(base + 8 * offset), count, h))
        return h

    vX, vB, vR = view(0, n * k), view(n * k, m * k), view((n + m) * k, m * k)
    vB_over_X, vR_over_X, vR_over_B = view(n * k - 1, m * k), view(1, m * k), view(n * k + (m * k) // 2, m * k)
    vB_same = view(n * k, m * k)
    assert call(vX, vB, vR) == _csx.OK
    assert call(vX, vB, vB_same) == _csx.OK                                   # the same range under another handle: in place
    assert call(vX, vB_over_X, vR) == E
    assert call(vX, vB, vR_over_X) == E
    assert call(vX, vB, vR_over_B) == E
    for h in (vX, vB, vR, vB_over_X, vR_over_X, vR_over_B, vB_same):
        _csx.free(h)
    # a pattern-only matrix, a handle that is no matrix
    hP = _csx.new_handle()
    _csx.check(lib.csx_csc_upload(m, n, _csx.pi(Ap), _csx.pi(Ai), None, hP))
    assert call(X.handle, B.handle, R.handle, hM=hP) == E
    _csx.free(hP)
    assert call(X.handle, B.handle, R.handle, hM=X.handle) == E
    # the mask kernels
    mask = _csx.i32(np.ones(k))
    assert lib.csx_block_add_cols(X.handle, X.handle, Q.handle, n, k, _csx.pi(mask)) == _csx.OK
    assert lib.csx_block_add_cols(X.handle, X.handle, Q.handle, n, 0, _csx.pi(mask)) == E
    assert lib.csx_block_add_cols(X.handle, X.handle, Q.handle, n + 1, k, _csx.pi(mask)) == E
    assert lib.csx_block_add_cols(X.handle, X.handle, Q.handle, n, k, None) == E
    assert lib.csx_block_select_cols(X.handle, Q.handle, n, k, _csx.pi(mask)) == _csx.OK
    assert lib.csx_block_select_cols(X.handle, X.handle, n, k, _csx.pi(mask)) == E
    assert lib.csx_block_select_cols(X.handle, Q.handle, n + 1, k, _csx.pi(mask)) == E
    assert lib.csx_block_select_cols(X.handle, Q.handle, -1, k, _csx.pi(mask)) == E


def test_mask_kernels_refuse_shifted_views_of_one_buffer(cs):
    """out as a csx_vec_wrap view one double into X or D, dst one double into src: CSX_EINVAL and nothing written; the
    same views laid end to end pass"""
    import _csx
    lib = _csx.lib()
    rows, k = 8, 4
    total = rows * k
    big = cs.dvec(np.full(3 * total, 7.0))
    views = []

    def view(offset):
        views.append(_csx.new_handle())
        _csx.check(lib.csx_vec_wrap(C.c_void_p(big.device_ptr() + 8 * offset), total, views[-1]))
        return views[-1]

    X, D, out, out_in_X, out_in_D = view(0), view(total), view(2 * total), view(1), view(total + 1)
    pm = _csx.pi(_csx.i32(np.ones(k)))
    try:
        assert lib.csx_block_add_cols(X, D, out_in_X, rows, k, pm) == _csx.EINVAL
        assert lib.csx_block_add_cols(X, D, out_in_D, rows, k, pm) == _csx.EINVAL
        assert lib.csx_block_select_cols(X, out_in_X, rows, k, pm) == _csx.EINVAL
        assert (big.numpy() == 7.0).all()
        assert lib.csx_block_add_cols(X, D, out, rows, k, pm) == _csx.OK
        assert lib.csx_block_select_cols(X, D, rows, k, pm) == _csx.OK
    finally:
        for h in views:
            _csx.free(h)


def test_the_transposed_direction_builds_no_plan(cs):
    import _csx
    lib = _csx.lib()
    m, n, Ap, Ai, Ax = SHAPES["200x150"]()
    A = cs.cs_pin(_host_cs(cs, m, n, Ap, Ai, Ax))

    def has_rows():
        r, t = C.c_int(-1), C.c_int(-1)
        _csx.check(lib.csx_gaxpy_plan_info(A._dev.handle, r, t, None))
        return r.value, t.value

    assert has_rows() == (0, 0)
    X, B = _blocks(n, m, 8, 1)
    assert cs.residual_block(A, cs.dvec(X), cs.dvec(B), trans=True) is not False
    assert has_rows() == (0, 0)
    assert cs.residual_block(A, cs.dvec(B), cs.dvec(X)) is not False
    assert has_rows() == (1, 0)


@pytest.mark.parametrize("k", [5, 66])
def test_mask_kernels_against_numpy(cs, k):
    import _csx
    lib = _csx.lib()
    rows = 37
    rng = np.random.default_rng(k)
    X, D, old = rng.standard_normal((rows + 1, k)), rng.standard_normal((rows + 1, k)) * 1e-3, rng.standard_normal((rows + 1, k))
    for mask in (np.zeros(k, np.int32), np.ones(k, np.int32), (np.arange(k) % 2).astype(np.int32),
                 (np.arange(k) % 2 == 0).astype(np.int32) * 7):
        on = mask != 0
        dX, dD, out = cs.dvec(X), cs.dvec(D), cs.dvec(old)
        _csx.check(lib.csx_block_add_cols(dX.handle, dD.handle, out.handle, rows, k, _csx.pi(mask)))
        want = np.where(on[None, :], X + D, X)
        want[rows] = old[rows]                                                   # the row past `rows` is not written
        assert out.numpy().tobytes() == want.tobytes()
        assert dX.numpy().tobytes() == X.tobytes() and dD.numpy().tobytes() == D.tobytes()
        _csx.check(lib.csx_block_add_cols(dX.handle, dD.handle, dX.handle, rows, k, _csx.pi(mask)))   # out is X
        assert dX.numpy().tobytes() == np.vstack([want[:rows], X[rows:]]).tobytes()
        dst = cs.dvec(old)
        _csx.check(lib.csx_block_select_cols(dD.handle, dst.handle, rows, k, _csx.pi(mask)))
        want = np.where(on[None, :], D, old)
        want[rows] = old[rows]
        assert dst.numpy().tobytes() == want.tobytes()
