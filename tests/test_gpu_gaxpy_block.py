"""gaxpy_block / csx_gaxpy_block: Y += A X for a block of right-hand sides in one call.

EXACT: every column of Y byte-equal to the plain-C cs_gaxpy on that column, twice over; AUTO within tol.componentwise of
it against the sum of |terms|.  Then edge cases and errors, the interplay with csx_gaxpy's cached plans, and the residual of
a batched Cholesky solve, at an oracle-feasible size and at config 5's full size."""
import ctypes as C

import numpy as np
import pytest

import c_oracle as CO
import synth
import tol
from conftest import golden, unpack
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 64, 65, 70, 128, 130)   # both sides of every cut of the launch table
GOLDEN = ("t1", "west0067", "bcsstk01", "bcsstk16", "ash219", "lp_afiro")


def _arrays(A):
    nnz = A.p[A.n]
    return (np.asarray(A.p, dtype=np.int32), np.asarray(A.i[:nnz], dtype=np.int32),
            np.asarray(A.x[:nnz], dtype=np.float64))


def _host(cs, m, n, Ap, Ai, Ax):
    A = cs.cs_spalloc(m, n, max(len(Ai), 1), True, False)
    A.p, A.i, A.x = np.asarray(Ap).tolist(), np.asarray(Ai).tolist(), np.asarray(Ax).tolist()
    return A


def _random(m, n, seed):
    """Rectangular, unsorted columns with duplicate entries, explicit (signed) zeros, empty columns, about a fifth of
    the rows empty, and one row far longer than the rest."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 12, n)
    counts[rng.choice(n, n // 8, replace=False)] = 0
    live = rng.choice(m, max(1, (4 * m) // 5), replace=False)
    nnz = int(counts.sum())
    Ai = rng.choice(live, nnz)
    Ai[rng.random(nnz) < 0.25] = live[0]                       # the long row
    Ax = rng.standard_normal(nnz)
    Ax[rng.random(nnz) < 0.05] = 0.0
    Ax[rng.random(nnz) < 0.02] = -0.0
    Ap = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return m, n, Ap, Ai.astype(np.int32), Ax


def _matrices(cs):
    for name in GOLDEN:
        A = unpack(cs, golden(name), "C")
        yield name, A
    for m, n, seed in ((300, 200, 1), (50, 700, 2), (1000, 40, 3)):
        mm, nn, Ap, Ai, Ax = _random(m, n, seed)
        yield "rand%dx%d" % (m, n), _host(cs, mm, nn, Ap, Ai, Ax)


def _inputs(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, k)) * 4.0, rng.standard_normal((m, k))


def _reference(A, X, Y0):
    Ap, Ai, Ax = _arrays(A)
    return [CO.gaxpy(A.m, A.n, Ap, Ai, Ax, np.ascontiguousarray(X[:, r]), np.ascontiguousarray(Y0[:, r]))
            for r in range(X.shape[1])]


def _terms(A, X, Y0):
    Ap, Ai, Ax = _arrays(A)
    return [CO.gaxpy(A.m, A.n, Ap, Ai, np.abs(Ax), np.abs(X[:, r]), np.abs(Y0[:, r])) for r in range(X.shape[1])]


def _run(cs, A, X, Y0, mode):
    dY = cs.dvec(Y0)
    assert cs.gaxpy_block(A, cs.dvec(X), dY, mode) is True
    return dY.numpy().reshape(Y0.shape)


@pytest.mark.parametrize("which", list(GOLDEN) + ["rand300x200", "rand50x700", "rand1000x40"])
def test_exact_every_column_byte_equal_to_the_reference(cs, which):
    name, A = next((nm, M) for nm, M in _matrices(cs) if nm == which)
    cs.cs_pin(A)
    for k in KS:
        X, Y0 = _inputs(A.m, A.n, k, k)
        ref = _reference(A, X, Y0)
        got = _run(cs, A, X, Y0, cs.GAXPY_EXACT)
        for r in range(k):
            assert got[:, r].tobytes() == ref[r].tobytes(), (name, k, r)
        again = _run(cs, A, X, Y0, cs.GAXPY_EXACT)
        assert again.tobytes() == got.tobytes(), (name, k)
        Yh = Y0.copy()                                         # host blocks: exact by default, written back
        assert cs.gaxpy_block(A, X, Yh) is True
        assert Yh.tobytes() == got.tobytes(), (name, k)


@pytest.mark.parametrize("which", list(GOLDEN) + ["rand300x200", "rand50x700", "rand1000x40"])
def test_auto_within_rounding_and_k1_is_cs_gaxpy(cs, which):
    name, A = next((nm, M) for nm, M in _matrices(cs) if nm == which)
    cs.cs_pin(A)
    for k in KS:
        X, Y0 = _inputs(A.m, A.n, k, 100 + k)
        ref, terms = _reference(A, X, Y0), _terms(A, X, Y0)
        dY = cs.dvec(Y0)
        assert cs.gaxpy_block(A, cs.dvec(X), dY) is True           # dvec blocks: AUTO by default
        got = dY.numpy().reshape(Y0.shape)
        for r in range(k):
            assert tol.componentwise(got[:, r], ref[r], terms[r]) <= 1e-10, (name, k, r)
        if k == 1:
            dy = cs.dvec(Y0[:, 0])
            assert cs.cs_gaxpy(A, cs.dvec(X[:, 0]), dy, cs.GAXPY_AUTO) is True
            assert got[:, 0].tobytes() == dy.numpy().tobytes()
            y1 = Y0[:, 0].copy()                                       # 1-D host vectors: cs_gaxpy's answer
            assert cs.gaxpy_block(A, X[:, 0].copy(), y1) is True
            assert y1.tobytes() == ref[0].tobytes()


def test_column_route_gives_cs_gaxpy_per_column(cs):
    """The column route (forced by option; AUTO's rule takes it only for matrices with a tiled plan): every column
    byte-equal to cs_gaxpy AUTO on it.  Then a matrix that holds a tiled plan: AUTO takes the route by itself for
    k <= 4, within rounding (the tiled plan sums in LDS with atomics)."""
    import _csx
    m, n, Ap, Ai, Ax = _random(3000, 2000, 7)
    A = cs.cs_pin(_host(cs, m, n, Ap, Ai, Ax))
    for k in (2, 8, 33, 130):
        X, Y0 = _inputs(m, n, k, k)
        with _csx.option("gaxpy.block_route", 2):
            got = _run(cs, A, X, Y0, cs.GAXPY_AUTO)
        for r in range(k):
            dy = cs.dvec(Y0[:, r])
            assert cs.cs_gaxpy(A, cs.dvec(np.ascontiguousarray(X[:, r])), dy, cs.GAXPY_AUTO) is True
            assert got[:, r].tobytes() == dy.numpy().tobytes(), (k, r)
        with _csx.option("gaxpy.block_route", 1):                       # the block kernel: EXACT's bits
            assert _run(cs, A, X, Y0, cs.GAXPY_AUTO).tobytes() == _run(cs, A, X, Y0, cs.GAXPY_EXACT).tobytes()
    n2, per_col = 20000, 16
    Gp, Gi, Gx = synth.grand(n2, per_col, 11)
    G = cs.cs_pin(_host(cs, n2, n2, Gp, Gi, Gx))
    assert cs.cs_gaxpy_prepare(G, cs.GAXPY_TILED)
    for k in (2, 4):
        X, Y0 = _inputs(n2, n2, k, 50 + k)
        got = _run(cs, G, X, Y0, cs.GAXPY_AUTO)
        ref, terms = _reference(G, X, Y0), _terms(G, X, Y0)
        for r in range(k):
            assert tol.componentwise(got[:, r], ref[r], terms[r]) <= 1e-10, (k, r)


@pytest.mark.parametrize("mode", ["EXACT", "AUTO"])
@pytest.mark.parametrize("shape", [(0, 5), (6, 0), (6, 5)])
def test_empty_matrices_are_no_ops(cs, mode, shape):
    m, n = shape
    A = cs.cs_spalloc(m, n, 1, True, False)
    A.p = [0] * (n + 1)
    k = 3
    X, Y0 = _inputs(m + 2, n + 2, k, 9)                     # two rows more than A needs: must stay untouched
    dX, dY = cs.dvec(X), cs.dvec(Y0)
    assert cs.gaxpy_block(A, dX, dY, getattr(cs, "GAXPY_" + mode)) is True
    assert dY.numpy().tobytes() == Y0.tobytes()
    assert dX.numpy().tobytes() == X.tobytes()


def test_python_errors(cs):
    A = _host(cs, 3, 2, [0, 2, 3], [0, 2, 1], [1.0, -2.0, 3.0])
    P = cs.cs_spalloc(3, 2, 3, False, False)
    P.p, P.i = [0, 2, 3], [0, 2, 1]
    with pytest.raises(TypeError):
        cs.gaxpy_block(P, np.ones((2, 4)), np.zeros((3, 4)))
    assert cs.gaxpy_block(A, cs.dvec(np.ones((2, 4))), cs.dvec(np.zeros((3, 5)))) is False
    assert cs.gaxpy_block(A, np.ones((2, 4)), np.zeros((3, 5))) is False
    assert cs.gaxpy_block(A, np.ones(2), np.zeros((3, 2))) is False
    with pytest.raises(IndexError):
        cs.gaxpy_block(A, cs.dvec(np.ones((1, 4))), cs.dvec(np.zeros((3, 4))))
    with pytest.raises(IndexError):
        cs.gaxpy_block(A, np.ones((2, 4)), np.zeros((2, 4)))
    Y = np.zeros((3, 4))
    assert cs.gaxpy_block(A, np.ones((2, 4)), Y) is True
    assert Y.tolist() == [[1.0] * 4, [3.0] * 4, [-2.0] * 4]


def test_c_abi_rejects_bad_arguments(cs):
    import _csx
    lib = _csx.lib()
    m, n, Ap, Ai, Ax = _random(40, 30, 5)
    A = cs.cs_pin(_host(cs, m, n, Ap, Ai, Ax))
    hA, k = A._dev.handle, 4
    X, Y = cs.dvec(np.ones((n, k))), cs.dvec(np.zeros((m, k)))
    E, EX, AU = _csx.EINVAL, cs.GAXPY_EXACT, cs.GAXPY_AUTO
    assert lib.csx_gaxpy_block(hA, X.handle, Y.handle, k, EX) == _csx.OK
    assert lib.csx_gaxpy_block(hA, Y.handle, Y.handle, k, EX) == E           # X == Y
    for bad in (0, -1):
        assert lib.csx_gaxpy_block(hA, X.handle, Y.handle, bad, AU) == E
    for mode in (cs.GAXPY_WAVE, cs.GAXPY_TILED, cs.GAXPY_ATOMIC, 5, -1):
        assert lib.csx_gaxpy_block(hA, X.handle, Y.handle, k, mode) == E
        assert lib.csx_gaxpy_block(hA, X.handle, Y.handle, 1, mode) == E
    assert lib.csx_gaxpy_block(hA, X.handle, Y.handle, k + 1, EX) == E       # both blocks too short for k + 1
    Xs, Ys = cs.dvec(np.ones(n * k - 1)), cs.dvec(np.zeros(m * k - 1))
    assert lib.csx_gaxpy_block(hA, Xs.handle, Y.handle, k, EX) == E
    assert lib.csx_gaxpy_block(hA, X.handle, Ys.handle, k, EX) == E
    # two wrapped views of one buffer that overlap, and two that do not
    big = cs.dvec(np.zeros((n + m) * k))
    base = big.device_ptr()
    hX1, hY1, hY2 = _csx.new_handle(), _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_vec_wrap(C.c_void_p(base), n * k, hX1))
    _csx.check(lib.csx_vec_wrap(C.c_void_p(base + 8 * (n * k - 1)), m * k, hY1))
    _csx.check(lib.csx_vec_wrap(C.c_void_p(base + 8 * n * k), m * k, hY2))
    assert lib.csx_gaxpy_block(hA, hX1, hY1, k, EX) == E
    assert lib.csx_gaxpy_block(hA, hX1, hY2, k, EX) == _csx.OK
    for h in (hX1, hY1, hY2):
        _csx.free(h)
    # a pattern-only matrix
    hP = _csx.new_handle()
    _csx.check(lib.csx_csc_upload(m, n, _csx.pi(Ap), _csx.pi(Ai), None, hP))
    assert lib.csx_gaxpy_block(hP, X.handle, Y.handle, k, EX) == E
    _csx.free(hP)


def test_unaligned_wide_blocks_exact(cs):
    """Blocks whose rows are not 16-byte aligned (an even k on a wrapped pointer 8 bytes into a buffer) take the
    one-column-per-lane form: still every column byte-equal to the reference."""
    import _csx
    lib = _csx.lib()
    m, n, Ap, Ai, Ax = _random(300, 200, 1)
    A = cs.cs_pin(_host(cs, m, n, Ap, Ai, Ax))
    k = 128
    X, Y0 = _inputs(m, n, k, 77)
    bx, by = cs.dvec(np.concatenate([[0.0], X.reshape(-1)])), cs.dvec(np.concatenate([[0.0], Y0.reshape(-1)]))
    hX, hY = _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_vec_wrap(C.c_void_p(bx.device_ptr() + 8), n * k, hX))
    _csx.check(lib.csx_vec_wrap(C.c_void_p(by.device_ptr() + 8), m * k, hY))
    _csx.check(lib.csx_gaxpy_block(A._dev.handle, hX, hY, k, cs.GAXPY_EXACT))
    got = by.numpy()[1:].reshape(m, k)
    ref = _reference(A, X, Y0)
    for r in range(k):
        assert got[:, r].tobytes() == ref[r].tobytes(), r
    for h in (hX, hY):
        _csx.free(h)


def test_plan_interplay_and_invalidate(cs):
    m, n, Ap, Ai, Ax = _random(1000, 40, 3)
    x = np.random.default_rng(1).standard_normal(n)
    y0 = np.random.default_rng(2).standard_normal(m)
    X, Y0 = _inputs(m, n, 8, 3)

    def single(A, mode):
        dy = cs.dvec(y0)
        assert cs.cs_gaxpy(A, cs.dvec(x), dy, mode) is True
        return dy.numpy().tobytes()

    for mode in (cs.GAXPY_AUTO, cs.GAXPY_EXACT):
        alone = single(cs.cs_pin(_host(cs, m, n, Ap, Ai, Ax)), mode)
        A = cs.cs_pin(_host(cs, m, n, Ap, Ai, Ax))
        assert single(A, mode) == alone
        _run(cs, A, X, Y0, cs.GAXPY_AUTO)
        _run(cs, A, X, Y0, cs.GAXPY_EXACT)
        assert single(A, mode) == alone
        B = cs.cs_pin(_host(cs, m, n, Ap, Ai, Ax))              # block call first on a fresh matrix
        _run(cs, B, X, Y0, mode)
        assert single(B, mode) == alone
    # edited values of a pinned matrix: after cs_invalidate the block call sees them
    A = cs.cs_pin(_host(cs, m, n, Ap, Ai, Ax))
    first = _run(cs, A, X, Y0, cs.GAXPY_EXACT)
    Ax2 = Ax * 1.5 - 0.25
    A.x[:len(Ax2)] = Ax2.tolist()
    cs.cs_invalidate(A)
    got = _run(cs, A, X, Y0, cs.GAXPY_EXACT)
    assert got.tobytes() != first.tobytes()
    for r in range(8):
        assert got[:, r].tobytes() == CO.gaxpy(m, n, Ap, Ai, Ax2, X[:, r].copy(), Y0[:, r].copy()).tobytes(), r


def test_residual_of_a_cholsol_batch(cs):
    """cholsol_factor(A).solve on a k = 70 dvec batch, then A X - B as gaxpy_block(A, X, -B) on the device:
    every column byte-equal to the plain-C cs_gaxpy of the downloaded X, and small."""
    nb, bs, k = 2000, 24, 70
    Ap, Ai, Ax = synth.gspd(nb, bs, 31)
    n = nb * bs
    A = cs.cs_pin(_host(cs, n, n, Ap, Ai, Ax))
    B = synth.rhs(n, k)
    F = cs.cholsol_factor(A)
    dX = cs.dvec(B)
    assert F.solve(dX) is True
    X = dX.numpy().reshape(n, k)
    dR = cs.dvec(-B)
    assert cs.gaxpy_block(A, dX, dR, cs.GAXPY_EXACT) is True
    R = dR.numpy().reshape(n, k)
    for r in range(k):
        ref = CO.gaxpy(n, n, Ap, Ai, Ax, np.ascontiguousarray(X[:, r]), -B[:, r])
        assert R[:, r].tobytes() == ref.tobytes(), r
    assert np.max(np.abs(R)) < 1e-12 * np.max(np.abs(B)) * bs
    dA = cs.dvec(-B)
    assert cs.gaxpy_block(A, dX, dA) is True                    # AUTO: within rounding
    terms = [CO.gaxpy(n, n, Ap, Ai, np.abs(Ax), np.abs(X[:, r]), np.abs(B[:, r])) for r in (0, 35, 69)]
    Ra = dA.numpy().reshape(n, k)
    for t, r in zip(terms, (0, 35, 69)):
        assert tol.componentwise(Ra[:, r], R[:, r], t) <= 1e-10, r


def test_residual_of_a_cholsol_batch_at_config5_size(cs):
    """Config 5 at full size (G-spd, 78 125 blocks of 64, n = 5M), k = 128: the solve, then A X on the device in one
    call; four columns byte-equal to single-vector csx_gaxpy EXACT on the device, and the residual small."""
    import _csx
    lib = _csx.lib()
    nb, bs, k = 78125, 64, 128
    n = nb * bs
    hA = _csx.new_handle()
    _csx.check(lib.csx_gen_gspd(nb, bs, 20240606, hA))
    A = cs._from_device(hA, lambda nnz: max(nnz, 1))
    hB = _csx.new_handle()
    _csx.check(lib.csx_gen_rhs(n, k, 0, hB))
    dX = cs.dvec(n, k, _handle=hB)
    F = cs.cholsol_factor(A)
    assert F.solve(dX) is True
    dZ = cs.dvec(n, k)
    assert cs.gaxpy_block(A, dX, dZ, cs.GAXPY_EXACT) is True
    X = dX.numpy()
    Z = dZ.numpy()
    for r in (0, 1, 64, 127):
        dx, dz = cs.dvec(np.ascontiguousarray(X[:, r])), cs.dvec(n)
        _csx.check(lib.csx_gaxpy(hA, dx.handle, dz.handle, cs.GAXPY_EXACT))
        assert Z[:, r].tobytes() == dz.numpy().tobytes(), r
        b = synth.rhs(n, 1, r)[:, 0]
        assert np.max(np.abs(Z[:, r] - b)) < 1e-12 * np.max(np.abs(b)) * bs, r
