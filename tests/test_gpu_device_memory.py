"""Device memory of the library comes back: after every plan kind has been built, used and freed, and after calls that
fail on bad input, the bytes the pool has handed out (csx_mem_info's live bytes) are what they were before.  Through the
C ABI, so that nothing but the library holds device memory in between."""
import ctypes as C
import gc

import numpy as np
import pytest
import scipy.sparse as sp

from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu


def _lib():
    import _csx
    return _csx, _csx.lib()


def _live():
    X, lib = _lib()
    X.check(lib.csx_sync(), "sync")
    cached, live, free = C.c_int64(), C.c_int64(), C.c_int64()
    X.check(lib.csx_mem_info(cached, live, free), "mem_info")
    return live.value


def _csc(S):
    X, lib = _lib()
    S = sp.csc_matrix(S)
    S.sort_indices()
    h = X.new_handle()
    x = S.data if S.nnz else np.zeros(1)
    X.check(lib.csx_csc_upload(S.shape[0], S.shape[1], X.pi(X.i32(S.indptr)), X.pi(X.i32(S.indices if S.nnz else [0])),
                               X.pd(X.f64(x)), h), "csc_upload")
    return h


def _vec(a):
    X, lib = _lib()
    a = X.f64(np.ravel(a))
    h = X.new_handle()
    X.check(lib.csx_vec_upload(X.pd(a), a.size, h), "vec_upload")
    return h


def _ivec(a):
    X, lib = _lib()
    a = X.i32(np.ravel(a))
    h = X.new_handle()
    X.check(lib.csx_ivec_upload(X.pi(a), a.size, h), "ivec_upload")
    return h


def _spd_blocks(nb, bs, seed=0, negative_block=None):
    rng = np.random.default_rng(seed)
    blocks = []
    for k in range(nb):
        M = rng.uniform(-1, 1, (bs, bs))
        B = M @ M.T + bs * np.eye(bs)
        blocks.append(-B if k == negative_block else B)
    return sp.block_diag(blocks, format="csc")


def _spd_band(n, half):
    return sp.diags([np.full(n - abs(k), -1.0 if k else 2.0 * half + 1.0) for k in range(-half, half + 1)],
                    list(range(-half, half + 1)), format="csc")


def _lu_blocks(nb, bs, seed=1, singular_block=None):
    rng = np.random.default_rng(seed)
    blocks = []
    for k in range(nb):
        B = np.ones((bs, bs)) if k == singular_block else rng.uniform(-1, 1, (bs, bs)) + bs * np.eye(bs)
        blocks.append(B)
    return sp.block_diag(blocks, format="csc")


def _symbolic(hA, n):
    X, lib = _lib()
    parent, cp = np.empty(n, np.int32), np.empty(n + 1, np.int32)
    X.check(lib.csx_schol(hA, X.pi(parent), X.pi(cp)), "schol")
    return parent, cp


def _chol(hA, n, forget_finding=False):
    """csx_schol + csx_chol; forget_finding: csx_chol without csx_schol's finding cached on A (finds it again itself)"""
    X, lib = _lib()
    parent, cp = _symbolic(hA, n)
    if forget_finding:
        X.check(lib.csx_csc_invalidate(hA), "csc_invalidate")
    hL = X.new_handle()
    X.check(lib.csx_chol(hA, X.pi(parent), X.pi(cp), None, hL), "chol")
    return hL


@pytest.fixture
def steady_live(cs):
    """live bytes before the test body and a check that they are the same after it; no Python finaliser frees a handle
    of another test in between"""
    gc.collect()
    gc.disable()
    try:
        before = _live()
        yield
        assert _live() == before
    finally:
        gc.enable()


def test_every_plan_kind_gives_its_memory_back(steady_live):
    X, lib = _lib()
    handles = []

    def keep(h):
        handles.append(h)
        return h

    rng = np.random.default_rng(3)
    # csx_cholsol_factor on a forest of equal dense blocks, both orders, and a solve with each plan
    S = _spd_blocks(64, 16)
    n = S.shape[0]
    hA = keep(_csc(S))
    for exact in (1, 0):
        hL, plan = keep(X.new_handle()), keep(X.new_handle())
        X.check(lib.csx_cholsol_factor(hA, exact, hL, plan), "cholsol_factor")
        hB = keep(_vec(rng.uniform(-1, 1, n * 8)))
        X.check(lib.csx_cholsol_solve(plan, hB, 8), "cholsol_solve")
    # csx_cholsol_plan of the same factor from csx_chol in the rounding-equal order: the diagonal tiles' inverses
    keep(_chol(hA, n, forget_finding=True))
    hL = keep(_chol(hA, n))
    plan = keep(X.new_handle())
    X.check(lib.csx_cholsol_plan(hL, None, plan), "cholsol_plan")
    X.check(lib.csx_cholsol_set_order(plan, 0), "cholsol_set_order")
    X.check(lib.csx_cholsol_solve(plan, keep(_vec(rng.uniform(-1, 1, n * 16))), 16), "cholsol_solve")
    # a banded factor: one big tree (supernodal schedule in the rounding-equal order) and triangular plans in both orders
    S = _spd_band(3000, 24)
    n = S.shape[0]
    hA = keep(_csc(S))
    hL = keep(_chol(hA, n))
    plan = keep(X.new_handle())
    X.check(lib.csx_cholsol_plan(hL, None, plan), "cholsol_plan")
    X.check(lib.csx_cholsol_set_order(plan, 0), "cholsol_set_order")
    X.check(lib.csx_cholsol_solve(plan, keep(_vec(rng.uniform(-1, 1, n * 4))), 4), "cholsol_solve")
    for kind in (X.TRI_L, X.TRI_LT):
        tp = keep(X.new_handle())
        X.check(lib.csx_tri_analyse(hL, kind, tp), "tri_analyse")
        for exact in (1, 0):
            X.check(lib.csx_tri_set_order(tp, exact), "tri_set_order")
            X.check(lib.csx_tri_solve(tp, keep(_vec(rng.uniform(-1, 1, n * 16))), 16), "tri_solve")
    # the csx_lusol_solve pair on the factors of a batch of small blocks, both orders
    S = _lu_blocks(256, 6)
    n = S.shape[0]
    hA = keep(_csc(S))
    hLl, hUl, pinv, done = keep(X.new_handle()), keep(X.new_handle()), np.empty(n, np.int32), C.c_int(0)
    X.check(lib.csx_lu_blocks(hA, 1.0, hLl, hUl, X.pi(pinv), done), "lu_blocks")
    assert done.value == 1
    pl, pu = keep(X.new_handle()), keep(X.new_handle())
    X.check(lib.csx_tri_analyse(hLl, X.TRI_L, pl), "tri_analyse")
    X.check(lib.csx_tri_analyse(hUl, X.TRI_U, pu), "tri_analyse")
    hp = keep(_ivec(pinv))
    fused = C.c_int(0)
    for exact in (1, 0):
        X.check(lib.csx_tri_set_order(pl, exact), "tri_set_order")
        X.check(lib.csx_tri_set_order(pu, exact), "tri_set_order")
        hb, hw = keep(_vec(rng.uniform(-1, 1, n * 40))), keep(_vec(np.zeros(n * 40)))
        X.check(lib.csx_lusol_solve(pl, pu, hp, 0, hb, hw, 40, fused), "lusol_solve")
    # csx_btf_plan: two diagonal blocks, one of more than 96 rows (its own triangular plans), and a solve
    n, r = 300, np.array([0, 200, 300], np.int32)
    I = sp.identity(n, format="csc") * 2.0
    hLb, hUb, hF = keep(_csc(I)), keep(_csc(I)), keep(_csc(sp.csc_matrix((n, n))))
    ident = X.i32(np.arange(n))
    bp = keep(X.new_handle())
    X.check(lib.csx_btf_plan(hLb, hUb, hF, X.pi(ident), X.pi(ident), X.pi(ident), X.pi(r), X.pi(X.i32([0, 0])), 2, bp),
            "btf_plan")
    X.check(lib.csx_btf_solve(bp, keep(_vec(rng.uniform(-1, 1, n * 3))), keep(_vec(np.zeros(n * 3))), 3), "btf_solve")
    # csx_gaxpy_prepare's cached plans, dropped by csx_csc_invalidate
    hG = keep(_csc(sp.random(4000, 3000, 0.01, random_state=4, format="csc")))
    for mode in (X.GAXPY_TILED, X.GAXPY_EXACT):
        X.check(lib.csx_gaxpy_prepare(hG, mode), "gaxpy_prepare")
    X.check(lib.csx_gaxpy(hG, keep(_vec(np.ones(3000))), keep(_vec(np.zeros(4000))), X.GAXPY_AUTO), "gaxpy")
    X.check(lib.csx_csc_invalidate(hG), "csc_invalidate")
    for h in reversed(handles):     # (plans before the factors they borrow from)
        X.check(lib.csx_free(h), "free")


def test_failed_calls_give_their_memory_back(steady_live):
    X, lib = _lib()
    # csx_chol / csx_cholsol_factor on a matrix that is not positive definite
    S = _spd_blocks(64, 16, negative_block=37)
    n = S.shape[0]
    hA = _csc(S)
    parent, cp = _symbolic(hA, n)
    hL = X.new_handle()
    assert lib.csx_chol(hA, X.pi(parent), X.pi(cp), None, hL) == X.ENOTSPD
    for exact in (1, 0):
        assert lib.csx_cholsol_factor(hA, exact, X.new_handle(), X.new_handle()) == X.ENOTSPD
    X.check(lib.csx_free(hA), "free")
    # ... and with the general path: one big tree
    S = _spd_band(2000, 8).tolil()
    S[1500, 1500] = -1.0
    hA = _csc(S.tocsc())
    parent, cp = _symbolic(hA, 2000)
    assert lib.csx_chol(hA, X.pi(parent), X.pi(cp), None, X.new_handle()) == X.ENOTSPD
    assert lib.csx_cholsol_factor(hA, 1, X.new_handle(), X.new_handle()) == X.ENOTSPD
    X.check(lib.csx_free(hA), "free")
    # csx_tri_analyse on a triangle with an empty column
    T = sp.csc_matrix((np.ones(4), ([0, 1, 3, 3], [0, 1, 1, 3])), shape=(4, 4))
    hT = _csc(T)
    for kind in (X.TRI_L, X.TRI_U):
        assert lib.csx_tri_analyse(hT, kind, X.new_handle()) == X.EINVAL
    X.check(lib.csx_free(hT), "free")
    # csx_lu_blocks on a batch with a singular block: refused after its staging arrays exist
    hA = _csc(_lu_blocks(256, 6, singular_block=100))
    n = 256 * 6
    pinv, done = np.empty(n, np.int32), C.c_int(0)
    assert lib.csx_lu_blocks(hA, 1.0, X.new_handle(), X.new_handle(), X.pi(pinv), done) == X.ENOTSPD
    X.check(lib.csx_free(hA), "free")
