"""Fixtures and the CPU restatement of refine() -- TEST INFRASTRUCTURE, NOT PRODUCT.

stale_pivot(seed): a block-diagonal A of about 64 dense blocks of 2 .. 6 rows, strictly column diagonally dominant -- cs_lu
at tol = 1 then keeps the diagonal as pivots, and elimination preserves the dominance -- and values A2 on A's pattern,
uniform in (-1, 1), with the first diagonal entry of every block scaled to about 1e-6: a refactor keeps that entry as the
block's first pivot, the elimination grows by about 1e6, and a solve loses about six digits, which one or two steps of
refinement win back.  B: 5 right-hand sides, column ZERO_COLUMN all zeros.

refine_loop(): the loop of refine() on callables solve(B) -> X and residual(X, B) -> (R, omega), numpy blocks: the same
decisions, the candidate added with one rounding, rejected columns untouched."""
import numpy as np

EPS = 2.0 ** -52
SEEDS = (11, 12, 13)
K, ZERO_COLUMN = 5, 2


def stale_pivot(seed, nblocks=64):
    """(n, Ap, Ai, Ax, Ax2, B): CSC arrays (sorted columns), the new values, the right-hand sides (n x K)"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 7, nblocks)
    n = int(sizes.sum())
    Ap, Ai, Ax, Ax2 = [0], [], [], []
    start = 0
    for s in sizes.tolist():
        blk = rng.uniform(-1.0, 1.0, (s, s))
        new = rng.uniform(-1.0, 1.0, (s, s))
        for j in range(s):
            blk[j, j] = np.sum(np.abs(blk[:, j])) - abs(blk[j, j]) + 1.0 + rng.random()
        new[0, 0] = 1e-6 * rng.uniform(0.5, 1.0)
        for j in range(s):
            Ai += list(range(start, start + s))
            Ax += blk[:, j].tolist()
            Ax2 += new[:, j].tolist()
            Ap.append(len(Ai))
        start += s
    B = rng.uniform(-1.0, 1.0, (n, K))
    B[:, ZERO_COLUMN] = 0.0
    return n, np.asarray(Ap, np.int32), np.asarray(Ai, np.int32), np.asarray(Ax), np.asarray(Ax2), B


def refine_loop(solve, residual, B, maxit=5):
    """{"x", "omega0", "omega", "steps", "solves"} of the loop of refine() on the n x k block B"""
    B = np.array(B, dtype=np.float64)
    k = B.shape[1]
    X = solve(B)
    R, w = residual(X, B)
    w = np.asarray(w, dtype=np.float64)
    w0 = w.copy()
    steps, solves = np.zeros(k, dtype=np.int64), 1
    with np.errstate(invalid="ignore"):
        live = w > EPS
        for _ in range(maxit):
            if not live.any():
                break
            D = solve(R)
            solves += 1
            Xc = np.where(live[None, :], X + D, X)
            Rc, wc = residual(Xc, B)
            wc = np.asarray(wc, dtype=np.float64)
            accept = live & (wc < w)
            X = np.where(accept[None, :], Xc, X)
            R = np.where(accept[None, :], Rc, R)
            steps += accept
            live = accept & (wc > EPS) & (2.0 * wc <= w)
            w = np.where(accept, wc, w)
    return {"x": X, "omega0": w0, "omega": w, "steps": steps, "solves": solves}
