"""Transposed solves and the 1-norm condition estimate, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

lusol_trans(): A' x = b from cs_lu's factors (L U = A(p, q)) as the reference's own functions run it:
cs_pvec(q), cs_utsolve(U), cs_ltsolve(L), cs_pvec(pinv).

btf_solve_trans(): the transposed solve of btf_factor (C = A(p, q) = D + F, L U = D(pinv, :)) in plain Python floats, one
right-hand side, like btf_oracle.solve: c = b(q); blocks first to last, for every column j of a block c_j -= F(i, j) w_i in
F's column storage order; then the block's part of cs_utsolve(U), cs_ltsolve(L), cs_pvec(pinv); x(p) = w.  Every multiply
and every subtract is rounded on its own: the device must give the same bits.

condest_dense(): Hager-Higham's 1-norm estimate of cond_1(A) as LAPACK's dlacn2 iterates it, on dense solves."""
import numpy as np

import csparse_oracle as O


def _arrays(M):
    """(p, i, x) lists of a `cs`-like object or a tuple."""
    if isinstance(M, tuple):
        p, i, x = M
    else:
        p, i, x = M.p, M.i, M.x
    n = len(p) - 1
    nnz = int(p[n])
    return [int(v) for v in p], [int(v) for v in i[:nnz]], [float(v) for v in x[:nnz]]


class _M(object):
    """The minimum of a csparse_oracle CSC matrix the triangular solves read."""

    def __init__(self, M):
        self.p, self.i, self.x = _arrays(M)
        self.n = len(self.p) - 1
        self.m = self.n
        self.nz = -1


def lusol_trans(L, U, pinv, q, b):
    """x of A' x = b (a list of n floats) from L U = A(p, q); q None for the natural order."""
    Lm, Um = _M(L), _M(U)
    n = Lm.n
    pinv = [int(v) for v in pinv]
    qq = None if q is None else [int(v) for v in q]
    y = [0.0] * n
    O.cs_pvec(qq, [float(v) for v in b], y, n)
    O.cs_utsolve(Um, y)
    O.cs_ltsolve(Lm, y)
    x = [0.0] * n
    O.cs_pvec(pinv, y, x, n)
    return x


def btf_solve_trans(L, U, F, pinv, p, q, r, b):
    """x of A' x = b for one right-hand side b; L, U, F: `cs` objects or (p, i, x)."""
    Lp, Li, Lx = _arrays(L)
    Up, Ui, Ux = _arrays(U)
    Fp, Fi, Fx = _arrays(F)
    n = len(p)
    pinv = [int(v) for v in pinv]
    r = [int(v) for v in r]
    v = [0.0] * n                               # w_i = v[pinv_i]
    c = [float(b[int(q[k])]) for k in range(n)]
    for blk in range(len(r) - 1):
        a, e = r[blk], r[blk + 1]
        for j in range(a, e):
            acc = c[j]
            for t in range(Fp[j], Fp[j + 1]):
                acc = acc - Fx[t] * v[pinv[Fi[t]]]
            v[j] = acc
        for j in range(a, e):                   # cs_utsolve
            for t in range(Up[j], Up[j + 1] - 1):
                v[j] = v[j] - Ux[t] * v[Ui[t]]
            v[j] = v[j] / Ux[Up[j + 1] - 1]
        for j in range(e - 1, a - 1, -1):       # cs_ltsolve
            for t in range(Lp[j] + 1, Lp[j + 1]):
                v[j] = v[j] - Lx[t] * v[Li[t]]
            v[j] = v[j] / Lx[Lp[j]]
    x = [0.0] * n
    for i in range(n):
        x[int(p[i])] = v[pinv[i]]
    return x


def condest_dense(A):
    """cond_1 estimate of a square matrix (dense array or scipy sparse): |A|_1 times dlacn2's estimate of |A^-1|_1."""
    A = np.asarray(A.toarray() if hasattr(A, "toarray") else A, dtype=np.float64)
    n = A.shape[0]
    if n == 0:
        return 0.0
    norm_a = float(np.max(np.sum(np.abs(A), axis=0)))
    AT = A.T.copy()
    x = np.full(n, 1.0 / n)                                  # KASE = 1, JUMP = 1
    x = np.linalg.solve(A, x)
    if n == 1:
        return norm_a * abs(float(x[0]))
    est = float(np.sum(np.abs(x)))
    isgn = np.where(x >= 0.0, 1, -1)
    x = np.linalg.solve(AT, isgn.astype(np.float64))        # KASE = 2, JUMP = 2
    j = int(np.argmax(np.abs(x)))
    it = 2
    while True:
        x = np.zeros(n)                                      # label 50
        x[j] = 1.0
        x = np.linalg.solve(A, x)                            # JUMP = 3
        est_old = est
        est = float(np.sum(np.abs(x)))
        s = np.where(x >= 0.0, 1, -1)
        if np.array_equal(s, isgn):                          # repeated sign vector
            break
        if est <= est_old:                                   # cycling
            break
        isgn = s
        x = np.linalg.solve(AT, isgn.astype(np.float64))    # JUMP = 4
        j_last = j
        j = int(np.argmax(np.abs(x)))
        if x[j_last] != abs(x[j]) and it < 5:
            it += 1
            continue
        break
    alt = np.array([(1.0 if i % 2 == 0 else -1.0) * (1.0 + i / (n - 1.0)) for i in range(n)])
    temp = 2.0 * (float(np.sum(np.abs(np.linalg.solve(A, alt)))) / (3.0 * n))   # JUMP = 5
    return norm_a * max(est, temp)
