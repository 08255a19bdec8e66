"""The value rule of gmres() and of the csx_gs_* kernels, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

Written from §28, in plain Python floats and numpy indexing only: every multiply, add, subtract and divide is one rounded
IEEE operation.  Blocks are numpy arrays of rows x k; the basis is a list of blocks; every column is its own system.

    ordered_sum(terms)   leaves of GS_CHUNK consecutive terms added in ascending order from +0.0, inner nodes of GS_FAN consecutive
                         children added in ascending order from +0.0, until one value is left
    project / update / scale / combine   the four operations on the columns with mask[c] != 0
    Arnoldi              one column's Hessenberg matrix under its Givens rotations, and the back substitution
    gmres_loop           the whole loop over callables solve(B) -> X and residual(X, B) -> (R, omega)

single_pass=True (one Gram-Schmidt pass instead of two) and descending=True (the terms of a leaf added from the last to the
first) are two MISTAKES an implementation could make, kept so that the tests can show that neither gives the right bytes."""
import math

import numpy as np

import _csx

LIMITS = _csx.gmres_limits()
CHUNK, FAN = LIMITS["GS_CHUNK"], LIMITS["GS_FAN"]
EPS = 2.0 ** -52


def div(a, b):
    """a / b as IEEE 754 has it (Python raises for b == 0)"""
    if b == 0.0:
        if a == 0.0 or a != a or b != b:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def ordered_sum(terms, descending=False):
    node = []
    for start in range(0, len(terms), CHUNK):
        leaf = terms[start:start + CHUNK]
        s = 0.0
        for t in (reversed(leaf) if descending else leaf):
            s = s + t
        node.append(s)
    if not node:
        return 0.0
    while len(node) > 1:
        up = []
        for start in range(0, len(node), FAN):
            s = 0.0
            for t in node[start:start + FAN]:
                s = s + t
            up.append(s)
        node = up
    return node[0]


def dot(a, b, descending=False):
    return ordered_sum([float(x) * float(y) for x, y in zip(a, b)], descending)


def project(V, W, mask, negate=False, descending=False):
    """h (len(V) x k); NaN where the column is masked"""
    k = W.shape[1]
    h = np.full((len(V), k), np.nan)
    for c in range(k):
        if mask[c]:
            w = [-float(v) for v in W[:, c]] if negate else [float(v) for v in W[:, c]]
            for i, Vi in enumerate(V):
                h[i, c] = dot(Vi[:, c].tolist(), w, descending)
    return h


def update(V, W, mask, h, negate=False, descending=False):
    """(the new W, nrm2); masked columns of W as they were, of nrm2 NaN"""
    W = np.array(W, dtype=np.float64)
    k = W.shape[1]
    nrm2 = np.full(k, np.nan)
    for c in range(k):
        if mask[c]:
            col = []
            for r in range(W.shape[0]):
                w = -float(W[r, c]) if negate else float(W[r, c])
                for i, Vi in enumerate(V):
                    p = float(h[i, c]) * float(Vi[r, c])
                    w = w - p
                col.append(w)
            W[:, c] = col
            nrm2[c] = dot(col, col, descending)
    return W, nrm2


def scale(W, s, mask, old):
    """the block W / s on the live columns, `old` on the others"""
    out = np.array(old, dtype=np.float64)
    for c in range(W.shape[1]):
        if mask[c]:
            out[:, c] = [div(float(v), float(s[c])) for v in W[:, c]]
    return out


def combine(V, y, length, mask, old):
    """U = y[0] V_0 + ... over the column's own length: the first product, then one rounded addition per further product"""
    out = np.array(old, dtype=np.float64)
    for c in range(out.shape[1]):
        if mask[c]:
            for r in range(out.shape[0]):
                u = 0.0
                for i in range(int(length[c])):
                    p = float(y[i][c]) * float(V[i][r, c])
                    u = p if i == 0 else u + p
                out[r, c] = u
    return out


class Arnoldi(object):
    """column j comes in as (h[0 .. j], hnext): the rotations so far are applied to it, a new one (c, s) = (a, b) / sqrt(a a + b b)
    ((1, 0) when both are zero) clears hnext and turns g = (beta, 0, ...); |g[j + 1]| estimates the residual"""

    def __init__(self, beta):
        self.cols, self.cs, self.sn, self.g, self.beta = [], [], [], [beta], beta

    def step(self, h, hnext):
        col = [float(v) for v in h]
        for i in range(len(self.cs)):
            a, b = col[i], col[i + 1]
            col[i] = self.cs[i] * a + self.sn[i] * b
            col[i + 1] = self.cs[i] * b - self.sn[i] * a
        a, b = col[-1], float(hnext)
        d = math.sqrt(a * a + b * b)
        c, s = (1.0, 0.0) if d == 0.0 else (div(a, d), div(b, d))
        col[-1] = c * a + s * b
        gj = self.g[-1]
        self.g[-1] = c * gj
        self.g.append(-(s * gj))
        self.cs.append(c)
        self.sn.append(s)
        self.cols.append(col)

    def estimate(self):
        return div(abs(self.g[-1]), self.beta)

    def solution(self):
        jl = len(self.cols)
        y = [0.0] * jl
        for i in range(jl - 1, -1, -1):
            s = self.g[i]
            for l in range(i + 1, jl):
                s = s - self.cols[l][i] * y[l]
            y[i] = div(s, self.cols[i][i])
        return y


def gmres_loop(solve, residual, B, restart=16, maxit=64, inner_tol=2.0 ** -26, single_pass=False, descending=False):
    """{"x", "omega0", "omega", "iters", "cycles", "solves", "resid_est"} of the loop of gmres() on the n x k block B"""
    B = np.array(B, dtype=np.float64)
    n, k = B.shape
    zero = np.zeros((n, k))
    X = solve(B)
    R, w = residual(X, B)
    R, w = np.asarray(R, dtype=np.float64), np.asarray(w, dtype=np.float64)
    w0 = w.copy()
    iters, cycles, solves = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), 1
    est = np.ones(k)
    with np.errstate(all="ignore"):
        live = w > EPS
        while (live & (iters < maxit)).any():
            cyc = live & (iters < maxit)
            beta = np.array([math.sqrt(b2) if b2 >= 0.0 else math.nan for b2 in
                             (dot(R[:, c].tolist(), R[:, c].tolist(), descending) if cyc[c] else math.nan for c in range(k))])
            cyc = cyc & np.isfinite(beta) & (beta > 0.0)
            live = live & cyc
            if not cyc.any():
                break
            V = [scale(R, beta, cyc, zero)]
            arn = [Arnoldi(float(beta[c])) if cyc[c] else None for c in range(k)]
            act = cyc.copy()
            for j in range(restart):
                if not act.any():
                    break
                Z = solve(V[j])
                solves += 1
                W = residual(Z, zero)[0]                      # 0 - A Z: the sign is taken up below
                h = project(V, W, act, negate=True, descending=descending)
                W, nrm2 = update(V, W, act, h, negate=True, descending=descending)
                if not single_pass:
                    h2 = project(V, W, act, descending=descending)
                    W, nrm2 = update(V, W, act, h2, descending=descending)
                    h = h + h2
                stay = act.copy()
                hnext = np.zeros(k)
                for c in np.flatnonzero(act):
                    hnext[c] = math.sqrt(nrm2[c]) if nrm2[c] >= 0.0 else math.nan
                    arn[c].step(h[:, c], hnext[c])
                    iters[c] += 1
                    est[c] = arn[c].estimate()
                    left = abs(arn[c].g[-1]) <= inner_tol * arn[c].beta or not hnext[c] > 0.0
                    stay[c] = not (left or iters[c] >= maxit)
                if j + 1 < restart and stay.any():
                    V.append(scale(W, hnext, stay, zero))
                act = stay
            length = [len(a.cols) if a is not None else 0 for a in arn]
            y = [[0.0] * k for _ in range(max(length))]
            for c in np.flatnonzero(cyc):
                for i, v in enumerate(arn[c].solution()):
                    y[i][c] = v
            U = combine(V, y, length, cyc, zero)
            D = solve(U)
            solves += 1
            Xc = np.where(cyc[None, :], X + D, X)
            Rc, wc = residual(Xc, B)
            Rc, wc = np.asarray(Rc, dtype=np.float64), np.asarray(wc, dtype=np.float64)
            accept = cyc & (wc < w)
            X = np.where(accept[None, :], Xc, X)
            R = np.where(accept[None, :], Rc, R)
            cycles += accept
            live = accept & (wc > EPS)
            w = np.where(accept, wc, w)
    return {"x": X, "omega0": w0, "omega": w, "iters": iters, "cycles": cycles, "solves": solves, "resid_est": est}
