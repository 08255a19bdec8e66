"""The value rule of eigsh() and of the csx_bgs_* kernels, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

Written from §29 in elementwise float64 operations only: every multiply, add and subtract below is one rounded IEEE operation
on every element it touches (numpy's elementwise ufuncs; no dot, no matmul, no sum, no fused multiply-add), and the order of
the operations on any one element is spelled out by the Python loops.  Blocks are numpy arrays, the basis is a list of blocks.

    ordered_sum(terms)   terms[r] added over r: leaves of GS_CHUNK consecutive rows in ascending order from +0.0, inner nodes of
                         GS_FAN consecutive children in ascending order from +0.0, until one value is left
    gram / update / combine   the three operations in which the columns of a block mix
    eig_loop             the whole loop over callables solve(B) -> X, product(X) -> -(M X) (None: no mass matrix) and
                         residual(X, B) -> (R, omega); its small dense steps are the product's own function (csparse._eig_dense)

single_pass=True (one projection pass instead of two) and descending=True (the (i, a) terms of combine taken from the last to
the first) are two MISTAKES an implementation could make, kept so that the tests can show that neither gives the right bytes."""
import numpy as np

import _csx
import csparse

LIMITS = _csx.bgs_limits()
CHUNK, FAN, MAXW, GROUP = LIMITS["GS_CHUNK"], LIMITS["GS_FAN"], LIMITS["BGS_MAXW"], LIMITS["BGS_GROUP"]
dense = csparse._eig_dense


def _tree(node, shape):
    """the inner levels of the ordered sum over the leaf sums in `node`"""
    if not node:
        return np.zeros(shape)
    while len(node) > 1:
        up = []
        for start in range(0, len(node), FAN):
            s = np.zeros(shape)
            for t in node[start:start + FAN]:
                s = s + t
            up.append(s)
        node = up
    return node[0]


def ordered_sum(terms):
    """terms: (rows, ...) -> (...): the ordered sum over the first axis"""
    terms = np.asarray(terms, dtype=np.float64)
    node = []
    for start in range(0, terms.shape[0], CHUNK):
        s = np.zeros(terms.shape[1:])
        for r in range(start, min(start + CHUNK, terms.shape[0])):
            s = s + terms[r]
        node.append(s)
    return _tree(node, terms.shape[1:])


def gram(V, W, negate=False):
    """out[i, a, c] = ordered sum over r of V_i[r, a] * (+-W[r, c]); the products are formed one leaf at a time"""
    W = np.asarray(W, dtype=np.float64)
    w = -W if negate else W
    rows, q = W.shape
    out = []
    for Vi in V:
        Vi = np.asarray(Vi, dtype=np.float64)
        node = []
        for start in range(0, rows, CHUNK):
            stop = min(start + CHUNK, rows)
            prod = Vi[start:stop, :, None] * w[start:stop, None, :]
            s = np.zeros(prod.shape[1:])
            for r in range(stop - start):
                s = s + prod[r]
            node.append(s)
        out.append(_tree(node, (Vi.shape[1], q)))
    return np.array(out).reshape(len(V), -1, q)


def update(V, W, H):
    """W[r, c] - H[0, 0, c] V_0[r, 0] - H[0, 1, c] V_0[r, 1] - ..., ascending in (i, a)"""
    W = np.array(W, dtype=np.float64)
    for i, Vi in enumerate(V):
        for a in range(Vi.shape[1]):
            p = H[i][a][None, :] * Vi[:, a][:, None]
            W = W - p
    return W


def combine(V, S, rows, q, descending=False):
    """S[0, 0, c] V_0[r, 0] + ..., ascending in (i, a): the first product as it is, then one rounded addition per product"""
    terms = [(i, a) for i, Vi in enumerate(V) for a in range(Vi.shape[1])]
    if descending:
        terms.reverse()
    U = np.zeros((rows, q))
    for t, (i, a) in enumerate(terms):
        p = S[i][a][None, :] * V[i][:, a][:, None]
        U = p if t == 0 else U + p
    return U


def eig_loop(solve, product, residual, n, nev, sigma=0.0, block=None, maxblocks=32, tol=2.0 ** -30, seed=0, v0=None,
             single_pass=False, descending=False):
    """the loop of eigsh(): its result dict, with vectors as an array"""
    b = block
    if b is None:
        b = min(MAXW, max(nev, 8))
        b = min(MAXW, b + (b & 1))
    b = min(b, n)
    nb = min(maxblocks, max(2, n // b))
    assert 1 <= nev <= (nb - 1) * b
    mass = product is not None
    sgn = -1.0 if mass else 1.0
    count = {"solves": 0, "products": 0}

    def prod(X):
        count["products"] += 1
        return np.asarray(product(X), dtype=np.float64)

    def orthonormalise(src, s):
        R, blk, sign = [], src, s
        for first in (True, False):
            G = gram([blk], prod(blk), negate=True)[0] if mass else gram([blk], blk)[0]
            r = dense("cholqr", G, first)
            if r is None:
                return None, None
            R.append(r[0])
            blk, sign = combine([blk], [sign * r[1]], n, b), 1.0
        return blk, R[1] @ R[0]

    with np.errstate(all="ignore"):
        start = np.random.default_rng(seed).random((n, b)) - 0.5 if v0 is None else np.array(v0, dtype=np.float64)
        q0, _ = orthonormalise(start, 1.0)
        if q0 is None:
            raise ValueError("dependent starting block")
        Q = [q0]
        P = [prod(q0)] if mass else Q
        T = np.zeros((nb * b, nb * b))
        breakdown, done, j = False, False, 0
        while not done:
            nv = j + 1
            W = np.asarray(solve(P[j]), dtype=np.float64)
            count["solves"] += 1
            H1 = gram(P, W)
            W = update(Q, W, sgn * H1)
            H = H1
            if not single_pass:
                H2 = gram(P, W)
                W = update(Q, W, sgn * H2)
                H = H1 + H2
            T[:nv * b, j * b:nv * b] = H.reshape(nv * b, b)
            qn, Bsub = orthonormalise(W, sgn)
            if qn is None:
                breakdown = True
            else:
                Q.append(qn)
                if mass:
                    P.append(prod(qn))
            m = nv * b
            theta, S, est = dense("ritz", T[:m, :m], Bsub)
            last = breakdown or j + 2 >= nb
            kk = min(nev, m)
            if last or (kk == nev and (est[:nev] <= tol).all()):
                resid, omega, X = np.empty(kk), np.empty(kk), np.empty((n, kk))
                for c0 in range(0, kk, MAXW):
                    c1 = min(c0 + MAXW, kk)
                    Sc = S[:, c0:c1].reshape(nv, b, c1 - c0)
                    Xc = combine(Q[:nv], Sc, n, c1 - c0, descending=descending)
                    th = theta[c0:c1]
                    Bc = prod(Xc) / (-th)[None, :] if mass else Xc / th[None, :]
                    Rc, w = residual(Xc, Bc)
                    Rc = np.asarray(Rc, dtype=np.float64)
                    omega[c0:c1] = w
                    resid[c0:c1] = np.sqrt(ordered_sum(Rc * Rc)) / np.sqrt(ordered_sum(Bc * Bc))
                    X[:, c0:c1] = Xc
                done = last or bool((resid <= tol).all())
            j += 1
    return {"values": sigma + 1.0 / theta[:kk], "vectors": X, "resid": resid, "omega": omega, "estimate": est[:kk].copy(),
            "converged": resid <= tol, "blocks": j, "solves": count["solves"], "products": count["products"], "breakdown": breakdown}
