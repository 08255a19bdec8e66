"""Block triangular LU, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

solve(): the solve sequence of btf_factor in plain Python, from given factors, one right-hand side:
c = b(p); blocks from last to first: c_i -= F_ij z_j for the block's rows in cs_gaxpy's order (ascending column,
storage order within a column), then the block's part of cs_ipvec(pinv), cs_lsolve(L), cs_usolve(U) as the
reference's column loops run them; x(q) = z.  Python floats round every multiply and every subtract: the operations
are the ones the device must do, so results compare bit for bit.

btf_order() / split(): a textbook restatement of the factor-time steps (matching, strong components, levels, D / F)
for the CPU tests.  reducible(): generated reducible matrices with known blocks and depth."""
import numpy as np
import scipy.sparse as sp

import dm_oracle


def _arrays(M):
    """(p, i, x) lists of a `cs`-like object or a tuple."""
    if isinstance(M, tuple):
        p, i, x = M
    else:
        p, i, x = M.p, M.i, M.x
    n = len(p) - 1
    nnz = int(p[n])
    return [int(v) for v in p], [int(v) for v in i[:nnz]], [float(v) for v in x[:nnz]]


def solve(L, U, F, pinv, p, q, r, b):
    """x for one right-hand side b (a sequence of n floats); L, U, F: `cs` objects or (p, i, x)."""
    Lp, Li, Lx = _arrays(L)
    Up, Ui, Ux = _arrays(U)
    Fp, Fi, Fx = _arrays(F)
    n = len(p)
    pinv = [int(v) for v in pinv]
    r = [int(v) for v in r]
    rows = [[] for _ in range(n)]
    for j in range(n):                          # rows of F in cs_gaxpy's order
        for t in range(Fp[j], Fp[j + 1]):
            rows[Fi[t]].append((j, Fx[t]))
    c = [float(b[int(p[k])]) for k in range(n)]
    z = [0.0] * n
    for blk in range(len(r) - 2, -1, -1):
        a, e = r[blk], r[blk + 1]
        for i in range(a, e):
            acc = c[i]
            for j, v in rows[i]:
                acc = acc - v * z[j]
            c[i] = acc
        for k in range(a, e):                   # cs_ipvec(pinv) on the block
            z[pinv[k]] = c[k]
        for j in range(a, e):                   # cs_lsolve
            z[j] = z[j] / Lx[Lp[j]]
            for t in range(Lp[j] + 1, Lp[j + 1]):
                z[Li[t]] = z[Li[t]] - Lx[t] * z[j]
        for j in range(e - 1, a - 1, -1):       # cs_usolve
            z[j] = z[j] / Ux[Up[j + 1] - 1]
            for t in range(Up[j], Up[j + 1] - 1):
                z[Ui[t]] = z[Ui[t]] - Ux[t] * z[j]
    x = [0.0] * n
    for k in range(n):
        x[int(q[k])] = z[k]
    return x


def btf_order(n, Ap, Ai):
    """p, q, r, levels of a square structurally nonsingular pattern: blocks by level, highest first (None if singular)."""
    rm, cm = dm_oracle.matching(n, n, Ap, Ai)
    if any(v < 0 for v in cm):
        return None
    rows = dm_oracle._rows(n, n, Ap, Ai)
    succ = [[w for w in rows[cm[u]] if w != u] for u in range(n)]      # column u -> column w through row cm[u]
    comps = dm_oracle.tarjan(n, succ)                                   # reverse topological order
    blk = [0] * n
    for b, comp in enumerate(comps):
        for v in comp:
            blk[v] = b
    level = [0] * len(comps)
    for b, comp in enumerate(comps):
        for u in comp:
            for w in succ[u]:
                if blk[w] != b:
                    level[b] = max(level[b], level[blk[w]] + 1)
    order = sorted(range(len(comps)), key=lambda b: -level[b])
    p, q, r = [], [], [0]
    for b in order:
        for u in sorted(comps[b]):
            q.append(u)
            p.append(cm[u])
        r.append(len(q))
    return p, q, r, [level[b] for b in order]


def split(n, Ap, Ai, Ax, p, q, r):
    """D and F of C = A(p, q) as (p, i, x) lists, C's storage order kept."""
    pinv = [0] * n
    for k, v in enumerate(p):
        pinv[v] = k
    blk = [0] * n
    for b in range(len(r) - 1):
        for k in range(r[b], r[b + 1]):
            blk[k] = b
    D, F = ([0], [], []), ([0], [], [])
    for k in range(n):
        j = q[k]
        for t in range(Ap[j], Ap[j + 1]):
            i = pinv[Ai[t]]
            M = D if blk[i] == blk[k] else F
            M[1].append(i)
            M[2].append(float(Ax[t]))
        for M in (D, F):
            M[0].append(len(M[1]))
    return D, F


def reducible(sizes, depth, seed, density=1.0):
    """A reducible matrix: strongly connected blocks of the given sizes (a cycle plus random entries inside every block
    of two or more rows), coupled only to blocks of lower levels, `depth` levels (every block of level l > 0 reaches a
    block of level l - 1), rows made diagonally dominant, rows and columns permuted at random.

    Returns S (scipy CSC, sorted indices), blocks (set of (frozenset rows, frozenset cols)) and the levels."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    nb = len(sizes)
    n = int(sizes.sum())
    starts = np.concatenate([[0], np.cumsum(sizes)])
    level = rng.integers(0, depth, nb)
    if nb >= depth:
        level[:depth] = np.arange(depth)      # every level present
    by_level = [np.flatnonzero(level == l) for l in range(depth)]
    idx = np.arange(n)
    bof = np.repeat(np.arange(nb), sizes)
    nxt = idx + 1
    nxt[starts[1:] - 1] = starts[:-1]
    multi = sizes[bof] >= 2
    rows, cols = [idx[multi]], [nxt[multi]]
    ne = int(density * n)
    eb = bof[rng.integers(0, n, ne)]
    keep = sizes[eb] >= 2
    eb = eb[keep]
    rows.append(starts[eb] + (rng.random(len(eb)) * sizes[eb]).astype(np.int64))
    cols.append(starts[eb] + (rng.random(len(eb)) * sizes[eb]).astype(np.int64))
    # coupling: one entry into a block of level l - 1, one more into any lower level half the time
    for l in range(1, depth):
        src = by_level[l]
        if len(src) == 0:
            continue
        for pick in (by_level[l - 1], np.concatenate(by_level[:l])):
            if len(pick) == 0:
                continue
            s = src if pick is by_level[l - 1] else src[rng.random(len(src)) < 0.5]
            tb = pick[rng.integers(0, len(pick), len(s))]
            rows.append(starts[s] + (rng.random(len(s)) * sizes[s]).astype(np.int64))
            cols.append(starts[tb] + (rng.random(len(s)) * sizes[tb]).astype(np.int64))
    r = np.concatenate(rows)
    c = np.concatenate(cols)
    off = r != c
    r, c = r[off], c[off]
    v = rng.uniform(-1.0, 1.0, len(r))
    O = sp.csr_matrix((v, (r, c)), shape=(n, n))
    O.sum_duplicates()
    dom = np.asarray(abs(O).sum(axis=1)).ravel() + 1.0 + rng.random(n)
    S = (O + sp.diags(dom)).tocsc()
    pr, pc = rng.permutation(n), rng.permutation(n)
    S = S[pr][:, pc].tocsc()
    S.sort_indices()
    rinv, cinv = np.empty(n, np.int64), np.empty(n, np.int64)
    rinv[pr], cinv[pc] = np.arange(n), np.arange(n)
    blocks = set((frozenset(rinv[starts[b]:starts[b + 1]].tolist()), frozenset(cinv[starts[b]:starts[b + 1]].tolist()))
                 for b in range(nb))
    return S, blocks, int(level.max()) + 1 if nb else 0


def block_sizes(n, seed, big=()):
    """Sizes 1 .. 64 (mostly small) summing to n, plus the `big` ones."""
    rng = np.random.default_rng(seed)
    out = list(big)
    tot = sum(out)
    while tot < n:
        s = int(min(rng.geometric(0.3) if rng.random() < 0.9 else rng.integers(8, 65), 64, n - tot))
        out.append(s)
        tot += s
    rng.shuffle(out)
    return out
