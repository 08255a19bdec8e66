"""A pure-Python restatement of updown_block's column-fused order, the order the device kernel runs in:

- the terms (columns of C) are grouped by the tree of the elimination forest their path lies in (the root of the path);
- chunk s holds ranks [64 s, 64 s + 64) of every tree; the chunks run in order;
- in a chunk, each tree walks the union of its terms' paths in ascending column order; at a column, the terms whose path holds
  it run in ascending order: the scalar chain first (L(j,j) and beta_t carried from term to term), then every entry below the
  diagonal takes the terms in order;
- a downdate that is not positive definite at term t stops the terms >= t of its tree (for the rest of the call); the smallest
  failing term over all trees is the loop's first failing column; the union columns are then restored from the snapshots the
  chunks took before they ran (last chunk first) and, unless all or nothing is asked for, the chunks run again with terms
  [0, t] only.

updown_block(L, sigma, C, parent, all_or_nothing) changes the oracle `cs` L in place and returns the number of columns applied
in full; tests/test_updown_block_cpu.py holds it byte-equal to the loop of csparse_oracle.cs_updown.  schedule(L, C, parent)
models the launch rule (chunks, trees, union columns, masks, the four launch classes) for the cases of tests/updown_cases.py."""
from math import sqrt


def tree_of(L):
    """parent[j] = the row of the second entry of column j of L (rows ascending), -1 when there is none"""
    return [L.i[L.p[j] + 1] if L.p[j + 1] - L.p[j] > 1 else -1 for j in range(L.n)]


def _path(f, parent):
    out = []
    j = f
    while j != -1:
        out.append(j)
        j = parent[j]
    return out


def _run(L, sig, cols, trees, paths, limit, tfail, snaps):
    """every chunk once, terms with an index above `limit` left out; snaps (a list) gets each chunk's snapshot when given.
    Returns the smallest failing term (None: none)."""
    Lp, Li, Lx = L.p, L.i, L.x
    fail_min = None
    nchunks = max((len(tr) + 63) // 64 for tr in trees)
    for s in range(nchunks):
        chunk = []
        for g, tr in enumerate(trees):
            terms = tr[64 * s:64 * s + 64]
            if terms:
                chunk.append((g, terms))
        if snaps is not None:
            snap = {}
            for g, terms in chunk:
                for t in terms:
                    for j in paths[t]:
                        snap[j] = Lx[Lp[j]:Lp[j + 1]]
            snaps.append(snap)
        for g, terms in chunk:
            if tfail[g] is not None:
                continue                              # its later terms come after the one that failed
            alive = [t <= limit for t in terms]
            on = {}                                   # column -> the positions (bits) of the terms whose path holds it
            for b, t in enumerate(terms):
                for j in paths[t]:
                    on.setdefault(j, []).append(b)
            W = {}                                    # (row, bit) -> w_t(row); 0 on the path, then C's entries in order
            for b, t in enumerate(terms):
                for j in paths[t]:
                    W[(j, b)] = 0.0
                rows, vals = cols[t]
                for r, v in zip(rows, vals):
                    if (r, b) in W:
                        W[(r, b)] = v
            beta = [1.0] * len(terms)
            for j in sorted(on):
                bits = [b for b in on[j] if alive[b]]
                if not bits:
                    continue
                p = Lp[j]
                ljj = Lx[p]
                done = []
                scal = {}
                for b in bits:
                    wj = W[(j, b)]
                    sigma = sig[terms[b]]
                    alpha = wj / ljj
                    beta2 = beta[b] * beta[b] + sigma * alpha * alpha
                    if beta2 <= 0:
                        tfail[g] = terms[b]
                        fail_min = terms[b] if fail_min is None else min(fail_min, terms[b])
                        for b2 in range(b, len(terms)):
                            alive[b2] = False
                        break
                    beta2 = sqrt(beta2)
                    delta = (beta[b] / beta2) if sigma > 0 else (beta2 / beta[b])
                    gamma = sigma * alpha / (beta2 * beta[b])
                    ljj = delta * ljj + ((gamma * wj) if sigma > 0 else 0)
                    beta[b] = beta2
                    scal[b] = (alpha, delta, gamma, sigma)
                    done.append(b)
                if not done:
                    continue
                Lx[p] = ljj
                for q in range(p + 1, Lp[j + 1]):
                    r = Li[q]
                    lx = Lx[q]
                    for b in done:
                        alpha, delta, gamma, sigma = scal[b]
                        w1 = W[(r, b)]
                        W[(r, b)] = w2 = w1 - alpha * lx
                        lx = delta * lx + gamma * (w1 if sigma > 0 else w2)
                    Lx[q] = lx
    return fail_min


def updown_block(L, sigma, C, parent=None, all_or_nothing=False):
    n, k = L.n, C.n
    sig = [sigma] * k if sigma in (1, -1) else list(sigma)
    if parent is None:
        parent = tree_of(L)
    cols, f = [], []
    for t in range(k):
        rows = C.i[C.p[t]:C.p[t + 1]]
        cols.append((rows, C.x[C.p[t]:C.p[t + 1]]))
        f.append(min(rows) if rows else -1)
    paths = {t: _path(f[t], parent) for t in range(k) if f[t] >= 0}
    if not paths:
        return k
    by_root = {}
    for t in range(k):
        if f[t] >= 0:
            by_root.setdefault(paths[t][-1], []).append(t)
    trees = [by_root[r] for r in sorted(by_root)]
    snaps = []
    tfail = [None] * len(trees)
    t_fail = _run(L, sig, cols, trees, paths, k, tfail, snaps)
    if t_fail is None:
        return k
    for snap in reversed(snaps):
        for j, vals in snap.items():
            L.x[L.p[j]:L.p[j + 1]] = vals
    if not all_or_nothing:
        _run(L, sig, cols, trees, paths, t_fail, [None] * len(trees), None)
    return t_fail


# The launch rule of csx_updown_block.hip, restated here on purpose: a test that leans on these constants has to be looked
# at again when someone moves one of them in the kernel file.
UD_CHUNK = 64           # terms of a tree per chunk, one bit of the 64-bit mask each
UD_LDS_W = 60 * 1024    # bytes of W (ucnt x nterm doubles) a workgroup keeps in LDS
UD_WAVE = 64            # a tree whose longest union column (diagonal included) is longer than this runs on 256 lanes


def schedule(L, C, parent=None):
    """A model of the schedule the device call builds for (L, C): one entry per chunk, {"groups": [(nterm, ucnt, maxlen, cls)
    per tree of the chunk, trees by ascending root], "masks": {union column: the 64-bit mask of the chunk's terms on it}}.
    Chunk s holds ranks [64 s, 64 s + 64) of each tree's terms (ascending), empty columns of C dropped; ucnt = the union of
    the terms' paths, maxlen = its longest column, diagonal included; cls = (256 lanes: maxlen > 64) + 2 * (W in LDS:
    ucnt * nterm * 8 <= 61440), the index of csx_updown_block_classes."""
    if parent is None:
        parent = tree_of(L)
    paths = {}
    for t in range(C.n):
        rows = C.i[C.p[t]:C.p[t + 1]]
        if rows:
            paths[t] = _path(min(rows), parent)
    by_root = {}
    for t in sorted(paths):
        by_root.setdefault(paths[t][-1], []).append(t)
    trees = [by_root[r] for r in sorted(by_root)]
    out = []
    nchunks = max([(len(tr) + UD_CHUNK - 1) // UD_CHUNK for tr in trees] or [0])
    for s in range(nchunks):
        groups, masks = [], {}
        for tr in trees:
            terms = tr[UD_CHUNK * s:UD_CHUNK * s + UD_CHUNK]
            if not terms:
                continue
            m = {}
            for b, t in enumerate(terms):
                for j in paths[t]:
                    m[j] = m.get(j, 0) | (1 << b)
            nterm, ucnt = len(terms), len(m)
            maxlen = max(L.p[j + 1] - L.p[j] for j in m)
            cls = (1 if maxlen > UD_WAVE else 0) + (2 if ucnt * nterm * 8 <= UD_LDS_W else 0)
            groups.append((nterm, ucnt, maxlen, cls))
            masks.update(m)                           # trees share no column
        out.append({"groups": groups, "masks": masks})
    return out


def schedule_facts(sched):
    """what updown_info() reports of a schedule: chunks, groups and union columns (summed over the chunks), classes[cls]"""
    classes = [0, 0, 0, 0]
    for ch in sched:
        for g in ch["groups"]:
            classes[g[3]] += 1
    return {"chunks": len(sched), "groups": sum(len(ch["groups"]) for ch in sched),
            "union_columns": sum(len(ch["masks"]) for ch in sched), "classes": classes}


def loop(L, sigma, C, parent, mod):
    """the loop updown_block stands for: mod.cs_updown column by column until one fails; the count applied in full"""
    k = C.n
    sig = [sigma] * k if sigma in (1, -1) else list(sigma)
    for t in range(k):
        W = mod.cs_spalloc(C.m, 1, max(1, C.p[t + 1] - C.p[t]), True, False)
        W.p = [0, C.p[t + 1] - C.p[t]]
        W.i = list(C.i[C.p[t]:C.p[t + 1]]) or [0]
        W.x = list(C.x[C.p[t]:C.p[t + 1]]) or [0.0]
        if not mod.cs_updown(L, sig[t], W, parent):
            return t
    return k
