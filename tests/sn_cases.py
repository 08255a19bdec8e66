"""Inputs of tests/test_gpu_snsolve.py: synthetic Cholesky-shaped factors built for the edges of the supernodal solve's
schedule (csparse.py_amd/csrc/csx_snsolve.hip), and a model of that schedule written from its rules.

A factor is (n, Lp, Li, Lx): a lower triangle, diagonal first, rows ascending, int32 indices.  Every pattern is
Cholesky-shaped by construction: parent[j] is the first row below the diagonal and struct(L[:, j]) \\ {j} is a subset of
struct(L[:, parent[j]]) (`is_cholesky_shaped`).  They go to the device as they are (csx_csc_upload, csx_cholsol_plan,
csx_cholsol_set_order(plan, 0)): no ordering and no factorisation stands between a case and the schedule.

`sn_model` restates what the plan builder decides from the pattern alone, `sn_expected_launches` what a sweep enqueues for
a number of right-hand sides.  tests/test_sn_cases_cpu.py shows (without a device) that every case of CASES sits on the
edge it is named for; the GPU tests then hold the library's read-backs (csx_cholsol_sn_geometry, csx_cholsol_sn_launches)
to the model field for field."""
import functools

import numpy as np

SN_SEG = 256      # terms per piece of a cut line
SN_WHOLE = 512    # a supernode's line of up to this many outside terms stays whole
SN_LEAF = 64      # columns of a leaf subtree
GUARD = 1e3       # largest || |inv(L_ii)| |L_ii| ||_inf the matrix-core triangles accept
WG_TASKS = 16384  # a step of up to this many tasks takes a workgroup per task
THIN_TASKS, THIN_RHS, THIN_SHORT, THIN_ANY = 8192, 32, 48, 50000


# ---- patterns -----------------------------------------------------------------------------------------------------

def _block(first, m, dense, reach, up):
    """columns first .. first + m - 1: a chain (column k: k, k + 1) or a clique (k .. m - 1); the last `reach` columns carry
    the rows `up` (ascending, all above the block) as well.  Returns (count per column, rows of all columns)."""
    up = np.asarray(up, np.int64)
    c = first + np.arange(m, dtype=np.int64)
    cnt = np.empty(m, np.int64)
    parts = []
    for k in range(m):
        own = c[k:] if dense else c[k:k + 2]
        rows = np.concatenate([own, up]) if k >= m - reach else own
        cnt[k] = rows.size
        parts.append(rows)
    return cnt, (np.concatenate(parts) if parts else np.zeros(0, np.int64))


def comb(branches, leaf, w, wr, reach=1, root_reach=1, leaf_root_reach=None, leaves=1, dense_leaf=False, reach0=None, spread=False):
    """`branches` x (`leaves` leaf subtrees of `leaf` columns under one fundamental supernode of `w` columns), all under a
    root supernode of `wr` columns.
    reach: how many of a leaf's last columns carry the rows of the supernode above (an int, or one per leaf of a branch):
        the outside terms of a supernode row.  reach0: the same for the first branch alone.
    root_reach: how many root rows (the first ones) the supernode columns carry: the outside rows of a supernode column.
    leaf_root_reach (default root_reach, at most root_reach): how many root rows the reaching leaf columns carry too.
    w = 0: the leaves hang off the root directly.
    spread (with root_reach = 1): branch b carries root row b mod wr instead of the first.  With thousands of branches under
        one root row that row's sum has tens of thousands of terms, and the reference's own rounding in such a sum -- up to
        terms x eps x sum|terms| -- is then as large as the 1e-12 the solutions are compared at.
    Returns the pattern (n, Lp, Li)."""
    lrr = root_reach if leaf_root_reach is None else leaf_root_reach
    assert 1 <= root_reach <= wr and 0 <= lrr <= root_reach and (w > 0 or lrr >= 1)
    assert not spread or (root_reach == 1 and reach0 is None)
    assert w == 0 or root_reach < wr        # (with all of the root's rows below it a supernode would join the root's)
    per = lambda r: [r] * leaves if np.isscalar(r) else list(r)
    stride = leaves * leaf + w
    root0 = branches * stride

    def branch(b, reaches):
        base = b * stride
        srows = base + leaves * leaf + np.arange(w, dtype=np.int64)
        up_leaf = np.concatenate([srows, root0 + np.arange(lrr, dtype=np.int64)])
        cnts, rows = [], []
        for t in range(leaves):
            assert 1 <= reaches[t] <= leaf
            c, r = _block(base + t * leaf, leaf, dense_leaf, reaches[t], up_leaf)
            cnts.append(c)
            rows.append(r)
        if w:
            c, r = _block(base + leaves * leaf, w, True, w, root0 + np.arange(root_reach, dtype=np.int64))
            cnts.append(c)
            rows.append(r)
        return np.concatenate(cnts), np.concatenate(rows)

    cnts, rows = [], []
    first_general = 0
    if reach0 is not None:
        c, r = branch(0, per(reach0))
        cnts.append(c)
        rows.append(r)
        first_general = 1
    nb = branches - first_general
    if nb > 0:      # one branch, shifted: the rows below root0 move with the branch, the root's rows stay
        c, r = branch(first_general, per(reach))
        shift = np.repeat(np.arange(nb, dtype=np.int64) * stride, r.size)
        tiled = np.tile(r, nb)
        rows.append(np.where(tiled < root0, tiled + shift, tiled + (shift // stride % wr if spread else 0)))
        cnts.append(np.tile(c, nb))
    c, r = _block(root0, wr, True, 0, [])
    cnts.append(c)
    rows.append(r)
    cnt = np.concatenate(cnts)
    n = root0 + wr
    Lp = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=Lp[1:])
    assert Lp[n] < 2 ** 31
    return n, Lp.astype(np.int32), np.concatenate(rows).astype(np.int32)


def band_chain(n, seed, dense_at=None, dense_w=0, twig=None):
    """one chain of n columns with a band of 3 and holes (a column: itself, the next of the chain, some of the two after), no
    two neighbours with the same rows; optionally a dense trapezoid of dense_w columns from column dense_at on (a fundamental
    run inside it), and a twig = (p, q): column p is off the chain, a single column whose only row below is q."""
    rng = np.random.default_rng(seed)
    has3 = rng.random(n) < 0.5
    has2 = rng.random(n) < 0.5
    has2[1:] |= has3[:-1]                     # a column has the third after it  =>  its parent has it too
    chain = [j for j in range(n) if twig is None or j != twig[0]]
    assert twig is None or (twig[0] < twig[1] < n and (dense_at is None or twig[1] + 3 < dense_at))
    cols = [None] * n
    for t, j in enumerate(chain):
        if dense_at is not None and dense_at <= j < dense_at + dense_w:
            rows = list(range(j, min(n, dense_at + dense_w + 1)))
        else:
            rows = [j] + [chain[t + d] for d, on in ((1, True), (2, has2[t]), (3, has3[t])) if on and t + d < len(chain)]
            if dense_at is not None and j < dense_at:      # nothing reaches over the trapezoid's first column but into it
                rows = [r for r in rows if r < dense_at + 3]
        cols[j] = rows
    if twig is not None:
        cols[twig[0]] = list(twig)
    cnt = np.asarray([len(c) for c in cols], np.int64)
    Lp = np.zeros(n + 1, np.int32)
    np.cumsum(cnt, out=Lp[1:])
    return n, Lp, np.concatenate([np.asarray(c, np.int32) for c in cols])


def stack(below, above):
    """the tree `above` on top of the tree `below`: the last column of `below` gets the first column of `above` as its parent"""
    (na, Ap, Ai), (nb, Bp, Bi) = below, above
    Ai = np.concatenate([Ai, [na]]).astype(np.int32)
    Lp = np.concatenate([Ap[:-1], [Ap[na] + 1], Ap[na] + 1 + Bp[1:]]).astype(np.int32)
    return na + nb, Lp, np.concatenate([Ai, Bi + na]).astype(np.int32)


def values(n, Lp, Li, seed, bad_block=None):
    """diagonal: 2 + the column's count with a random sign; off-diagonals uniform in (-1, 1).  bad_block = first column of a
    16 x 16 diagonal block of a dense trapezoid that gets -0.9 below a unit diagonal (the growth guard's cases)."""
    rng = np.random.default_rng(seed)
    Lx = rng.uniform(-1.0, 1.0, Li.size)
    cnt = np.diff(Lp)
    Lx[Lp[:-1]] = rng.choice([-1.0, 1.0], n) * (2.0 + cnt)
    if bad_block is not None:
        for t in range(16):
            j = bad_block + t
            assert cnt[j] >= 16 - t and Li[Lp[j] + 15 - t] == bad_block + 15      # dense inside the block
            Lx[Lp[j]] = 1.0
            Lx[Lp[j] + 1:Lp[j] + 16 - t] = -0.9
    return Lx


def parent_of(n, Lp, Li):
    cnt = np.diff(Lp)
    par = np.full(n, -1, np.int64)
    has = cnt > 1
    par[has] = Li[Lp[:-1][has] + 1]
    return par


def is_cholesky_shaped(n, Lp, Li):
    """diagonal first, rows ascending, and every column's rows below its parent's diagonal are rows of the parent"""
    Lp64 = Lp.astype(np.int64)
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(Lp64))
    rows = Li.astype(np.int64)
    if not (np.all(rows[Lp64[:-1]] == np.arange(n)) and np.all(rows < n)):
        return False
    inner = np.ones(rows.size, bool)
    inner[Lp64[:-1]] = False
    if not np.all(np.diff(rows)[inner[1:]] > 0):
        return False
    par = parent_of(n, Lp, Li)
    key = np.sort(col * n + rows)                               # the pattern as a set of (column, row)
    want = inner & (rows != par[col])                           # the rows that the parent has to have
    probe = par[col[want]] * n + rows[want]
    at = np.searchsorted(key, probe)
    return bool(np.all(at < key.size) and np.all(key[np.minimum(at, key.size - 1)] == probe))


# ---- the schedule, restated -----------------------------------------------------------------------------------------

def _ceil(a, b):
    return -(-a // b)


def _supernodes(n, par, cnt, leaf_of, chunk, relaxed_ok):
    """The columns outside the leaf subtrees, in order, as supernodes (first, width, kind).
    FUNDAMENTAL: a column continues its predecessor's supernode when it is that column's parent and has one row less; the
    supernode that starts at a is then the whole run of such columns after a.
    RELAXED (where allowed, and unless a run of 32 or more starts at a): the range [a, e) with the largest e such that
      * e <= a + chunk, all of [a, e) lies outside the leaf subtrees, and no column after a inside it starts a fundamental
        run of 32 or more (such a run stays a supernode of its own);
      * every column of [a, e - 1) has its parent inside [a, e) -- so a root can only be the last column.
    It is taken when it has more than one column; it then wins over the fundamental run that starts at a."""
    out = leaf_of < 0
    fj = np.zeros(n + 1, bool)                      # column c continues the fundamental supernode of c - 1
    fj[1:n] = out[1:] & out[:-1] & (par[:-1] == np.arange(1, n)) & (cnt[1:] == cnt[:-1] - 1)
    stops = np.flatnonzero(~fj[1:]) + 1             # run that starts at c: up to the first column after c that does not continue
    run = stops[np.searchsorted(stops, np.arange(n), side="right")] - np.arange(n)
    wide_start = (run >= 32) & ~fj[:n]
    up = np.where(par >= 0, par, n + chunk)         # a root's parent is nowhere
    sns = []
    a = 0
    while a < n:
        if not out[a]:
            a += 1
            continue
        e = a + 1
        if relaxed_ok and run[a] < 32:
            lim = min(n, a + chunk)
            barred = np.flatnonzero(~out[a + 1:lim] | wide_start[a + 1:lim])
            if barred.size:
                lim = a + 1 + int(barred[0])
            ends = np.arange(a + 2, lim + 1)                              # candidates for e
            ok = np.maximum.accumulate(up[a:lim - 1])[:ends.size] < ends    # max parent of [a, e - 1) inside [a, e)
            if ok.any():
                e = int(ends[ok][-1])
        if e > a + 1:
            sns.append((a, e - a, "relaxed"))
        else:
            sns.append((a, int(run[a]), "fundamental"))
            e = a + int(run[a])
        a = e
    return sns


def _build(n, Lp, Li, mode, chunk):
    Lp64 = Lp.astype(np.int64)
    cnt = np.diff(Lp64)
    par = parent_of(n, Lp, Li)
    relaxed_ok = mode == 1
    leaf_min = 8 if relaxed_ok else 1       # (shorter twigs are left to the relaxed ranges)
    # leaf subtrees: the maximal subtrees of leaf_min .. SN_LEAF columns
    size = np.ones(n, np.int64)
    height = np.zeros(n, np.int64)
    pl, sl, hl = par.tolist(), size.tolist(), height.tolist()
    for j in range(n):
        p = pl[j]
        if p >= 0:
            sl[p] += sl[j]
            if hl[j] + 1 > hl[p]:
                hl[p] = hl[j] + 1
    col_levels = max(hl) + 1
    leaf_of = [-1] * n
    nleaf = 0
    for j in range(n - 1, -1, -1):
        p = pl[j]
        if p >= 0 and leaf_of[p] >= 0:
            leaf_of[j] = leaf_of[p]
        elif leaf_min <= sl[j] <= SN_LEAF:
            leaf_of[j] = nleaf
            nleaf += 1
    leaf_of = np.asarray(leaf_of, np.int64)
    leaf_sizes = np.bincount(leaf_of[leaf_of >= 0], minlength=nleaf)
    sns = _supernodes(n, par, cnt, leaf_of, chunk, relaxed_ok)
    if not sns:
        return None
    first = np.asarray([s[0] for s in sns], np.int64)
    width = np.asarray([s[1] for s in sns], np.int64)
    nsn = len(sns)
    sn_of = np.full(n, -1, np.int64)
    sn_of[np.concatenate([np.arange(a, a + w) for a, w, _ in sns])] = np.repeat(np.arange(nsn), width)
    last = first + width - 1
    spar = np.where(par[last] >= 0, sn_of[np.maximum(par[last], 0)], -1)
    hgt, dep = [0] * nsn, [0] * nsn
    for S in range(nsn):
        if spar[S] >= 0:
            hgt[spar[S]] = max(hgt[spar[S]], hgt[S] + 1)
    for S in range(nsn - 1, -1, -1):
        if spar[S] >= 0:
            dep[S] = dep[spar[S]] + 1
    hgt, dep = np.asarray(hgt), np.asarray(dep)
    lev_w = np.zeros(hgt.max() + 1, np.int64)
    np.maximum.at(lev_w, hgt, width)
    est_steps = int(np.sum(_ceil(lev_w, chunk)))
    # outside terms of every line: a row's terms from columns before its supernode, a column's rows below its supernode;
    # of a leaf column: its rows outside its subtree
    col = np.repeat(np.arange(n, dtype=np.int64), cnt)
    row = Li.astype(np.int64)
    off = row != col
    a_of = np.where(sn_of >= 0, first[np.maximum(sn_of, 0)], 0)
    e_of = np.where(sn_of >= 0, (first + width)[np.maximum(sn_of, 0)], 0)
    fwd_out = np.bincount(row[off & (col < a_of[row])], minlength=n)
    bwd_out = np.bincount(col[off & (row >= e_of[col])], minlength=n)
    leaf_out = np.bincount(col[off & (leaf_of[col] >= 0) & (leaf_of[row] != leaf_of[col])], minlength=n)
    pieces = _ceil(leaf_out, SN_SEG)
    chunks = [(a + c, min(chunk, w - c)) for a, w, _ in sns for c in range(0, w, chunk)]
    M = {
        "mode": mode, "chunk": chunk, "has_relaxed": int(any(s[2] == "relaxed" for s in sns)),
        "leaf_subtrees": nleaf, "leaf_sizes": leaf_sizes.tolist(), "leaf_cols": int(leaf_sizes.sum()),
        "leaf_tasks": int(pieces.sum()), "leaf_slots": int(pieces[pieces > 1].sum()),
        "supernodes": sns, "fundamental": sum(s[2] == "fundamental" for s in sns),
        "relaxed": sum(s[2] == "relaxed" for s in sns), "chunks": chunks,
        "est_steps": est_steps, "col_levels": col_levels, "kept": 8 * est_steps <= col_levels,
        "leaf_of": leaf_of, "max_tree": int(max(sl)),
    }
    for name, level, outside in (("fwd", hgt, fwd_out), ("bwd", dep, bwd_out)):
        steps = []
        for lv in range(level.max() + 1):
            here = np.flatnonzero(level == lv)
            nch = _ceil(width[here], chunk)
            for q in range(int(nch.max())):
                st = {"tasks": 0, "terms": 0, "cut": [], "max_uncut": 0, "narrow": 0, "medium": 0, "wide": 0}
                for S, k in zip(here, nch):
                    if q >= k:
                        continue
                    a, w = int(first[S]), int(width[S])
                    if q == 0:          # every line of the supernode: its outside terms, cut into pieces past SN_WHOLE
                        c = outside[a:a + w]
                        whole = c[(c > 0) & (c <= SN_WHOLE)]
                        st["tasks"] += whole.size
                        st["max_uncut"] = max(st["max_uncut"], int(whole.max()) if whole.size else 0)
                        for v in c[c > SN_WHOLE].tolist():
                            st["cut"].append([SN_SEG] * (v // SN_SEG) + ([v % SN_SEG] if v % SN_SEG else []))
                            st["tasks"] += _ceil(v, SN_SEG)
                        st["terms"] += int(c.sum())
                        cw = min(chunk, w) if name == "fwd" else w - (k - 1) * chunk
                    elif name == "fwd":  # chunk q - 1 is solved: the rows after it take their terms of its columns
                        st["tasks"] += w - q * chunk
                        st["terms"] += (w - q * chunk) * chunk
                        cw = min(chunk, w - q * chunk)
                    else:                # chunk k - q is solved: the columns before it take their terms of its rows
                        r0 = (k - q) * chunk
                        st["tasks"] += r0
                        st["terms"] += r0 * (min(w, r0 + chunk) - r0)
                        cw = chunk
                    st["wide" if cw > 32 else "medium" if cw > 16 else "narrow"] += 1
                st["triangles"] = st["narrow"] + st["medium"] + st["wide"]
                steps.append(st)
        M[name] = {
            "step_list": steps, "steps": len(steps), "tasks": sum(s["tasks"] for s in steps),
            "max_step_tasks": max(s["tasks"] for s in steps), "cut_lines": sum(len(s["cut"]) for s in steps),
            "slots": sum(len(p) for s in steps for p in s["cut"]),
            "narrow": sum(s["narrow"] for s in steps), "medium": sum(s["medium"] for s in steps),
            "wide": sum(s["wide"] for s in steps), "one_triangle_steps": sum(s["triangles"] == 1 for s in steps),
        }
    return M


def guard_measure(n, Lp, Li, Lx, M):
    """the largest || |inv(D)| |D| ||_inf over the 16 x 16 diagonal blocks D of every chunk's triangle and (when the plan
    puts the leaf subtrees on the matrix cores too: mode 1) of every leaf subtree's, rows past the end those of the identity"""
    unit = np.full(n, -1, np.int64)
    loc = np.zeros(n, np.int64)
    widths = []
    for u, (a, w) in enumerate(M["chunks"]):
        unit[a:a + w] = u
        loc[a:a + w] = np.arange(w)
        widths.append(w)
    if M["mode"] == 1 and M["leaf_subtrees"]:
        lo = M["leaf_of"]
        cols = np.flatnonzero(lo >= 0)
        order = cols[np.argsort(lo[cols], kind="stable")]
        sizes = np.asarray(M["leaf_sizes"], np.int64)
        start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        unit[order] = len(M["chunks"]) + lo[order]
        loc[order] = np.arange(order.size) - np.repeat(start, sizes)
        widths += sizes.tolist()
    nb = _ceil(np.asarray(widths, np.int64), 16)
    base = np.concatenate([[0], np.cumsum(nb)])
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(Lp.astype(np.int64)))
    row = Li.astype(np.int64)
    keep = (unit[row] == unit[col]) & (unit[col] >= 0) & (loc[row] // 16 == loc[col] // 16)
    worst = 0.0
    D = np.zeros((int(base[-1]), 16, 16))
    D[:, np.arange(16), np.arange(16)] = 1.0
    D[base[unit[col[keep]]] + loc[col[keep]] // 16, loc[row[keep]] % 16, loc[col[keep]] % 16] = Lx[keep]
    for s in range(0, D.shape[0], 8192):
        blk = D[s:s + 8192]
        worst = max(worst, float((np.abs(np.linalg.inv(blk)) @ np.abs(blk)).sum(axis=2).max()))
    return worst


def sn_model(n, Lp, Li, mode, guard=None):
    """What the plan builder decides for "tri.supernodes" = mode (1: relaxed supernodes, triangles on the matrix cores;
    2: fundamental supernodes only, triangles by substitution), from the pattern alone.  guard(M): the growth guard's measure
    of a build (`guard_measure`; None: every block passes).  Returns None when there is no supernodal plan.
    Mode 1 builds with chunks of 128 first.  That plan exists only with the matrix-core fragments; when the guard refuses
    them the build is repeated with chunks of 64 -- other ranges, other diagonal blocks, so the guard is asked again.  The
    second plan goes to the matrix cores if it passes, and is otherwise kept (by substitution) only if it has no relaxed
    supernode.  M["growth"]: the measure of every build tried, by chunk size."""
    growth = {}
    for chunk in ((128, 64) if mode == 1 else (64,)):
        M = _build(n, Lp, Li, mode, chunk)
        if M is None or not M["kept"]:
            continue
        growth[chunk] = guard(M) if guard and mode == 1 else 0.0
        M["growth"] = growth
        M["matrix_cores"] = int(mode == 1 and growth[chunk] <= GUARD)
        if (M["has_relaxed"] or chunk > 64) and not M["matrix_cores"]:
            continue
        return M
    return None


GEOMETRY_PLAN = ("chunk", "has_relaxed", "matrix_cores", "leaf_subtrees", "leaf_cols", "leaf_tasks", "leaf_slots",
                 "fundamental", "relaxed")
GEOMETRY_DIR = ("steps", "tasks", "max_step_tasks", "cut_lines", "slots", "narrow", "medium", "wide", "one_triangle_steps")


def model_geometry(M):
    """the model in the shape of _csx.cholsol_sn_geometry's dict"""
    g = {k: M[k] for k in GEOMETRY_PLAN}
    for d in ("fwd", "bwd"):
        g[d] = {k: M[d][k] for k in GEOMETRY_DIR}
    return g


LAUNCHES = ("outside_wg", "outside", "thin1", "thin2", "thin4", "thin8", "thin16", "thin32", "combine", "mfma_w128",
            "mfma_leaf_ct1", "mfma_leaf_ct4", "mfma_ct1", "mfma_ct4", "tri16", "tri32", "tri64", "leaf", "use0")


def sn_expected_launches(M, nrhs):
    """the kernels one solve of nrhs right-hand sides enqueues, per sweep, in the shape of _csx.cholsol_sn_launches"""
    nblk = _ceil(nrhs, 64)
    res = {}
    for d in ("fwd", "bwd"):
        L = dict.fromkeys(LAUNCHES, 0)

        def many(tasks, short):
            # lanes per task when the right-hand sides are few and the tasks many and short -- or very many
            if nrhs <= THIN_RHS and tasks >= THIN_TASKS and (short or tasks >= THIN_ANY):
                L["thin%d" % max(1, 1 << (nrhs - 1).bit_length())] += 1
            else:
                L["outside"] += 1

        def triangles(count, leaf):
            if not leaf and count == 1:
                L["use0"] += 1
            if not leaf and M["chunk"] > 64:
                L["mfma_w128"] += 1
            else:               # one wave per 16 right-hand sides while the launch is small, else one per 64
                L[("mfma_leaf_" if leaf else "mfma_") + ("ct1" if count * nblk <= 512 else "ct4")] += 1

        def leaves():
            if M["leaf_subtrees"]:
                if M["matrix_cores"]:
                    triangles(M["leaf_subtrees"], True)
                else:
                    L["leaf"] += 1

        if d == "fwd":
            leaves()
        for st in M[d]["step_list"]:
            if 0 < st["tasks"] <= WG_TASKS:
                L["outside_wg"] += 1
            elif st["tasks"]:
                many(st["tasks"], st["terms"] <= THIN_SHORT * st["tasks"])
            if st["cut"]:
                L["combine"] += 1
            if M["matrix_cores"]:
                triangles(st["triangles"], False)
            else:
                for k, name in (("narrow", "tri16"), ("medium", "tri32"), ("wide", "tri64")):
                    L[name] += st[k] > 0
        if d == "bwd" and M["leaf_subtrees"]:
            if M["leaf_tasks"]:
                many(M["leaf_tasks"], True)
            if M["leaf_slots"]:
                L["combine"] += 1
            leaves()
        res[d] = L
    return res


# ---- the cases ------------------------------------------------------------------------------------------------------

K_DEFAULT = (1, 33, 64, 128)


class Case:
    """name, the pattern's generator, "tri.supernodes", the batch sizes it is solved at, the edge it is built for (a
    predicate on the model and on `launches(k)`, the expected launches at k right-hand sides), the guard case's bad block"""

    def __init__(self, name, gen, edge, mode=1, ks=K_DEFAULT, bad_block=None, path=4, growth=None):
        self.name, self.gen, self.edge, self.mode, self.ks, self.bad_block, self.path = name, gen, edge, mode, ks, bad_block, path
        # where the guard's measure of the last build tried has to lie: tame without a bad block, past the guard with one
        self.growth = growth or ((0.0, 10.0) if bad_block is None else (GUARD, np.inf))

    def build(self):
        n, Lp, Li = self.gen()
        seed = sum(ord(c) * (k + 1) for k, c in enumerate(self.name))
        return n, Lp, Li, values(n, Lp, Li, seed, self.bad_block)


def _root_chunks(M):
    a = M["supernodes"][-1][0]
    return [w for c, w in M["chunks"] if c >= a]


def _steps(M, d):
    return M[d]["step_list"]


CASES = []


def _add(*a, **k):
    CASES.append(Case(*a, **k))


# chunks of 128 on the matrix cores: 1, 1, 2, 2, 3 chunks, the last of one column
for wr, want in ((127, [127]), (128, [128]), (129, [128, 1]), (256, [128, 128]), (257, [128, 128, 1])):
    _add("root%d" % wr, lambda wr=wr: comb(4, 64, 8, wr, reach=4, root_reach=100),
         lambda M, la, want=want: M["chunk"] == 128 and _root_chunks(M) == want and la(1)["fwd"]["mfma_w128"] == 1 + len(want)
         and la(1)["bwd"]["mfma_w128"] == 1 + len(want))
# chunks of 64 by substitution: the narrow / medium / wide lists and a last chunk of one
for wr, want in ((15, [15]), (16, [16]), (17, [17]), (32, [32]), (33, [33]), (63, [63]), (64, [64]), (65, [64, 1]), (129, [64, 64, 1])):
    cls = lambda w: "tri16" if w <= 16 else "tri32" if w <= 32 else "tri64"
    _add("sub_root%d" % wr, lambda wr=wr: comb(4, 64, 8, wr, reach=4, root_reach=min(wr - 1, 40)),
         lambda M, la, want=want, cls=cls: M["chunk"] == 64 and not M["matrix_cores"] and _root_chunks(M) == want
         and all(la(1)[d][cls(w)] >= 1 for w in want for d in ("fwd", "bwd")) and la(1)["fwd"]["leaf"] == 1
         and la(1)["fwd"]["tri16"] == 1 + sum(w <= 16 for w in want), mode=2)
# cut lines.  A supernode row with 512 outside terms (whole) and one with 513 (256 + 256 + 1) beside a whole one of 512
_add("fwd512", lambda: comb(2, 64, 8, 64, reach=[64] * 8, leaves=8, leaf_root_reach=0),
     lambda M, la: M["fwd"]["cut_lines"] == 0 and _steps(M, "fwd")[0]["max_uncut"] == 512 and la(1)["fwd"]["combine"] == 0)
_add("fwd513", lambda: comb(2, 64, 8, 64, reach=[64] * 7 + [63, 1], reach0=[64] * 8 + [1], leaves=9, leaf_root_reach=0),
     lambda M, la: _steps(M, "fwd")[0]["cut"] == [[256, 256, 1]] * 8 and _steps(M, "fwd")[0]["max_uncut"] == 512
     and M["fwd"]["cut_lines"] == 8 and la(1)["fwd"]["combine"] == 1)
# a supernode column with 512 and with 513 rows below its supernode
_add("bwd512", lambda: comb(4, 64, 8, 520, reach=2, root_reach=512, leaf_root_reach=0),
     lambda M, la: M["bwd"]["cut_lines"] == 0 and _steps(M, "bwd")[-1]["max_uncut"] == 512 and la(1)["bwd"]["combine"] == 0)
_add("bwd513", lambda: comb(4, 64, 8, 520, reach=2, root_reach=513, leaf_root_reach=0),
     lambda M, la: _steps(M, "bwd")[-1]["cut"] == [[256, 256, 1]] * 32 and la(1)["bwd"]["combine"] == 1)
# a leaf column with 256 and with 257 rows outside its subtree: the leaf rule cuts past SN_SEG
_add("leaf256", lambda: comb(3, 64, 128, 136, reach=3, root_reach=129, leaf_root_reach=128),
     lambda M, la: M["leaf_tasks"] == 9 and M["leaf_slots"] == 0 and la(1)["bwd"]["combine"] == 0)
_add("leaf257", lambda: comb(3, 64, 128, 136, reach=3, root_reach=129, leaf_root_reach=129),
     lambda M, la: M["leaf_tasks"] == 18 and M["leaf_slots"] == 18 and la(1)["bwd"]["combine"] == 1)
# leaf subtrees of 64 and of 65 columns (the 65th column joins the supernode above); cliques here, chains in the other cases
_add("leaf64", lambda: comb(4, 64, 8, 64, reach=3, dense_leaf=True),
     lambda M, la: M["leaf_sizes"] == [64] * 4 and M["supernodes"][0][1] == 8)
_add("leaf65", lambda: comb(4, 65, 8, 64, reach=3, dense_leaf=True),
     lambda M, la: M["leaf_sizes"] == [64] * 4 and M["supernodes"][0][1] == 9)
# twigs of 8 and of 7 columns: leaves in both modes / only where relaxed supernodes are not there to take them
for mode in (1, 2):
    _add("twig8_mode%d" % mode, lambda: comb(4, 8, 8, 64, reach=2, leaves=9),
         lambda M, la: M["leaf_sizes"] == [8] * 36, mode=mode)
_add("twig7_mode1_no_leaf", lambda: comb(4, 7, 8, 64, reach=2, leaves=10),
     lambda M, la: M["leaf_subtrees"] == 0 and M["has_relaxed"] == 1 and la(1)["bwd"]["mfma_leaf_ct1"] == 0)
_add("twig7_mode2", lambda: comb(4, 7, 8, 64, reach=2, leaves=10),
     lambda M, la: M["leaf_sizes"] == [7] * 40 and la(1)["bwd"]["leaf"] == 1, mode=2)
# every column but the root supernode's in a leaf subtree
_add("all_leaf", lambda: comb(5, 64, 0, 64, reach=5, root_reach=7),
     lambda M, la: M["leaf_cols"] == 320 and len(M["supernodes"]) == 1 and M["fwd"]["steps"] == 1)
# leaf triangles per launch: a wave per 16 right-hand sides up to 512 (subtrees x blocks of 64), one per 64 beyond
for nl, ks in ((512, (1, 64, 128)), (513, (1, 64, 128)), (256, (64, 128)), (257, (64, 128))):
    _add("leaves%d" % nl, lambda nl=nl: comb(nl, 8, 0, 64, reach=1, root_reach=1),
         lambda M, la, nl=nl: M["leaf_subtrees"] == nl and all(
             la(k)[d]["mfma_leaf_ct1"] == (nl * -(-k // 64) <= 512) and la(k)[d]["mfma_leaf_ct4"] == (nl * -(-k // 64) > 512)
             for k in (64, 128) for d in ("fwd", "bwd")), ks=ks)
# step size: 16384 tasks (2048 supernodes of 8 columns, one outside term per row) take a workgroup each; 16385 (3277
# supernodes of 5) go by waves, or by lanes when the right-hand sides are few and the tasks short -- or 50000 and more
K_THIN = (1, 2, 3, 5, 9, 17, 32, 33)
THIN_R = (1, 2, 4, 8, 16, 32, 32)


def _thin(L):
    return [L["thin%d" % r] for r in (1, 2, 4, 8, 16, 32)]


_add("step16384", lambda: comb(2048, 64, 8, 64, reach=1, root_reach=1, leaf_root_reach=0, spread=True),
     lambda M, la: M["fwd"]["max_step_tasks"] == 16384 == M["bwd"]["max_step_tasks"]
     and all(la(k)["fwd"]["outside_wg"] == 2 and la(k)["fwd"]["outside"] + sum(_thin(la(k)["fwd"])) == 0 for k in K_THIN)
     and all(la(k)["bwd"]["outside_wg"] == 1 and la(k)["bwd"]["outside"] == 1 for k in K_THIN), ks=K_THIN)
_add("step16385", lambda: comb(3277, 64, 5, 64, reach=1, root_reach=1, leaf_root_reach=0, spread=True),
     lambda M, la: M["fwd"]["max_step_tasks"] == 16385 == M["bwd"]["max_step_tasks"]
     and all(la(k)[d]["thin%d" % r] == 1 and la(k)[d]["outside"] == (d == "bwd") for k, r in zip(K_THIN, THIN_R) for d in ("fwd", "bwd"))
     and la(33)["fwd"]["outside"] == 1 and sum(_thin(la(33)["fwd"])) == 0, ks=K_THIN)
_add("step16385_long", lambda: comb(3277, 64, 5, 64, reach=49, root_reach=1, leaf_root_reach=0, spread=True),
     lambda M, la: _steps(M, "fwd")[0]["tasks"] == 16385 and _steps(M, "fwd")[0]["terms"] == 49 * 16385
     and la(32)["fwd"]["outside"] == 1 and la(32)["fwd"]["thin32"] == 0
     and la(32)["bwd"]["thin32"] == 2 and M["leaf_tasks"] >= THIN_TASKS, ks=(1, 32, 33))
# (3.3e6 entries, the one case above the 1.5e6 the others stay under: 50000 tasks of 49 terms are 2.45e6 entries of L by
# themselves, each in a reaching leaf column that also carries the supernode's other rows)
_add("step50000_long", lambda: comb(3125, 64, 16, 64, reach=49, root_reach=1, leaf_root_reach=0, spread=True),
     lambda M, la: _steps(M, "fwd")[0]["tasks"] == 50000 and _steps(M, "fwd")[0]["terms"] == 49 * 50000
     and la(32)["fwd"]["thin32"] == 1 and la(1)["fwd"]["thin1"] == 1 and la(33)["fwd"]["outside"] == 1, ks=(1, 32, 33))
for lt in (8191, 8192):
    _add("leaf_tasks%d" % lt, lambda lt=lt: comb(1024, 8, 0, 64, reach=8, root_reach=1, reach0=7 if lt == 8191 else None),
         lambda M, la, lt=lt: M["leaf_tasks"] == lt and la(32)["bwd"]["thin32"] == (lt >= 8192) and la(32)["bwd"]["outside"] == (lt < 8192)
         and la(33)["bwd"]["outside"] == 1, ks=(1, 32, 33))
# a step of one triangle takes its descriptor with the launch, a step of two reads the list
_add("two_on_a_level", lambda: comb(2, 64, 8, 64, reach=3, leaves=2),
     lambda M, la: [s["triangles"] for s in _steps(M, "fwd")] == [2, 1] and la(1)["fwd"]["use0"] == 1 == la(1)["bwd"]["use0"])
_add("one_on_every_level", lambda: comb(1, 64, 8, 64, reach=3, leaves=4),
     lambda M, la: [s["triangles"] for s in _steps(M, "fwd")] == [1, 1] and la(1)["fwd"]["use0"] == 2 == la(1)["bwd"]["use0"])
# relaxed runs: a banded chain of 128 k + 1 columns after its leaf subtree -- full runs and a trailing single column
for k in (2, 3):
    _add("band_128x%d+1" % k, lambda k=k: band_chain(64 + 128 * k + 1, 5 + k),
         lambda M, la, k=k: [s[1:] for s in M["supernodes"]] == [(128, "relaxed")] * k + [(1, "fundamental")]
         and M["leaf_sizes"] == [64] and M["chunk"] == 128)
# a fundamental run inside a chain: 31 columns are absorbed by a range, 32 stay a fundamental supernode
_add("frun31", lambda: band_chain(64 + 400, 11, dense_at=64 + 150, dense_w=31),
     lambda M, la: [s for s in M["supernodes"] if s[0] <= 64 + 150 < s[0] + s[1]] == [(64 + 128, 128, "relaxed")]
     and M["fundamental"] == 0)
_add("frun32", lambda: band_chain(64 + 400, 11, dense_at=64 + 150, dense_w=32),
     lambda M, la: (64 + 150, 32, "fundamental") in M["supernodes"] and M["has_relaxed"] == 1)
# the growth guard: one bad block.  Fundamental supernodes only (runs of 32 columns and more are never taken by a range):
# chunks of 64 by substitution.  With relaxed ones: no plan.
_add("guard_fundamental", lambda: comb(4, 64, 32, 129, reach=4, root_reach=3),
     lambda M, la: M["chunk"] == 64 and M["matrix_cores"] == 0 and M["has_relaxed"] == 0 and la(1)["fwd"]["tri64"] == 2
     and la(1)["fwd"]["leaf"] == 1, bad_block=4 * 96 + 32)
_add("guard_relaxed", lambda: band_chain(64 + 400, 11, dense_at=64 + 150, dense_w=32),
     lambda M, la: M is None, bad_block=64 + 150 + 16, path=0)
# the guard asked twice: a bad block that is one diagonal block of a 128-column range (refused) but straddles two blocks of
# the 64-column ranges, which a twig has shifted (its parent lies 30 columns on: the first range of at most 64 ends before
# it, the range of 128 takes both; the ranges start at the last column of the root supernode below the chain).  The plan has chunks of 64 AND the matrix cores: k_sn_mfma<., false, 1 | 4, 4>,
# one wave per 16 right-hand sides up to 512 (triangles x blocks of 64) and one per 64 beyond -- 257 supernodes on a level.
SHIFTED_BELOW = 257 * 72 + 40
_add("guard_chunk64_cores",
     lambda: stack(comb(257, 64, 8, 40, reach=2, root_reach=3), band_chain(300, 13, dense_at=143, dense_w=16, twig=(40, 70))),
     lambda M, la: M["chunk"] == 64 and M["matrix_cores"] == 1 and M["has_relaxed"] == 1 and M["growth"][128] > GUARD
     and [s[:2] for s in M["supernodes"][-6:-1]] == [(SHIFTED_BELOW + a, w) for a, w in ((-1, 41), (40, 64), (104, 64), (168, 64), (232, 64))]
     and all(la(64)[d]["mfma_ct1"] == M[d]["steps"] and la(64)[d]["mfma_ct4"] == 0 for d in ("fwd", "bwd"))
     and all(la(128)[d]["mfma_ct4"] == 1 and la(128)[d]["mfma_ct1"] == M[d]["steps"] - 1 for d in ("fwd", "bwd")),
     ks=(1, 64, 128), bad_block=SHIFTED_BELOW + 143, growth=(10.0, GUARD))
# right-hand-side tails: column tiles of 16 (tiles = min(4, ceil(k / 16))) and blocks of 64
_add("rhs_tails", lambda: comb(4, 64, 24, 140, reach=5, root_reach=20),
     lambda M, la: M["chunk"] == 128 and _root_chunks(M) == [128, 12], ks=(1, 15, 16, 17, 48, 49, 63, 64, 65, 127, 128, 129))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def built(name):
    """(n, Lp, Li, Lx, guard measure of the last build tried, model, launches(k)) of a case, made once per process and
    left unchanged"""
    c = BY_NAME[name]
    n, Lp, Li, Lx = c.build()
    for a in (Lp, Li, Lx):
        a.setflags(write=False)
    tried = []

    def guard(M):
        tried.append(guard_measure(n, Lp, Li, Lx, M))
        return tried[-1]

    M = sn_model(n, Lp, Li, c.mode, guard)
    if not tried:       # (mode 2 builds no fragments: the measure of the blocks all the same, for the CPU test)
        tried.append(guard_measure(n, Lp, Li, Lx, M))
    growth = tried[-1]
    launches = functools.lru_cache(maxsize=None)(lambda k: sn_expected_launches(M, k))
    return n, Lp, Li, Lx, growth, M, launches
