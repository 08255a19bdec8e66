"""Inputs for the tiled cs_gaxpy plan (csparse.py_amd/csrc/csx_gaxpy_tiled.hip) whose result has ONE right answer in any
order of summation, and a mirror of the plan's arithmetic so that every construction can be checked without a device.
Pure numpy: the CPU tests check the constructions, the GPU tests run them.

The tiled kernel adds into LDS with atomics, in arrival order.  Two classes of values make the order irrelevant:

    integer    Ax and x nonzero integers in [-8, 8], y0 integers in [-1000, 1000], at most 2^14 terms per row: every partial
               sum in every order is an integer below 2^21, exact in float64.  No y0 is -0.0.
    singleton  a row with exactly one entry; Ax, x and y0 full-mantissa doubles (assemble_oracle.wide).  The result is
               fl(y0 + fl(a x)) in any kernel: a value or an x that lost low bits on the way shows, which small integers
               would let through.

x is shared by a column, so the columns are split too: a column that holds a singleton's entry holds singletons' entries only.
_finish() checks both conditions on every case it returns.

    geometry(m, n, cus)          the arithmetic of gaxpy_tiled_prepare: row_block, nrb, rb_bits, slab_cols, nslab, rounds, LDS bytes
    plan(m, n, cus, Ap, Ai)      ... plus what follows from the entries: groups per row block, key bytes, the largest run offset
    group_ladder, slabs, key_edges, lds_edges, degenerate, density_ladder      the cases; (m, n, Ap, Ai, Ax, x, y0)
"""
import numpy as np

from assemble_oracle import wide

TL_GROUP = 256
TL_LDS_BYTES = 160 * 1024 - 256
TL_LDS_ROWS = TL_LDS_BYTES // 8 - 2          # 20446
SLAB_COLS = 131072                            # 1 MiB of x
SHAPES = ((4, 5), (2, 10), (8, 4), (2, 8))    # (waves per workgroup NW, groups per wave and step NG) of "gaxpy.shape" 0..3
NONZERO = np.array([v for v in range(-8, 9) if v != 0], dtype=np.float64)


def geometry(m, n, cus):
    nwg = cus if cus > 0 else 256
    tries = 1
    while True:
        row_block = (m + nwg * tries - 1) // (nwg * tries)
        if row_block <= TL_LDS_ROWS:
            break
        tries += 1
    row_block = max(row_block, 1)
    nrb = (m + row_block - 1) // row_block
    rb_bits = 1
    while (1 << rb_bits) <= row_block:
        rb_bits += 1
    slab_cols = min(SLAB_COLS, 1 << (32 - rb_bits))
    if slab_cols > n:
        slab_cols = n if n > 0 else 1
    nslab = max(1, (n + slab_cols - 1) // slab_cols)
    grid = min(nrb, nwg)
    return {"row_block": row_block, "nrb": nrb, "rb_bits": rb_bits, "slab_cols": slab_cols, "nslab": nslab, "grid": grid,
            "rounds": (nrb + grid - 1) // grid if grid else 0,               # passes of the kernel's row-block loop
            "lds_bytes": ((row_block + 1) * 8 + 15) & ~15}


def plan(m, n, cus, Ap, Ai):
    """geometry() and what the entries add: tile_counts[nrb, nslab], groups[nrb] (groups of 256 per row block, every tile padded
    by itself), ngroups, key_bytes (3 when no run of 64 column-sorted entries of a tile is 512 columns wide or wider -- the
    decision with "gaxpy.keys24" = 1), max_offset (the largest column offset inside a run) and saturated (an entry in the
    last local row the LDS tile can hold, at run offset 511: the 24-bit key with every offset bit set)."""
    g = geometry(m, n, cus)
    Ap, Ai = np.asarray(Ap, np.int64), np.asarray(Ai, np.int64)
    nnz = int(Ap[-1])
    col = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    b, s = Ai // g["row_block"], col // g["slab_cols"]
    tile = b * g["nslab"] + s
    ntiles = g["nrb"] * g["nslab"]
    counts = np.bincount(tile, minlength=ntiles).astype(np.int64)
    order = np.argsort(tile, kind="stable")                     # column order (the CSC order) kept inside a tile
    st, lc, lr = tile[order], (col - s * g["slab_cols"])[order], (Ai - b * g["row_block"])[order]
    e = np.arange(nnz, dtype=np.int64) - (np.cumsum(counts) - counts)[st]
    off = lc - lc[np.arange(nnz, dtype=np.int64) - (e & 63)]
    per_tile = (counts + TL_GROUP - 1) // TL_GROUP
    g["tile_counts"] = counts.reshape(g["nrb"], g["nslab"])
    g["groups"] = per_tile.reshape(g["nrb"], g["nslab"]).sum(axis=1)
    g["ngroups"] = int(per_tile.sum())
    g["max_offset"] = int(off.max()) if nnz else 0
    g["key_bytes"] = 3 if (g["ngroups"] > 0 and g["rb_bits"] <= 15 and g["max_offset"] < 512) else 4
    g["saturated"] = bool(np.any((off == 511) & (lr == TL_LDS_ROWS - 1)))
    return g


def _finish(rng, m, n, I, J, single, x_int=None):
    """CSC arrays and vectors of the entries (I[k], J[k]), single[k] = the entry of a singleton row.  Entries are shuffled and
    then sorted by column alone: rows are unsorted inside a column, duplicates stay."""
    I, J, single = np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(single, bool)
    assert I.shape == J.shape == single.shape
    if I.size:
        assert 0 <= I.min() and I.max() < m and 0 <= J.min() and J.max() < n
    perm = rng.permutation(I.size)
    perm = perm[np.argsort(J[perm], kind="stable")]
    I, J, single = I[perm], J[perm], single[perm]
    srows, scols = I[single], J[single]
    assert np.unique(srows).size == srows.size and not np.isin(I[~single], srows).any()    # one entry per singleton row
    assert not np.isin(J[~single], scols).any()                                          # their columns hold nothing else
    assert I.size == 0 or np.bincount(I).max() <= 1 << 14
    Ax = rng.choice(NONZERO, I.size)
    Ax[single] = wide(rng, int(single.sum()))
    x = rng.choice(NONZERO, n) if x_int is None else np.array(x_int, dtype=np.float64)
    x[scols] = wide(rng, scols.size)
    y0 = rng.integers(-1000, 1001, m).astype(np.float64)        # integers from +0.0: no -0.0
    y0[srows] = wide(rng, srows.size)
    Ap = np.concatenate([[0], np.cumsum(np.bincount(J, minlength=n))]).astype(np.int32)
    out = (int(m), int(n), Ap, I.astype(np.int32), Ax, x, y0)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def is_integer_row(case):
    """mask of the rows of the integer class (rows without entries included)"""
    m, n, Ap, Ai, Ax, x, y0 = case
    return y0 == np.rint(y0)


def _is_wide_col(j):
    return j % 16 == 5


def ladder_groups(cus, shape):
    """(G_b, r_b) of group_ladder: row block b holds 256 G_b - r_b entries"""
    NW, NG = SHAPES[shape]
    K = NW * NG
    ladder = (0, 1, 2, NW - 1, NW, NW + 1, K - 1, K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1)
    short = (0, 1, 255)          # the last group full, one entry short, a single entry
    return [(ladder[b % 12], short[(b // 12) % 3]) for b in range(cus)]


def group_ladder(cus, shape):
    """8 rows per row block, one row block per workgroup, one slab; the groups per row block walk round the edges of the
    shape's wave count NW and step NW NG.  Each block's columns lie in a window of 500, so the plan may take 3-byte keys."""
    rng = np.random.default_rng(7100 + shape)
    m, n = 8 * cus, 4096
    I, J, S = [], [], []
    for b, (G, r) in enumerate(ladder_groups(cus, shape)):
        c = max(TL_GROUP * G - r, 0)
        if c == 0:
            continue
        c0 = (b * 37) % (n - 500)
        window = np.arange(c0, c0 + 500)
        has_single = b % 2 == 1
        ci = c - has_single
        rows = 8 * b + rng.integers(0, 7, ci)
        cols = rng.choice(window[~_is_wide_col(window)], ci)
        if ci >= 3:
            rows[1], cols[1] = rows[0], cols[0]           # a duplicate of one (i, j)
        I.append(rows), J.append(cols), S.append(np.zeros(ci, bool))
        if has_single:
            I.append([8 * b + 7]), J.append([rng.choice(window[_is_wide_col(window)])]), S.append([True])
    return _finish(rng, m, n, np.concatenate(I), np.concatenate(J), np.concatenate(S))


def _pick_x_differing(rng, n, slab_cols):
    """integer x whose values differ between the slabs at equal offsets inside the slab"""
    k = rng.integers(0, 16, n)
    for s in range(1, (n + slab_cols - 1) // slab_cols):
        lo, hi = s * slab_cols, min((s + 1) * slab_cols, n)
        k[lo:hi] = (k[lo - slab_cols:hi - slab_cols] + 1 + rng.integers(0, 7, hi - lo)) % 16    # +1..+7 twice is never 0 mod 16
    return NONZERO[k]


def slabs(cus):
    """Three column slabs (the last of 5 columns), 4 rows per row block and a last row block of one row.  Every row block has
    entries in all three slabs, in the first and the last column of each, and no tile's count is a multiple of 256.  A tile's
    entries sit in two windows of 500 columns at the ends of the slab, the first holding a multiple of 64 entries: no run of
    64 reaches from one window into the other, so 3-byte keys stay possible."""
    rng = np.random.default_rng(7200)
    m, n = 3 * cus + 1, 2 * SLAB_COLS + 5
    g = geometry(m, n, cus)
    rb, sc = g["row_block"], g["slab_cols"]
    I, J, S = [], [], []
    for b in range(g["nrb"]):
        nrows = min(rb, m - b * rb)
        int_rows = np.arange(b * rb, b * rb + (nrows - 1 if nrows > 1 else 1))
        single_slab = (b // 3) % 3 if (b % 3 == 0 and nrows == rb) else -1
        counts = [70 + (b * 37) % 400, 257 + (b * 53) % 300, 259 + b % 7 if b % 5 == 0 else 3 + (b * 5) % 11]
        for s in range(3):
            cnt = counts[s] + (counts[s] % TL_GROUP == 0)
            if s < 2:
                low = 64 * int(rng.integers(1, (cnt - 1) // 64 + 1))
                lo_win, hi_win = np.arange(s * sc, s * sc + 500), np.arange((s + 1) * sc - 500, (s + 1) * sc)
                cols = np.concatenate([[s * sc], rng.choice(lo_win[~_is_wide_col(lo_win)], low - 1),
                                       [(s + 1) * sc - 1], rng.choice(hi_win[~_is_wide_col(hi_win)], cnt - low - 1)])
                wide_col = rng.choice(lo_win[_is_wide_col(lo_win)])
            else:
                cols = np.concatenate([[s * sc, s * sc + 4], s * sc + rng.choice([0, 1, 3, 4], cnt - 2)])
                wide_col = s * sc + 2
            rows = rng.choice(int_rows, cnt)
            single = np.zeros(cnt, bool)
            if s == single_slab:
                k = 1 if s < 2 else 2                     # one of the first window's entries; not a first or last column
                rows[k], cols[k], single[k] = b * rb + rb - 1, wide_col, True
            I.append(rows), J.append(cols), S.append(single)
    return _finish(rng, m, n, np.concatenate(I), np.concatenate(J), np.concatenate(S), _pick_x_differing(rng, n, sc))


def key_edges(cus):
    """[(label, key bytes the plan must pick with "gaxpy.keys24" = 1, case)]: one tile each (row block 1 of 4 rows, one slab)"""
    m, n = 4 * cus, 1024
    out = []
    for label, cols, kb in (("run_511_wide", list(range(63)) + [511], 3), ("run_512_wide", list(range(63)) + [512], 4),
                            ("two_narrow_runs", list(range(64)) + list(range(600, 664)), 3)):
        rng = np.random.default_rng(7300 + len(out))
        cols = np.asarray(cols)
        rows = 4 + rng.integers(0, 3, cols.size)
        single = np.zeros(cols.size, bool)
        rows[-1], single[-1] = 7, True                 # the last column of the tile: the widest offset of its run
        out.append((label, kb, _finish(rng, m, n, rows, cols, single)))
    return out


def lds_edges(cus, two_rounds):
    """two_rounds False: m = cus * 20446, the largest LDS tile, one row block per workgroup.  Row block 1 opens with a run of
    64 whose last entry is 511 columns from its first and sits in local row 20445: the 24-bit key with all bits of the offset
    set at the largest row.  Entries in the first and the last row of the first and the last row block.
    two_rounds True: one row more, so every workgroup walks two row blocks, of different lengths; row block 3 is empty and
    row block 3 + cus is not.
    Columns are spread evenly over a tile, so every run of 64 is narrow (3-byte keys); the class follows the column."""
    rng = np.random.default_rng(7400 + two_rounds)
    m, n = cus * TL_LDS_ROWS + (1 if two_rounds else 0), 1000
    g = geometry(m, n, cus)
    rb, nrb = g["row_block"], g["nrb"]
    I, J, S = [], [], []
    for b in range(nrb):
        nrows = min(rb, m - b * rb)
        if two_rounds:
            cnt = 0 if b == 3 else (600 + (b * 13) % 400 if b < cus else 200 + (b * 7) % 200)
        else:
            cnt = 700 + (b * 13) % 500
        if cnt == 0:
            continue
        e = np.arange(cnt)
        if not two_rounds and b == 1:
            head = np.arange(102, 200)
            head = head[~_is_wide_col(head)][:63]                                   # 63 integer entries from column 102 ...
            cols = np.concatenate([head, [613], 614 + (e[:cnt - 64] * 386) // (cnt - 64)])   # ... and column 102 + 511
        else:
            cols = (e * n) // cnt
        single = _is_wide_col(cols)
        rows = np.empty(cnt, np.int64)
        rows[~single] = 2 * rng.integers(0, (nrows + 1) // 2, int((~single).sum()))
        odd = np.arange(1, nrows - 2, 2)
        rows[single] = rng.choice(odd, int(single.sum()), replace=False)
        forced = []
        if b in (0, nrb - 1):
            forced += [0, nrows - 1]
        if not two_rounds and b == 1:
            rows[63] = rb - 1                                                       # column 613 is a singleton's (613 % 16 == 5)
            assert single[63] and (rb - 1) % 2 == 1
        for t, r in enumerate(forced):
            rows[np.flatnonzero(single if r % 2 else ~single)[-1 - t]] = r
        I.append(b * rb + rows), J.append(cols), S.append(single)
    return _finish(rng, m, n, np.concatenate(I), np.concatenate(J), np.concatenate(S))


def degenerate(cus):
    """[(label, case)]"""
    out = []

    def add(label, m, n, I, J, single):
        rng = np.random.default_rng(7500 + len(out))
        out.append((label, _finish(rng, m, n, I, J, single)))

    rng = np.random.default_rng(7599)
    add("no_entries", 5, 7, [], [], [])
    add("one_by_one", 1, 1, [0], [0], [True])
    # fewer rows than workgroups: row blocks of one row
    m, n = cus // 2 + 1, 300
    cnt = 4 * m
    add("m_below_cus", m, n, np.concatenate([rng.integers(0, m - 1, cnt), [m - 1]]),
        np.concatenate([rng.integers(0, n - 1, cnt), [n - 1]]), np.arange(cnt + 1) == cnt)
    # one row more than workgroups: row blocks of two rows, the last of one
    m = cus + 1
    cnt = 3 * m
    add("m_cus_plus_1", m, n, np.concatenate([rng.integers(1, m, cnt), [0]]),
        np.concatenate([rng.integers(1, n, cnt), [0]]), np.arange(cnt + 1) == cnt)
    # one column: every row with an entry is a singleton
    m = 3 * cus + 2
    rows = np.sort(rng.choice(m, m // 2, replace=False))
    add("one_column", m, 1, rows, np.zeros(rows.size, np.int64), np.ones(rows.size, bool))
    # one row
    n = 700
    cols = np.concatenate([np.arange(n), rng.integers(0, n, 100)])
    add("one_row", 1, n, np.zeros(cols.size, np.int64), cols, np.zeros(cols.size, bool))
    # entries in the last row block only
    m, n = 4 * cus, 64
    cnt = 300
    add("last_row_block_only", m, n, np.concatenate([m - 4 + rng.integers(0, 3, cnt), [m - 1]]),
        np.concatenate([rng.integers(0, n - 1, cnt), [n - 1]]), np.arange(cnt + 1) == cnt)
    return out


DENSITIES = (3, 6, 7, 12, 13, 24, 25, 48, 49)


def density_ladder(avg):
    """515 rows of avg - 2 .. avg + 2 entries, exactly avg on average: the row kernels (GAXPY_WAVE) pick their lane-group width
    from that average, with thresholds at 6, 12, 24 and 48.  Integer class."""
    rng = np.random.default_rng(7600 + avg)
    m, n = 515, 257
    lens = avg + np.tile([-2, 2, -1, 1, 0], m // 5)
    I = np.repeat(np.arange(m), lens)
    assert I.size == avg * m
    return _finish(rng, m, n, I, rng.integers(0, n, I.size), np.zeros(I.size, bool))
