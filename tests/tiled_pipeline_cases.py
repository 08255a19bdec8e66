"""Inputs for the pipelined step and the bulk tile copy of the tiled cs_gaxpy kernel (csx_gaxpy_tiled.hip), built with the
helpers of tests/tiled_cases.py and of its two value classes: every sum has one right answer in any order.  Pure numpy:
tests/test_tiled_pipeline_cases_cpu.py checks the constructions, tests/test_gpu_gaxpy_tiled_pipeline.py runs them.

What the kernel does that these cases aim at:

    the walk   a wave takes NG groups per step (g, g + NW, ...).  Keys and values of a step are loaded one step ahead into
               two key sets and two value sets named by the step number modulo 2 (the ablation build can run the keys two
               steps ahead in a ring of three, named modulo 6: the ladder reaches 7 steps for its wrap).  A step whose NG
               groups all exist takes a body without tests; a row block's last step, when it is short, a predicated one that
               loads nothing.  The loads ahead are clamped to the row block's last group.
    the tile   the rows of a row block move between y and LDS as 16-byte pairs from the first 16-byte-aligned row on, in
               batches of eight pairs per thread, a row before the pairs and a row after them singly.

    ring_ladder(cus, shape)     row blocks whose waves run 1 .. 7 steps (the six phases of the ring and its wrap to phase 0),
                                the last step full, one group per wave short, and of one group of one entry
    two_rounds_restart(cus)     two row blocks per workgroup; empty first blocks, empty second blocks, both; walks of 2 - 3 steps
    tile_rows(cus, R, ...)      row blocks of R rows, entries in some rows only, y0 distinct and non-zero in every row
    SPECIALS                    bit patterns a pure copy must keep: -0.0 and NaNs with payloads
"""
import numpy as np

import tiled_cases as TC

STEPS = tuple(range(1, 8))
SPECIALS = np.array([0x8000000000000000, 0x7FF8000000000001, 0xFFF4DEADBEEF0123, 0x7FF0000000000ABC],
                    dtype=np.uint64).view(np.float64)


def ring_groups(shape):
    """[(groups G, entries in the last group)] for walks of k = 1 .. 7 steps at this shape: k NW NG groups (last step full),
    k NW NG - NW (every wave's last step one group short) and (k - 1) NW NG + 1 (a last step of one group of one entry)"""
    NW, NG = TC.SHAPES[shape]
    K = NW * NG
    out = []
    for k in STEPS:
        out += [(k * K, TC.TL_GROUP), (k * K - NW, TC.TL_GROUP), ((k - 1) * K + 1, 1)]
    return out


def ring_blocks(cus, shape):
    """{row block: (G, entries in the last group)}: the ladder over the first row blocks and once more over the last ones, so
    that the plan's very last group ends a row block (the clamp of the loads ahead meets the end of the arrays); every other
    row block has no entry"""
    lad = ring_groups(shape)
    assert cus >= 2 * len(lad)
    blocks = {b: lad[b] for b in range(len(lad))}
    blocks.update({cus - len(lad) + b: lad[b] for b in range(len(lad))})
    return blocks


def ring_ladder(cus, shape):
    """8 rows per row block, one row block per workgroup, one slab, as tiled_cases.group_ladder: each block's columns lie in a
    window of 500 (3-byte keys possible), odd blocks hold a singleton row"""
    rng = np.random.default_rng(8100 + shape)
    m, n = 8 * cus, 4096
    I, J, S = [], [], []
    for b, (G, last) in sorted(ring_blocks(cus, shape).items()):
        c = TC.TL_GROUP * (G - 1) + last
        c0 = (b * 37) % (n - 500)
        window = np.arange(c0, c0 + 500)
        has_single = b % 2 == 1
        ci = c - has_single
        rows = 8 * b + rng.integers(0, 7, ci)
        cols = rng.choice(window[~TC._is_wide_col(window)], ci)
        I.append(rows), J.append(cols), S.append(np.zeros(ci, bool))
        if has_single:
            I.append([8 * b + 7]), J.append([rng.choice(window[TC._is_wide_col(window)])]), S.append([True])
    return TC._finish(rng, m, n, np.concatenate(I), np.concatenate(J), np.concatenate(S))


def restart_empty_blocks(cus):
    """row blocks without entries in two_rounds_restart: a first block, a second block, and both blocks of one workgroup"""
    return (5, cus + 7, 9, cus + 9)


def two_rounds_restart(cus):
    """m = cus * TL_LDS_ROWS + 1: every workgroup walks two row blocks.  The first eight workgroups' blocks hold 40 - 42 groups
    (walks of 2 - 3 steps at 4 x 5), the others 2 - 3 groups (some waves without a group).  Columns spread evenly over the
    tile (narrow runs: 3-byte keys), the class follows the column as in tiled_cases.lds_edges."""
    rng = np.random.default_rng(8200)
    m, n = cus * TC.TL_LDS_ROWS + 1, 1000
    g = TC.geometry(m, n, cus)
    rb, nrb = g["row_block"], g["nrb"]
    I, J, S = [], [], []
    for b in range(nrb):
        nrows = min(rb, m - b * rb)
        if b in restart_empty_blocks(cus):
            continue
        cnt = TC.TL_GROUP * (40 + b % 3) - 5 if b % cus < 8 else 300 + (b * 7) % 300
        cols = (np.arange(cnt) * n) // cnt
        single = TC._is_wide_col(cols)
        rows = np.empty(cnt, np.int64)
        rows[~single] = 2 * rng.integers(0, (nrows + 1) // 2, int((~single).sum()))
        rows[single] = rng.choice(np.arange(1, nrows - 2, 2), int(single.sum()), replace=False)
        I.append(b * rb + rows), J.append(cols), S.append(single)
    return TC._finish(rng, m, n, np.concatenate(I), np.concatenate(J), np.concatenate(S))


def tile_rows_m(cus, R, last_one=False):
    """m for row blocks of R rows on `cus` workgroups: the last block one row short (R >= 2), or of ONE row (last_one)"""
    if last_one:
        assert 2 <= R <= cus
        return R * (cus - 1) + 1
    return R * cus - 1 if R >= 2 else cus


def tile_rows(cus, R, last_one=False, every=1):
    """Row blocks of R rows (one per workgroup, one slab of 512 columns).  Entries -- up to 40 per block -- in the local rows
    that are multiples of 3, and in a block's last row for even blocks; not in its first row for odd blocks; a singleton in
    local row 1 of every fourth block.  Every other row is empty.  Only blocks with b % every == 0 hold entries at all.
    y0 is replaced: row i of the integer class starts at i + 1, distinct and non-zero (sums stay integers below 2^53 in any
    order), so a row that lands in another row's slot, or is dropped where the pairs begin or end, shows."""
    rng = np.random.default_rng(8300 + 7 * R + last_one + 100 * every)
    m, n = tile_rows_m(cus, R, last_one), 512
    g = TC.geometry(m, n, cus)
    assert g["row_block"] == R and g["rounds"] == 1
    allcols = np.arange(n)
    intcols, widecols = allcols[~TC._is_wide_col(allcols)], allcols[TC._is_wide_col(allcols)]
    I, J, S = [], [], []
    for b in range(g["nrb"]):
        if b % every:
            continue
        nrows = min(R, m - b * R)
        cand = set(range(0, nrows, 3))
        if b % 2 == 0:
            cand.add(nrows - 1)
        else:
            cand.discard(0)
        cand = np.array(sorted(cand), np.int64)
        if cand.size:
            cnt = int(min(40, 4 * cand.size))
            rows = np.concatenate([cand[[0, -1]], rng.choice(cand, cnt - 2)])       # the first and the last of them for sure
            I.append(b * R + rows), J.append(rng.choice(intcols, cnt)), S.append(np.zeros(cnt, bool))
        if b % 4 == 1 and nrows >= 3:
            I.append([b * R + 1]), J.append([rng.choice(widecols)]), S.append([True])
    cat = (lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt))
    m, n, Ap, Ai, Ax, x, y0 = TC._finish(rng, m, n, cat(I, np.int64), cat(J, np.int64), cat(S, bool))
    ints = y0 == np.rint(y0)
    y0 = np.where(ints, np.arange(1, m + 1, dtype=np.float64), y0)
    y0.setflags(write=False)
    return (m, n, Ap, Ai, Ax, x, y0)


UNTOUCHED_R, UNTOUCHED_EVERY = 257, 3


def untouched_tiles(cus):
    """(case, rows): row blocks of 257 rows of which only every third holds entries; `rows` lie in blocks without entries --
    block 1 (its first row is odd in y) and block 2 (even) -- at the first, second, middle and last row of the block: where
    test_gpu_gaxpy_tiled_pipeline puts SPECIALS into y"""
    case = tile_rows(cus, UNTOUCHED_R, every=UNTOUCHED_EVERY)
    R = UNTOUCHED_R
    rows = np.array([b * R + r for b in (1, 2) for r in (0, 1, R // 2, R - 1)], np.int64)
    return case, rows


def with_specials(case, rows):
    """the case with SPECIALS (cycled) in y0 at `rows`"""
    m, n, Ap, Ai, Ax, x, y0 = case
    y0 = y0.copy()
    y0[rows] = np.resize(SPECIALS, rows.size)
    y0.setflags(write=False)
    return (m, n, Ap, Ai, Ax, x, y0)


TILE_ROWS = (1, 2, 3, 255, 256, 257, 4095, 4097)          # 8 * 256 * 2 +- 1: one batch of eight pairs per thread more or less


def batch_edge_rows(shape):
    """row-block lengths one row either side of a full batch of 16-byte pairs at this shape's thread count: eight pairs per
    thread up to 256 threads, four with 512 (tile_batch in csx_gaxpy_tiled.hip)"""
    NW, NG = TC.SHAPES[shape]
    threads = 64 * NW
    per_thread = 4 if threads > 256 else 8
    return (per_thread * threads * 2 - 1, per_thread * threads * 2 + 1)
