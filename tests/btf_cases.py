"""Constructed inputs for btf_factor's device kernels (csx_btf.hip: k_btf_small, k_btf_rows, k_btf_strip, k_btf_tcols;
csx_refactor.hip: k_refactor; csx_sweep.h: load_terms, apply_terms): one named case on each side of every block-size cut, term
chunk, level mix and refactor group count, built with fixed seeds.  TEST INFRASTRUCTURE, NOT PRODUCT.

Every cut comes from the library (`_csx.btf_limits()`, no device needed), never from a literal.  A case names the facts it must show
(`claims`) and, where its edge has another side, the case across it (`other`) and the fact that differs (`cut`): of ROUTE_FACTS the
two cases differ in that one alone.  tests/test_btf_cases_cpu.py holds the table to its claims without a device and admits every
case by the CPU restatements alone; tests/test_gpu_btf_edges.py runs every case on the device and compares bytes.

A case is a list of diagonal blocks (rows, level, fill: dense, cyclic or `banded k`), highest level first, and coupling entries
F(i, j) with row i in a block of a higher level than column j's block; the whole is permuted by seeded row and column
permutations.  A dense block is strongly connected, a sparse one holds the cycle a -> a + 1 -> ... -> a, and the couplings only go
down the levels: the fine blocks of dmperm are the intended ones.  Unless a case says otherwise the blocks are diagonally dominant
by columns (cs_lu keeps the dominant entries as pivots whatever order the columns come in), and a coupling value in a row or column
of t couplings is scaled by 1 / t.

What no case reaches is listed in NOT_REACHED with the reason."""
import functools

import numpy as np
import scipy.sparse as sp

import _csx

LIM = _csx.btf_limits()
BTF_SMALL, RF_MAX, RF_WAVES, RHS_TILE, TERM_CHUNK, TERM_GROUP = (LIM[k] for k in _csx.BTF_LIMITS)
SMALL, CHUNK, GROUP = BTF_SMALL, TERM_CHUNK, TERM_GROUP

# what the table as a whole must hold (test_btf_cases_cpu.py: test_the_table_covers_every_edge)
BLOCK_SIZES = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, SMALL - 1, SMALL, SMALL + 1)
TERM_COUNTS = (GROUP - 1, GROUP, GROUP + 1, CHUNK - 1, CHUNK, CHUNK + 1)                  # of an L or U program row
F_ROW_COUNTS = (0, 1, GROUP - 1, GROUP, GROUP + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)
F_COL_COUNTS = F_ROW_COUNTS[1:]
RF_GROUP_COUNTS = (1, RF_WAVES - 1, RF_WAVES, RF_WAVES + 1)
WIDTHS = (1, RHS_TILE - 1, RHS_TILE, RHS_TILE + 1, 2 * RHS_TILE + 2)
WIDE_COLUMNS = (0, RHS_TILE - 1, RHS_TILE, RHS_TILE + 1)                                  # and the last, of the widest block
BOUND = 1e-13                                                                             # normwise backward error of every solve

ROUTE_FACTS = ("levels", "large_blocks", "launches", "lu_chunks", "f_chunks", "fc_chunks", "rf_workgroups")

NOT_REACHED = {
    "F programs past 2^31 terms": "Fp is int32 and csx_btf_split refuses nothing of that size before the scan overflows; 2^31 "
                                  "coupling entries are 24 GB of F alone, far past what a test can hold",
    "k_btf_small with nr == 0": "is_blocks refuses r[b + 1] <= r[b], so no block has zero rows and every LDS tile has a row",
    "a refactor group with duplicate rows in a column of D": "btf_factor sums nothing and keeps duplicates, but dmperm_arrays and "
                                                             "the split are out of this table's scope; the lusol duplicate group "
                                                             "is covered by test_lusol_refactor_mixed_groups_with_duplicates",
    "k_refactor with a non-finite pivot in the second pass": "the failing case forces an exact zero pivot; an inf or NaN in A2 "
                                                             "takes the same branch (piv == 0.0 || !isfinite) one operand later",
}


# ---- the model: csx_btf_plan / csx_btf_info / refactor_build restated ---------------------------------------------------------
def plan_model(sizes, levels, fnz):
    """what csx_btf_info must say for blocks of these sizes and levels, and per level (0 first) the small blocks' sizes, the
    largest of them (the LDS rows of the level's launch; 0: no launch) and the large blocks' sizes"""
    sizes, levels = np.asarray(sizes, np.int64), np.asarray(levels, np.int64)
    nlev = int(levels.max()) + 1 if len(levels) else 0
    per = []
    for l in range(nlev):
        s = sizes[levels == l]
        small, large = s[s <= BTF_SMALL], s[s > BTF_SMALL]
        per.append({"small": sorted(small.tolist()), "lds_rows": int(small.max()) if len(small) else 0,
                    "large": sorted(large.tolist())})
    return {"blocks": len(sizes), "levels": nlev, "max_block": int(sizes.max()) if len(sizes) else 0,
            "large_blocks": int((sizes > BTF_SMALL).sum()), "launches": 1 + sum(1 for p in per if p["small"]),
            "fnz": int(fnz), "per_level": per}


def refactor_model(sizes):
    """refactor_build on groups of these sizes (none with duplicate entries): columns and groups on each side, the workgroups of
    k_refactor and the waves of the last one that have a group"""
    sizes = np.asarray(sizes, np.int64)
    dev = sizes[sizes <= RF_MAX]
    g = len(dev)
    wg = -(-g // RF_WAVES)
    return {"device_columns": int(dev.sum()), "host_columns": int(sizes.sum() - dev.sum()), "device_groups": g,
            "host_groups": len(sizes) - g, "rf_workgroups": wg, "rf_last_waves": g - (wg - 1) * RF_WAVES if g else 0}


def arrays(M):
    """(p, i) of a `cs`-like object or of a tuple (p, i, x)"""
    p, i = (M[0], M[1]) if isinstance(M, tuple) else (M.p, M.i)
    p = np.asarray(p, np.int64)
    return p, np.asarray(i[:int(p[-1])], np.int64)


def term_counts(L, U, F, r):
    """terms of every row program from factors (`cs` objects or (p, i, x)) with the block boundaries r: forward L (row of L
    without its diagonal), U, F (row of F); transposed UT (column of U without its diagonal), LT, FC (column of F); `small`: the
    row is in a block that k_btf_small solves"""
    (Lp, Li), (Up, Ui), (Fp, Fi) = arrays(L), arrays(U), arrays(F)
    n = len(Lp) - 1
    r = np.asarray(r, np.int64)
    small = np.repeat(np.diff(r) <= BTF_SMALL, np.diff(r))
    return {"L": np.bincount(Li, minlength=n) - 1, "U": np.bincount(Ui, minlength=n) - 1, "F": np.bincount(Fi, minlength=n),
            "UT": np.diff(Up) - 1, "LT": np.diff(Lp) - 1, "FC": np.diff(Fp), "small": small}


def check_counts(claims, tc):
    """the term counts a case claims occur among the program rows k_btf_small walks: lu_counts in each of L, U, UT and LT,
    f_row_counts in F, f_col_counts in FC"""
    sm = tc["small"]
    for key, progs in (("lu_counts", ("L", "U", "UT", "LT")), ("f_row_counts", ("F",)), ("f_col_counts", ("FC",))):
        for k in progs:
            missing = set(claims.get(key, ())) - set(tc[k][sm].tolist())
            assert not missing, (key, k, sorted(missing))


def chunks(count):
    return int(-(-int(count) // TERM_CHUNK))


def facts(M, tc):
    """every fact a claim or a cut may name: the plan's, the refactor's, and the chunk counts of the longest program rows that
    k_btf_small walks (tc: term_counts of factors of this case)"""
    f = dict(plan_model(M["sizes"], M["levels"], M["fnz"]))
    f.update(refactor_model(M["sizes"]))
    sm = tc["small"]
    top = lambda *keys: max([int(tc[k][sm].max()) if sm.any() else 0 for k in keys])
    f.update(n=M["n"], lu_chunks=chunks(top("L", "U", "UT", "LT")), f_chunks=chunks(top("F")), fc_chunks=chunks(top("FC")),
             lds_rows=tuple(p["lds_rows"] for p in f["per_level"]), min_block=int(np.min(M["sizes"])))
    return f


# ---- builders -----------------------------------------------------------------------------------------------------------------
def _block(rng, m, fill, dominant):
    ix = np.arange(m)
    if fill == "dense":
        D = rng.uniform(0.1, 1.0, (m, m)) * rng.choice([-1.0, 1.0], (m, m))
    else:
        D = np.zeros((m, m))
        if fill.startswith("banded"):
            k = int(fill.split()[1])
            band = np.abs(ix[:, None] - ix[None, :]) <= k
            D[band] = (rng.uniform(0.1, 1.0, (m, m)) * rng.choice([-1.0, 1.0], (m, m)))[band]
        else:
            assert fill == "cyclic", fill
        D[ix, (ix + 1) % m] = rng.uniform(0.3, 1.0, m) * rng.choice([-1.0, 1.0], m)      # the cycle: strongly connected
    D[ix, ix] = 0.0
    D[ix, ix] = np.abs(D).sum(axis=0) + 1.0 + rng.random(m) if dominant else rng.uniform(0.05, 0.2, m) * rng.choice([-1.0, 1.0], m)
    return D


class Layout(object):
    """the blocks of a case in the unpermuted order (highest level first): rows(b) = the indices of block b"""

    def __init__(self, blocks):
        self.sizes = np.asarray([b[0] for b in blocks], np.int64)
        self.levels = np.asarray([b[1] for b in blocks], np.int64)
        assert np.all(np.diff(self.levels) <= 0), "list the blocks highest level first"
        self.starts = np.concatenate([[0], np.cumsum(self.sizes)])
        self.n = int(self.starts[-1])

    def rows(self, b):
        return np.arange(self.starts[b], self.starts[b + 1])

    def of_level(self, l):
        return np.concatenate([self.rows(b) for b in np.flatnonzero(self.levels == l)] or [np.zeros(0, np.int64)])


def build(seed, blocks, couple, tol=1.0, weak=(), widths=(1, RHS_TILE + 1), refactor=None):
    """blocks: (rows, level, fill) highest level first; couple(rng, layout) -> (rows, cols) of the coupling entries in the
    unpermuted order; weak: blocks that are NOT diagonally dominant; refactor: None, "perturb" (entrywise 1e-3) or "singular"."""
    rng = np.random.default_rng(seed)
    lay = Layout(blocks)
    n = lay.n
    bof = np.repeat(np.arange(len(blocks)), lay.sizes)
    rr, cc, vv = [], [], []
    for b, (m, _, fill) in enumerate(blocks):
        D = _block(rng, m, fill, b not in weak)
        c, r = np.nonzero(D.T)
        rr.append(lay.starts[b] + r)
        cc.append(lay.starts[b] + c)
        vv.append(D[r, c])
    fr, fc = (np.asarray(a, np.int64) for a in couple(rng, lay))
    assert len(set(zip(fr.tolist(), fc.tolist()))) == len(fr), "a coupling entry twice"
    assert np.all(lay.levels[bof[fr]] > lay.levels[bof[fc]]), "couplings go down the levels"
    t = np.maximum(np.bincount(fr, minlength=n)[fr], np.bincount(fc, minlength=n)[fc])
    fv = rng.uniform(0.3, 1.0, len(fr)) * rng.choice([-1.0, 1.0], len(fr)) / t
    S0 = sp.csc_matrix((np.concatenate(vv + [fv]), (np.concatenate(rr + [fr]), np.concatenate(cc + [fc]))), shape=(n, n))
    S0.sort_indices()
    pr, pc = rng.permutation(n), rng.permutation(n)
    S = S0[pr][:, pc].tocsc()
    S.sort_indices()
    return {"n": n, "S": S, "S0": S0, "pr": pr, "pc": pc, "sizes": lay.sizes, "levels": lay.levels, "starts": lay.starts,
            "fnz": len(fr), "tol": tol, "widths": tuple(widths), "refactor": refactor, "seed": seed, "layout": lay}


def with_values(S, x):
    return sp.csc_matrix((np.asarray(x, np.float64), S.indices.copy(), S.indptr.copy()), shape=S.shape)


def perturbed(S, seed):
    """new values on S's pattern: every entry scaled by 1 + 1e-3 u: the dominant diagonals stay dominant, the pivots stay"""
    return with_values(S, S.data * (1.0 + 1e-3 * np.random.default_rng(seed).uniform(-1, 1, S.nnz)))


def block_of(M, permuted):
    """the rows and columns of the first block of SMALL rows of the case, as indices of M["S"] (permuted) or of M["S0"]; entry k of
    the two is the block's k-th dominant entry"""
    b = int(np.flatnonzero(M["sizes"] == BTF_SMALL)[0])
    idx = np.arange(M["starts"][b], M["starts"][b + 1])
    if not permuted:
        return idx, idx
    rinv, cinv = np.empty(M["n"], np.int64), np.empty(M["n"], np.int64)
    rinv[M["pr"]], cinv[M["pc"]] = np.arange(M["n"]), np.arange(M["n"])
    return rinv[idx], cinv[idx]                              # S[i, j] = S0[pr[i], pc[j]]


def singular_values(S, rows, cols, last, prev, seed):
    """values on S's pattern that give a zero pivot in the LAST column of the dense SMALL-row block with the pivots kept: the
    block becomes the identity on its dominant entries (rows[k], cols[k]) -- small integers, every operation exact -- but for
    column `last` (an index into cols: the column the factorisation takes last in the block), which is a copy of column `prev`:
    1 in prev's pivot row, 0 in its own.  Everything else is perturbed(S, seed)."""
    m, n = len(rows), S.shape[0]
    B = np.eye(m)
    B[:, last] = B[:, prev]
    x = perturbed(S, seed).data
    row, col = S.indices, np.repeat(np.arange(n), np.diff(S.indptr))
    rl, cl = np.full(n, -1), np.full(n, -1)
    rl[rows], cl[cols] = np.arange(m), np.arange(m)
    inside = (rl[row] >= 0) & (cl[col] >= 0)
    assert inside.sum() == m * m
    x[inside] = B[rl[row[inside]], cl[col[inside]]]
    return with_values(S, x)


def _to_lower(rng, lay, per_block=1):
    """every block of level l > 0 reaches level l - 1: `per_block` entries from seeded rows into seeded columns"""
    fr, fc = [], []
    for b in np.flatnonzero(lay.levels > 0):
        below = lay.of_level(lay.levels[b] - 1)
        k = min(per_block, len(below), lay.sizes[b])
        fr += rng.choice(lay.rows(b), k, replace=False).tolist()
        fc += rng.choice(below, k, replace=False).tolist()
    return fr, fc


# ---- the table ----------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, other=None, cut=None, **claims):
    def deco(fn):
        CASES[name] = {"name": name, "other": other, "cut": cut, "claims": claims, "build": functools.lru_cache(maxsize=None)(fn)}
        return fn
    return deco


def get(name):
    return CASES[name]["build"]()


# block size and route: one dense block of r rows at level 1 over a few small blocks; a dense block of r rows has L program rows of
# 0 .. r - 1 terms and U program rows of r - 1 .. 0 terms
def _size_case(r, seed, widths=(1, RHS_TILE + 1)):
    # (the case over the cut keeps what the one below it has in ROUTE_FACTS: a dense block that needs a second chunk, and as many
    # device groups in a refactor)
    rest = [(5, 0, "cyclic"), (1, 0, "dense")] if r != SMALL + 1 else [(CHUNK + 2, 0, "dense"), (1, 0, "dense"), (1, 0, "dense")]
    return build(seed, [(r, 1, "dense"), (2, 1, "dense")] + rest, lambda rng, lay: _to_lower(rng, lay, 3), widths=widths)


_SIZE_CUTS = {CHUNK + 1: ("size_%d" % (CHUNK + 2), "lu_chunks"), CHUNK + 2: ("size_%d" % (CHUNK + 1), "lu_chunks"),
              SMALL: ("size_%d" % (SMALL + 1), "large_blocks"), SMALL + 1: ("size_%d" % SMALL, "large_blocks")}
for _k, _r in enumerate(BLOCK_SIZES):
    _claims = {"max_block": max(_r, 5), "large_blocks": int(_r > SMALL), "levels": 2, "launches": 3,
               "lu_chunks": chunks(max(_r - 1, 1)) if _r <= SMALL else 2}
    if _r <= SMALL:
        _claims.update(lu_counts=tuple(range(_r)))
    if _r == SMALL:
        _claims.update(device_columns=SMALL + 8, host_columns=0)
    if _r == SMALL + 1:
        _claims.update(host_columns=SMALL + 1, host_groups=1)
    case("size_%d" % _r, *_SIZE_CUTS.get(_r, (None, None)), **_claims)(
        functools.partial(_size_case, _r, 200 + _k, WIDTHS if _r in (SMALL, CHUNK + 2) else (1, RHS_TILE + 1)))


@case("all_small_max", max_block=SMALL, min_block=SMALL, large_blocks=0, levels=2, lu_chunks=2)
def _():
    """every block has SMALL rows: one dense, the others banded"""
    blocks = [(SMALL, 1, "dense"), (SMALL, 1, "banded 6"), (SMALL, 0, "banded 2"), (SMALL, 0, "cyclic")]
    return build(220, blocks, lambda rng, lay: _to_lower(rng, lay, 20), refactor="perturb")


@case("all_ones", max_block=1, min_block=1, blocks=200, levels=3, launches=4, lds_rows=(1, 1, 1))
def _():
    """every block has one row: every level's LDS tile is one row"""
    blocks = [(1, 2, "dense")] * 40 + [(1, 1, "dense")] * 60 + [(1, 0, "dense")] * 100
    return build(221, blocks, lambda rng, lay: _to_lower(rng, lay, 1), widths=WIDTHS, refactor="perturb")


@case("pivoted%d" % SMALL, max_block=SMALL, large_blocks=0, pivots_move=True)
def _():
    """a dense SMALL-row block that is not diagonally dominant, tol = 1: pinv is not the identity inside it -- the scatter
    X[(pinv[i] - r0) * RHS_TILE + lane] of the forward solve"""
    blocks = [(SMALL, 1, "dense"), (10, 0, "cyclic"), (1, 0, "dense")]
    return build(222, blocks, lambda rng, lay: _to_lower(rng, lay, 5), weak=(0,), widths=(1, RHS_TILE, RHS_TILE + 1))


# F terms per row (forward) and per column (transposed)
@case("f_rows", levels=2, f_chunks=3, fc_chunks=1, large_blocks=0, f_row_counts=F_ROW_COUNTS)
def _():
    """a level-1 block whose rows hold each count of F_ROW_COUNTS coupling entries into level-0 columns"""
    blocks = [(len(F_ROW_COUNTS), 1, "cyclic"), (CHUNK + 2, 0, "cyclic"), (40, 0, "banded 2"), (2 * CHUNK - 40, 0, "cyclic")]

    def couple(rng, lay):
        below = lay.of_level(0)
        assert len(below) >= max(F_ROW_COUNTS)
        fr, fc = [], []
        for i, cnt in zip(lay.rows(0), F_ROW_COUNTS):
            fr += [int(i)] * cnt
            fc += rng.choice(below, cnt, replace=False).tolist()
        return fr, fc
    return build(230, blocks, couple, widths=WIDTHS)


@case("f_cols", levels=3, fc_chunks=3, f_chunks=1, large_blocks=0, f_col_counts=F_COL_COUNTS)
def _():
    """a level-0 block whose columns are coupled each to a count of F_COL_COUNTS rows of blocks of levels 1 and 2"""
    blocks = [(30, 2, "banded 1"), (CHUNK + 2, 1, "cyclic"), (CHUNK - 20, 1, "cyclic"), (len(F_COL_COUNTS), 0, "cyclic"),
              (3, 0, "cyclic")]

    def couple(rng, lay):
        above = np.concatenate([lay.of_level(2), lay.of_level(1)])
        assert len(above) >= max(F_COL_COUNTS)
        fr, fc = [], []
        for j, cnt in zip(lay.rows(3), F_COL_COUNTS):
            fr += rng.choice(above, cnt, replace=False).tolist()
            fc += [int(j)] * cnt
        fr += [int(lay.rows(0)[4])]                          # level 2 reaches level 1
        fc += [int(lay.rows(1)[7])]
        return fr, fc
    return build(231, blocks, couple, widths=WIDTHS)


# level mix
def _mix(seed, top_single):
    big = SMALL + 1
    # (the single block moves between level 2 and level 0: as many device groups in a refactor either way)
    blocks = ([(big + 3, 2, "banded 2")] + ([(1, 2, "dense")] if top_single else [])
              + [(big + 1, 1, "banded 1"), (big, 1, "cyclic"), (4, 1, "cyclic"), (big + 30, 0, "banded 2"), (2, 0, "dense")]
              + ([] if top_single else [(1, 0, "dense")]))
    return build(seed, blocks, lambda rng, lay: _to_lower(rng, lay, 12), refactor="perturb")


@case("mix_levels", other="mix_levels_top_small", cut="launches", levels=3, large_blocks=4, launches=3, lds_rows=(2, 4, 0),
      host_groups=4)
def _():
    """level 2 holds only a large block (no launch of k_btf_small: launches = 1 + 2), with F rows; level 1 two large blocks and a
    small one together; level 0 a large block and a small one"""
    return _mix(240, False)


@case("mix_levels_top_small", other="mix_levels", cut="launches", levels=3, large_blocks=4, launches=4, lds_rows=(2, 4, 1))
def _():
    return _mix(241, True)


@case("chain_max_1", levels=5, blocks=5, launches=6, lds_rows=(SMALL, 1, SMALL, 1, SMALL), large_blocks=0)
def _():
    """five levels, one block each, SMALL rows and 1 row in turn: the dynamic LDS size changes from launch to launch"""
    blocks = [(SMALL, 4, "dense"), (1, 3, "dense"), (SMALL, 2, "dense"), (1, 1, "dense"), (SMALL, 0, "banded 3")]

    def couple(rng, lay):
        fr, fc = _to_lower(rng, lay, 1)
        for b in (0, 2):                                     # and the two upper large-tile blocks reach level 0 directly
            fr += rng.choice(lay.rows(b), 30, replace=False).tolist()
            fc += rng.choice(lay.rows(4), 30, replace=False).tolist()
        return fr, fc
    return build(242, blocks, couple, widths=WIDTHS)


# refactor groups
def _rf_groups(g, seed):
    if g == 1:                                               # one block alone: no F at all
        return build(seed, [(CHUNK + 2, 0, "dense")], lambda rng, lay: ([], []), refactor="perturb")
    blocks = [(CHUNK + 2, 1, "dense")] + [(m, 0, "cyclic") for m in (3, 1, 2, 4, 1)[:g - 1]]
    return build(seed, blocks, lambda rng, lay: _to_lower(rng, lay, 2), refactor="perturb")


_RF_CUTS = {RF_WAVES: ("rf_groups_%d" % (RF_WAVES + 1), "rf_workgroups"), RF_WAVES + 1: ("rf_groups_%d" % RF_WAVES, "rf_workgroups")}
for _k, _g in enumerate(RF_GROUP_COUNTS):
    case("rf_groups_%d" % _g, *_RF_CUTS.get(_g, (None, None)), device_groups=_g, host_groups=0, lu_chunks=2,
         rf_workgroups=-(-_g // RF_WAVES), rf_last_waves=_g - (-(-_g // RF_WAVES) - 1) * RF_WAVES)(
        functools.partial(_rf_groups, _g, 250 + _k))


@case("rf_max_and_ones", device_groups=41, host_groups=0, max_block=SMALL, min_block=1, lu_chunks=2)
def _():
    """one dense SMALL-row block listed between many 1-row blocks: k_refactor launches the groups biggest first"""
    blocks = [(1, 1, "dense")] * 15 + [(SMALL, 1, "dense")] + [(1, 1, "dense")] * 5 + [(1, 0, "dense")] * 20
    return build(260, blocks, lambda rng, lay: _to_lower(rng, lay, 4), refactor="perturb")


@case("rf_host_beside_device", device_groups=2, host_groups=1, host_columns=SMALL + 1, device_columns=2 * SMALL, large_blocks=1)
def _():
    """a dense block over the cut beside two of SMALL rows: the host loop and k_refactor in one refactor"""
    blocks = [(SMALL + 1, 1, "dense"), (SMALL, 0, "dense"), (SMALL, 0, "banded 4")]
    return build(261, blocks, lambda rng, lay: _to_lower(rng, lay, 10), refactor="perturb")


@case("rf_fail_max", device_groups=3, host_groups=0, max_block=SMALL, lu_chunks=2, fails=True)
def _():
    """new values that make the dense SMALL-row block exactly singular with the pivots kept: a zero pivot in its last column, on
    the two-pass path of k_refactor; the refactor gives False and nothing changes"""
    blocks = [(SMALL, 1, "dense"), (3, 0, "cyclic"), (1, 0, "dense")]
    return build(262, blocks, lambda rng, lay: _to_lower(rng, lay, 3), refactor="singular")


def refactor_cases():
    return [name for name in CASES if get(name)["refactor"] is not None]


# lusol_factor.refactor on the same kernel: disconnected dense components on each side of the chunk and of RF_MAX
LUSOL_SIZES = (CHUNK + 2, SMALL, SMALL + 1, CHUNK + 2, SMALL, SMALL + 1)


@functools.lru_cache(maxsize=None)
def lusol_components():
    """(S, S2, sizes): dense diagonally dominant components, no couplings, natural order (lusol_factor at order 0 keeps it)"""
    rng = np.random.default_rng(270)
    S = sp.block_diag([_block(rng, m, "dense", True) for m in LUSOL_SIZES], format="csc")
    S.sort_indices()
    return S, perturbed(S, 271), np.asarray(LUSOL_SIZES)
