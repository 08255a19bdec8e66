"""Constructed inputs for the block routes of cs_lu and cs_qr (csx_lu_blocks, csx_qr_blocks in csx_lu.hip), the connected-components
pass under them (csx_components.hip), the strip-to-CSC fill and csx_happly (csx_qr.hip): one named case per edge, built with fixed
seeds.  TEST INFRASTRUCTURE, NOT PRODUCT.

Every cut comes from the library (`_csx.block_limits()`, no device needed), never from a literal.  A case names the facts it must
show (`claims`: route, ncomp, maxc, waves, lanes of the last wave, ...) and, where its edge has another side, the case across it
(`other`) and the fact that differs (`cut`).  tests/test_block_cases_cpu.py holds the table to these claims without a device and
pins csx_lu_host, the code the device is compared with, to the oracle; tests/test_gpu_block_factor.py runs every case on the device
and compares bytes.

Unless a case says otherwise a block has a cyclic off-diagonal (it keeps the block connected and m2 == m), the blocks' indices are
interleaved by a seeded permutation, and columns are stored with ascending rows.  Tie and cancellation cases use small integers, so
every operation is exact.  Only `sing_nan_*` holds a NaN; no case has an inf, or tol = 0 with a zero diagonal.

What no case reaches is listed in NOT_REACHED with the reason."""
import functools

import numpy as np

import _csx

LIM = _csx.block_limits()
LU_MAX_M, LU_MIN_COMPONENTS, QR_MAX_M, QR_MIN_COMPONENTS, HAPPLY_MAX_LEVELS = (LIM[k] for k in _csx.BLOCK_LIMITS)
MAX_M, MIN_C = LU_MAX_M, LU_MIN_COMPONENTS       # the table is built on the LU cuts; the CPU test holds the QR cuts equal to them
WAVE = 64                                        # lanes of a wave = components of a workgroup of k_lu_blocks / k_qr_blocks

NOT_REACHED = {
    "connected_components: 64 rounds": "a round hooks every edge whose ends have different roots and then flattens every chain, so "
                                       "components merge many at a time; the scrambled path of `comp_long_path` settles inside the "
                                       "cap, and no graph of a size a test can hold is known to need 64 rounds",
    "k_qr_blocks: root[cc] != myroot": "the walk up the column elimination tree leaves the block only with parent / leftmost / "
                                       "pinv taken from the analysis of another matrix; cs_qr always passes the analysis of A itself",
    "k_qr_blocks: pinv[i] < 0": "cs_sqr gives every row of a square matrix with m2 == m a place; as above it needs a foreign analysis",
    "n * ld past 2^31": "the strips hold n * maxc entries each: 2^31 needs n > 22 M with a 96-row block, 3 x 17 GB of strips",
}


# ---- the model ----------------------------------------------------------------------------------------------------------------
def roots(n, Ap, Ai, skip_first=0, skip_last=0):
    """union-find over the edges (j, Ai[q]), q in [Ap[j] + skip_first, Ap[j + 1] - skip_last): root[v] = the smallest vertex of
    v's component"""
    par = list(range(n))

    def find(v):
        while par[v] != v:
            par[v] = par[par[v]]
            v = par[v]
        return v

    Ap, Ai = np.asarray(Ap).tolist(), np.asarray(Ai).tolist()
    for j in range(n):
        a = find(j)
        for q in range(Ap[j] + skip_first, Ap[j + 1] - skip_last):
            b = find(Ai[q])
            if a != b:
                a, b = (a, b) if a < b else (b, a)
                par[b] = a
    return np.asarray([find(v) for v in range(n)], np.int32)


def grouping(root):
    """what group_by_root must give for these roots: nodes, first, count, comp_of_pos, ncomp, maxc"""
    n = len(root)
    nodes = np.argsort(root, kind="stable").astype(np.uint32)
    if n == 0:
        return nodes, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 0, 0
    sroot = root[nodes]
    head = np.concatenate([[True], sroot[1:] != sroot[:-1]])
    first = np.flatnonzero(head).astype(np.int32)
    count = np.diff(np.concatenate([first, [n]])).astype(np.int32)
    comp_of_pos = (np.cumsum(head) - 1).astype(np.int32)
    return nodes, first, count, comp_of_pos, len(first), int(count.max())


def route(n, ncomp, maxc):
    """csx_lu_blocks / csx_qr_blocks: the device route, or done = 0"""
    return "device" if n >= MIN_C and ncomp >= MIN_C and maxc <= MAX_M else "host"


def facts(n, Ap, Ai):
    root = roots(n, Ap, Ai)
    _, first, count, _, ncomp, maxc = grouping(root)
    return {"n": n, "ncomp": ncomp, "maxc": maxc, "route": route(n, ncomp, maxc), "waves": -(-ncomp // WAVE),
            "last_lanes": ncomp - (ncomp - 1) // WAVE * WAVE, "minc": int(count.min()), "counts": count, "root": root}


def house_levels(n, Vp, Vi, m):
    """csx_qr.hip house_levels: level of a reflection = the highest level + 1 among the earlier ones sharing a row; the number of levels"""
    rowlev = [0] * m
    nlev = 0
    Vp, Vi = np.asarray(Vp).tolist(), np.asarray(Vi).tolist()
    for k in range(n):
        rows = Vi[Vp[k]:Vp[k + 1]]
        lv = max([rowlev[r] for r in rows], default=0)
        for r in rows:
            rowlev[r] = lv + 1
        nlev = max(nlev, lv + 1)
    return nlev


def happly_route(nlevels, n):
    return "one_launch" if nlevels > HAPPLY_MAX_LEVELS or nlevels == n else "levelled"


# ---- builders -----------------------------------------------------------------------------------------------------------------
def members(rng, sizes, interleave=True, low_singles=0):
    """the vertex sets of the blocks: a seeded permutation cut into pieces (each sorted); the first `low_singles` blocks, which
    must be of one row, get the vertices 0 .. low_singles - 1"""
    n = int(np.sum(sizes))
    perm = np.arange(n)
    if interleave:
        perm = np.concatenate([np.arange(low_singles), low_singles + rng.permutation(n - low_singles)])
    out, base = [], 0
    for m in sizes:
        out.append(np.sort(perm[base:base + m]))
        base += m
    return n, out


def entries(D):
    """(r, c, v) of the nonzeros of a dense block, column by column, rows ascending"""
    c, r = np.nonzero(D.T)
    return r, c, D[r, c]


def rand_block(rng, m, density=0.3, diag="weak", band=None):
    D = rng.uniform(-1, 1, (m, m)) * (rng.random((m, m)) < density)
    ix = np.arange(m)
    if band is not None:
        D *= np.abs(ix[:, None] - ix[None, :]) <= band
    if diag == "weak":                                                   # pivoting must move rows
        D[ix, ix] = rng.uniform(-0.2, 0.2, m)
        D += np.diag(rng.uniform(0.5, 1.0, m)) * (rng.random(m) < 0.3)   # sometimes strong
    else:
        D[ix, ix] = rng.uniform(0.5, 1.5, m)
    for a in range(m):
        D[a, (a + 1) % m] += 0.7
    if diag == "dominant":                                               # by columns: no pivot is ever 0 without pivoting
        D[ix, ix] = np.abs(D).sum(axis=0) + 1.0
    return D


def assemble(n, mems, blocks, storage="asc", rng=None):
    """CSC of the blocks (r, c, v in local indices) on their vertex sets.  storage: asc / desc (rows inside a column), shuffled (by
    rng), given (the order the entries of a column come in)"""
    if not blocks:
        return {"n": n, "Ap": np.zeros(n + 1, np.int32), "Ai": np.zeros(0, np.int32), "Ax": np.zeros(0)}
    r = np.concatenate([mem[b[0]] for mem, b in zip(mems, blocks)])
    c = np.concatenate([mem[b[1]] for mem, b in zip(mems, blocks)])
    v = np.concatenate([np.asarray(b[2], dtype=np.float64) for b in blocks])
    if storage == "asc":
        order = np.lexsort((r, c))
    elif storage == "desc":
        order = np.lexsort((-r, c))
    elif storage == "shuffled":
        pre = rng.permutation(len(r))
        order = pre[np.argsort(c[pre], kind="stable")]
    else:
        order = np.argsort(c, kind="stable")
    Ap = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.int32)
    return {"n": n, "Ap": Ap, "Ai": r[order].astype(np.int32), "Ax": v[order].astype(np.float64)}


def last_wins(M):
    """the matrix cs_lu factors when a column stores a row twice: the last value (x[i] = Ax[p]); rows ascending, as (Ap, Ai, Ax)"""
    n = M["n"]
    c = np.repeat(np.arange(n), np.diff(M["Ap"]))
    order = np.lexsort((np.arange(len(c)), M["Ai"], c))
    r, cc, v = M["Ai"][order], c[order], M["Ax"][order]
    last = np.concatenate([(r[1:] != r[:-1]) | (cc[1:] != cc[:-1]), [True]])
    Ap = np.concatenate([[0], np.cumsum(np.bincount(cc[last], minlength=n))]).astype(np.int32)
    return Ap, r[last].astype(np.int32), v[last]


def random_blocks(seed, sizes, storage="asc", low_singles=0, **kw):
    rng = np.random.default_rng(seed)
    n, mems = members(rng, sizes, low_singles=low_singles)
    M = assemble(n, mems, [entries(rand_block(rng, int(m), **kw)) for m in sizes], storage, rng)
    M["mems"] = mems
    return M


def small_sizes(seed, k, lo=2, hi=5):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=k)


# ---- the table ----------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name, kinds, tols=(1.0,), other=None, cut=None, **claims):
    """kinds: "lu", "qr", "comp" (the case also runs through csx_prim_components alone).  claims: facts() entries the case must show"""
    def deco(fn):
        CASES[name] = {"name": name, "kinds": kinds, "tols": tols, "other": other, "cut": cut, "claims": claims,
                       "build": functools.lru_cache(maxsize=None)(fn)}
        return fn
    return deco


def get(name):
    return CASES[name]["build"]()


# size cuts
@case("singletons_63", ("lu", "qr"), other="singletons_64", cut="n", route="host", n=MIN_C - 1, ncomp=MIN_C - 1, maxc=1)
def _():
    return random_blocks(101, np.ones(MIN_C - 1, int))


@case("singletons_64", ("lu", "qr"), other="singletons_63", cut="n", route="device", n=MIN_C, ncomp=MIN_C, maxc=1, waves=1)
def _():
    return random_blocks(102, np.ones(MIN_C, int))


@case("ncomp_63", ("lu", "qr"), other="ncomp_64", cut="route", route="host", ncomp=MIN_C - 1)
def _():
    return random_blocks(103, small_sizes(103, MIN_C - 1))


@case("ncomp_64", ("lu", "qr"), other="ncomp_63", cut="route", route="device", ncomp=MIN_C, waves=1, last_lanes=WAVE)
def _():
    return random_blocks(104, small_sizes(104, MIN_C))


@case("ncomp_65", ("lu", "qr", "comp"), other="ncomp_64", cut="waves", route="device", ncomp=WAVE + 1, waves=2, last_lanes=1)
def _():
    return random_blocks(105, small_sizes(105, WAVE + 1))


@case("ncomp_129", ("lu", "qr"), tols=(1.0, 0.001), route="device", ncomp=2 * WAVE + 1, waves=3, last_lanes=1)
def _():
    return random_blocks(106, small_sizes(106, 2 * WAVE + 1))


@case("maxc_96", ("lu", "qr"), other="maxc_97", cut="route", route="device", ncomp=MIN_C + 1, maxc=MAX_M)
def _():
    return random_blocks(107, np.concatenate([small_sizes(107, MIN_C), [MAX_M]]), density=0.08)


@case("maxc_97", ("lu", "qr"), other="maxc_96", cut="route", route="host", ncomp=MIN_C + 1, maxc=MAX_M + 1)
def _():
    return random_blocks(108, np.concatenate([small_sizes(108, MIN_C), [MAX_M + 1]]), density=0.08)


@case("wave_96_and_ones", ("lu", "qr"), route="device", ncomp=WAVE, maxc=MAX_M, minc=1, waves=1)
def _():
    """one wave: a 96-row block (ld = 96) between one-row blocks (m = 1): the strip base tr.first * ld and the (m + 1)-slot
    pointer strips at tr.first + c of the lanes behind the large block"""
    M = random_blocks(109, np.concatenate([np.ones(20, int), [MAX_M], np.ones(WAVE - 21, int)]), low_singles=20, density=0.08)
    return M


@case("blocks96_band8", ("lu", "qr"), route="device", ncomp=MIN_C, maxc=MAX_M, minc=MAX_M)
def _():
    return random_blocks(110, np.full(MIN_C, MAX_M), density=1.0, band=8)


@case("blocks96_dense", ("lu", "qr"), route="device", ncomp=MIN_C, maxc=MAX_M, minc=MAX_M)
def _():
    return random_blocks(111, np.full(MIN_C, MAX_M), density=1.0)


# membership
@case("stride_members", ("lu", "qr", "comp"), route="device", ncomp=70, maxc=4, minc=4)
def _():
    """block c = {c, c + ncomp, c + 2 ncomp, c + 3 ncomp}"""
    rng = np.random.default_rng(120)
    nc, m = 70, 4
    mems = [c + nc * np.arange(m) for c in range(nc)]
    M = assemble(nc * m, mems, [entries(rand_block(rng, m)) for _ in range(nc)])
    M["mems"] = mems
    return M


@case("root_via_last", ("lu", "qr", "comp"), route="device", ncomp=70)
def _():
    """the smallest vertex of a block has only its diagonal entry in its column and hangs on the block by one entry A(v, j), j the
    block's largest vertex"""
    rng = np.random.default_rng(121)
    sizes = small_sizes(121, 70, 3, 6)
    n, mems = members(rng, sizes)
    blocks = []
    for m in sizes.tolist():
        D = np.zeros((m, m))
        D[1:, 1:] = rand_block(rng, m - 1, density=0.4)
        D[0, 0] = rng.uniform(0.5, 1.5)
        D[0, m - 1] = rng.uniform(0.5, 1.5)
        blocks.append(entries(D))
    M = assemble(n, mems, blocks)
    M["mems"] = mems
    return M


def _graph_block(rng, m, edges, diag="weak"):
    D = np.zeros((m, m))
    for a, b in edges:
        D[a, b] = rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0])
        D[b, a] = rng.uniform(0.3, 1.0) * rng.choice([-1.0, 1.0])
    D[np.arange(m), np.arange(m)] = rng.uniform(-0.2, 0.2, m) if diag == "weak" else rng.uniform(0.5, 1.5, m)
    return D


@case("path_scrambled", ("lu", "qr", "comp"), route="device", ncomp=66, maxc=MAX_M)
def _():
    """every block a path whose vertices are labelled in a scrambled order (one of 96 vertices among them)"""
    rng = np.random.default_rng(122)
    sizes = np.concatenate([rng.integers(2, 30, size=65), [MAX_M]])
    n, mems = members(rng, sizes)
    blocks = []
    for m in sizes.tolist():
        lab = rng.permutation(m)
        blocks.append(entries(_graph_block(rng, m, [(lab[a], lab[a + 1]) for a in range(m - 1)], diag="strong")))
    M = assemble(n, mems, blocks)
    M["mems"] = mems
    return M


@case("star_scrambled", ("lu", "qr", "comp"), route="device", ncomp=66)
def _():
    """every block a star whose centre is not its smallest vertex"""
    rng = np.random.default_rng(123)
    sizes = rng.integers(3, 30, size=66)
    n, mems = members(rng, sizes)
    blocks = []
    for m in sizes.tolist():
        centre = int(rng.integers(1, m))
        blocks.append(entries(_graph_block(rng, m, [(centre, a) for a in range(m) if a != centre], diag="strong")))
    M = assemble(n, mems, blocks)
    M["mems"] = mems
    return M


@case("halves_one_link", ("lu", "qr", "comp"), route="device", ncomp=MIN_C + 1, maxc=MAX_M)
def _():
    """two 48-row halves, each connected in itself, joined by ONE entry A(i, j) with no A(j, i): one component of 96 rows"""
    rng = np.random.default_rng(124)
    sizes = np.concatenate([small_sizes(124, MIN_C), [MAX_M]])
    n, mems = members(rng, sizes)
    blocks = [entries(rand_block(rng, int(m))) for m in sizes[:-1]]
    h = MAX_M // 2
    D = np.zeros((MAX_M, MAX_M))
    half = rng.permutation(MAX_M)                                        # the halves interleave inside the block as well
    for part in (half[:h], half[h:]):
        D[np.ix_(part, part)] = rand_block(rng, len(part), density=0.1)
    assert D[half[h + 3], half[2]] == 0.0 and D[half[2], half[h + 3]] == 0.0
    D[half[h + 3], half[2]] = 0.9
    blocks.append(entries(D))
    M = assemble(n, mems, blocks)
    M["mems"], M["link"] = mems, (int(mems[-1][half[h + 3]]), int(mems[-1][half[2]]))
    return M


# pivot rule
TIE_BLOCK = np.array([[1.0, 2.0, 1.0, -1.0],
                      [2.0, -1.0, 2.0, 1.0],
                      [-2.0, 2.0, 1.0, 0.0],
                      [0.0, 3.0, 0.0, 1.0]])
# column 0: rows 1 and 2 tie at 2 above the diagonal's 1.  Column 1 after the exact update with the pivot row 2 (multipliers
# -1 and -1/2): x = (3, 1, ., 3): rows 0 and 3 tie at 3 above the diagonal's 1.  In both columns the reach lists the rows in
# reverse storage order, so the first maximum is the candidate stored LAST; the entries of the other candidate, which a
# scaling by 1 + 2^-40 turns into the only maximum:
TIE_BREAKERS = ((1, 0), (0, 1))


@case("ties", ("lu",), route="device", ncomp=70, maxc=4)
def _():
    """blocks of +-1, +-2 (and one 3) entries, each scaled by a power of two and by a sign: two candidates tie in the first column
    and again in the second after one exact update"""
    rng = np.random.default_rng(130)
    sizes = np.full(70, 4)
    n, mems = members(rng, sizes)
    scale = 2.0 ** rng.integers(-3, 4, size=70) * rng.choice([-1.0, 1.0], size=70)
    scale[0] = 1.0
    M = assemble(n, mems, [entries(TIE_BLOCK * s) for s in scale])
    M["mems"] = mems
    return M


@case("no_diagonal", ("lu",), tols=(1.0, 0.001), route="device", ncomp=70)
def _():
    """cyclic-shift blocks with no diagonal entry stored: x[k] read by the threshold test must be a clean 0.0"""
    rng = np.random.default_rng(131)
    sizes = small_sizes(131, 70, 2, 9)
    n, mems = members(rng, sizes)
    blocks = []
    for m in sizes.tolist():
        D = rng.uniform(-1, 1, (m, m)) * (rng.random((m, m)) < 0.3)
        for a in range(m):
            D[a, (a + 1) % m] = rng.uniform(1.0, 2.0)
        D[np.arange(m), np.arange(m)] = 0.0
        blocks.append(entries(D))
    M = assemble(n, mems, blocks)
    M["mems"] = mems
    return M


@case("row_k_taken_early", ("lu",), tols=(1.0, 0.5), route="device", ncomp=70)
def _():
    """A(c + 1, c) dominates every even column c: row c + 1 is pivotal before column c + 1 comes, whose threshold test must skip it"""
    rng = np.random.default_rng(132)
    sizes = small_sizes(132, 70, 2, 9)
    n, mems = members(rng, sizes)
    blocks = []
    for m in sizes.tolist():
        D = rand_block(rng, m, density=0.5, diag="strong")
        for c in range(0, m - 1, 2):
            D[c + 1, c] = 5.0
        blocks.append(entries(D))
    M = assemble(n, mems, blocks)
    M["mems"] = mems
    return M


@case("mixed_tol", ("lu", "qr"), tols=(1.0, 0.5, 0.001), route="device", ncomp=100)
def _():
    return random_blocks(133, np.random.default_rng(133).integers(1, 40, size=100))


@case("dominant_tol0", ("lu",), tols=(0.0, 1.0), route="device", ncomp=80)
def _():
    """column-dominant diagonals: with tol = 0 the diagonal is always taken and is never 0"""
    return random_blocks(134, np.random.default_rng(134).integers(1, 30, size=80), diag="dominant")


# storage
@case("storage_desc", ("lu", "qr"), tols=(1.0, 0.001), route="device", ncomp=80)
def _():
    return random_blocks(140, np.random.default_rng(140).integers(1, 30, size=80), storage="desc")


@case("storage_shuffled", ("lu", "qr"), tols=(1.0, 0.001), route="device", ncomp=80)
def _():
    return random_blocks(141, np.random.default_rng(141).integers(1, 30, size=80), storage="shuffled")


@case("storage_dups", ("lu", "qr"), tols=(1.0, 0.001), route="device", ncomp=80)
def _():
    """every third entry stored a second time with another value, anywhere in its column: the LAST one is the value (x[i] = Ax[p]),
    and the first one places the row in the reach"""
    rng = np.random.default_rng(142)
    sizes = rng.integers(1, 30, size=80)
    n, mems = members(rng, sizes)
    blocks = []
    for m in sizes.tolist():
        r, c, v = entries(rand_block(rng, int(m)))
        dup = rng.random(len(r)) < 1.0 / 3.0
        blocks.append((np.concatenate([r, r[dup]]), np.concatenate([c, c[dup]]),
                       np.concatenate([v, rng.uniform(-1, 1, int(dup.sum()))])))
    M = assemble(n, mems, blocks, "shuffled", rng)
    M["mems"] = mems
    return M


# singular blocks (cs_lu gives None)
SINGULAR_KINDS = ("empty", "zero", "cancel", "nan")
SINGULAR_PLACES = ("first", "last")


def _singular(kind, place, seed):
    rng = np.random.default_rng(seed)
    sizes = small_sizes(seed, WAVE + 1, 3, 5)
    n, mems = members(rng, sizes)
    lows = [int(mem[0]) for mem in mems]
    t = int(np.argmin(lows)) if place == "first" else int(np.argmax(lows))     # component 0 / component 64: lane 0 of wave 1
    blocks = []
    for b, m in enumerate(sizes.tolist()):
        D = rand_block(rng, m)
        r, c, v = entries(D)
        if b == t:
            if kind == "empty":                                                 # (vertex 1 stays in the block through its row)
                keep = c != 1
                r, c, v = r[keep], c[keep], v[keep]
            elif kind == "zero":
                keep = c != 1
                r, c, v = np.append(r[keep], 1), np.append(c[keep], 1), np.append(v[keep], 0.0)
            elif kind == "cancel":                                              # columns 0 and 1 equal, +-1 and +-2: exact
                D = rng.choice([-2.0, -1.0, 1.0, 2.0], size=(m, m))
                D[:, 1] = D[:, 0]
                r, c, v = entries(D)
            else:
                v = np.where(c == 1, np.nan, v)
        blocks.append((r, c, v))
    M = assemble(n, mems, blocks)
    M["mems"], M["target"] = mems, t
    return M


for _k, _kind in enumerate(SINGULAR_KINDS):
    for _p, _place in enumerate(SINGULAR_PLACES):
        case("sing_%s_%s" % (_kind, _place), ("lu",), route="device", ncomp=WAVE + 1, waves=2, last_lanes=1, singular=True,
             target=0 if _place == "first" else WAVE)(functools.partial(_singular, _kind, _place, 150 + 2 * _k + _p))
HEALTHY_AFTER_SINGULAR = ("ncomp_65", 1.0)


# cs_house with tail2 == 0 (QR)
HOUSE_HEADS = (1.5, -1.5, 0.0, -0.0)


@case("house_1x1", ("qr",), route="device", ncomp=68, maxc=1, tail2_zero=True)
def _():
    """1 x 1 blocks with a positive, a negative, a +0.0 and a -0.0 entry"""
    n = 68
    return {"n": n, "Ap": np.arange(n + 1, dtype=np.int32), "Ai": np.arange(n, dtype=np.int32),
            "Ax": np.asarray([HOUSE_HEADS[k % 4] * (1 + k // 4) for k in range(n)])}


@case("house_upper", ("qr",), route="device", ncomp=72, tail2_zero=True)
def _():
    """upper-triangular blocks (nothing below a diagonal: tail2 == 0 in every column) whose diagonals run through the four heads"""
    rng = np.random.default_rng(161)
    sizes = rng.integers(1, 8, size=72)
    n, mems = members(rng, sizes)
    blocks, t = [], 0
    for m in sizes.tolist():
        r, c = np.triu_indices(m)
        keep = (r == c) | (c == r + 1) | (rng.random(len(r)) < 0.4)            # the superdiagonal keeps the block connected
        r, c = r[keep], c[keep]
        v = rng.uniform(0.5, 1.5, len(r)) * rng.choice([-1.0, 1.0], len(r))
        for q in np.flatnonzero(r == c):
            v[q] = HOUSE_HEADS[t % 4]
            t += 1
        blocks.append((r, c, v))
    M = assemble(n, mems, blocks)
    M["mems"] = mems
    return M


@case("house_zero_head", ("qr",), route="device", ncomp=72, zero_head=True)
def _():
    """the other branch of cs_house at a zero head: the first column of every block stores +0.0 or -0.0 on the diagonal above a
    nonzero tail, so v(0) = head - s and not -tail2 / (head + s)"""
    rng = np.random.default_rng(162)
    sizes = rng.integers(3, 12, size=72)
    n, mems = members(rng, sizes)
    blocks = []
    for b, m in enumerate(sizes.tolist()):
        D = rand_block(rng, m, density=0.5, diag="strong")
        D[1:, 0] = rng.uniform(0.5, 1.5, m - 1) * rng.choice([-1.0, 1.0], m - 1)
        r, c, v = entries(D)
        v[(r == 0) & (c == 0)] = 0.0 if b % 2 == 0 else -0.0
        blocks.append((r, c, v))
    M = assemble(n, mems, blocks)
    M["mems"] = mems
    return M


# csx_happly: V from cs_qr of a lower-bidiagonal chain of c columns (natural order: reflection k shares row k + 1 with k + 1, so
# nlevels = c) followed by s one-row blocks
def chain(c, s, seed):
    rng = np.random.default_rng(seed)
    n = c + s
    cols = np.concatenate([np.repeat(np.arange(c - 1), 2), [c - 1], np.arange(c, n)])
    rows = np.concatenate([(np.arange(c - 1)[:, None] + np.array([0, 1])[None, :]).reshape(-1), [c - 1], np.arange(c, n)])
    Ap = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int32)
    return {"n": n, "Ap": Ap, "Ai": rows.astype(np.int32), "Ax": rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows))}


HAPPLY_CASES = {      # name -> (matrix, nlevels, route)
    "chain_at_cut": (lambda: chain(HAPPLY_MAX_LEVELS, 8, 170), HAPPLY_MAX_LEVELS, "levelled"),
    "chain_over_cut": (lambda: chain(HAPPLY_MAX_LEVELS + 1, 8, 171), HAPPLY_MAX_LEVELS + 1, "one_launch"),
    "chain_200": (lambda: chain(200, 0, 172), 200, "one_launch"),
    "ncomp_65": (lambda: get("ncomp_65"), None, "levelled"),                 # many reflections to a level
}
HAPPLY_NRHS = (1, 63, 64, 65, 130)
HAPPLY_COLUMNS = (0, 63, 64)                                                  # and nrhs - 1


@functools.lru_cache(maxsize=None)
def happly_matrix(name):
    return HAPPLY_CASES[name][0]()


# components alone (csx_prim_components): (n, Ap, Ai, skip_first, skip_last, order, malformed)
def _triangle(name, lower):
    """the lower (diagonal first) or upper (diagonal last) triangle of the symmetrised pattern of a case"""
    M = get(name)
    n = M["n"]
    c = np.repeat(np.arange(n), np.diff(M["Ap"]))
    r = M["Ai"].astype(np.int64)
    rr, cc = np.concatenate([r, c, np.arange(n)]), np.concatenate([c, r, np.arange(n)])
    keep = rr >= cc if lower else rr <= cc
    pairs = np.unique(np.stack([cc[keep], rr[keep]], axis=1), axis=0)
    Ap = np.concatenate([[0], np.cumsum(np.bincount(pairs[:, 0], minlength=n))]).astype(np.int32)
    return n, Ap, pairs[:, 1].astype(np.int32)


def _long_path(n, seed):
    lab = np.random.default_rng(seed).permutation(n)
    r = np.concatenate([lab[:-1], lab[1:]])
    c = np.concatenate([lab[1:], lab[:-1]])
    order = np.lexsort((r, c))
    Ap = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.int32)
    return n, Ap, r[order].astype(np.int32)


def _one_star(n, centre):
    leaves = np.delete(np.arange(n), centre)
    r = np.concatenate([leaves, np.full(n - 1, centre)])
    c = np.concatenate([np.full(n - 1, centre), leaves])
    order = np.lexsort((r, c))
    Ap = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.int32)
    return n, Ap, r[order].astype(np.int32)


def _with_index(name, value):
    M = get(name)
    Ai = M["Ai"].copy()
    Ai[len(Ai) // 2] = value
    return M["n"], M["Ap"], Ai


def _matrix(name):
    M = get(name)
    return M["n"], M["Ap"], M["Ai"]


COMPONENT_CASES = {
    "comp_n1": (lambda: (1, np.array([0, 1], np.int32), np.array([0], np.int32)), 0, 0, 0, False),
    "comp_n1_empty": (lambda: (1, np.array([0, 0], np.int32), np.zeros(0, np.int32)), 0, 0, 0, False),
    "comp_no_entries": (lambda: (100, np.zeros(101, np.int32), np.zeros(0, np.int32)), 0, 0, 0, False),
    "comp_long_path": (lambda: _long_path(3000, 180), 0, 0, 0, False),                  # one component of all n
    "comp_one_star": (lambda: _one_star(500, 310), 0, 0, 0, False),                     # its centre is not the root
    "comp_index_minus1": (lambda: _with_index("ncomp_65", -1), 0, 0, 0, True),
    "comp_index_n": (lambda: _with_index("ncomp_65", get("ncomp_65")["n"]), 0, 0, 0, True),
    # as the triangular planner passes them: L' by the columns of L (diagonal first, skipped; neighbours above the row: order 2),
    # U' by the columns of U (diagonal last, skipped; neighbours below: order 1)
    "comp_lower_order2": (lambda: _triangle("stride_members", True), 1, 0, 2, False),
    "comp_upper_order1": (lambda: _triangle("path_scrambled", False), 0, 1, 1, False),
    "comp_lower_order0": (lambda: _triangle("star_scrambled", True), 0, 0, 0, False),
    "comp_lower_wrong_side": (lambda: _triangle("stride_members", True), 1, 0, 1, True),
    "comp_upper_wrong_side": (lambda: _triangle("path_scrambled", False), 0, 1, 2, True),
    "comp_diagonal_not_skipped": (lambda: _triangle("stride_members", True), 0, 0, 2, True),
}
for _name, _c in CASES.items():
    if "comp" in _c["kinds"]:
        COMPONENT_CASES["comp_" + _name] = (functools.partial(_matrix, _name), 0, 0, 0, False)


@functools.lru_cache(maxsize=None)
def component_case(name):
    build, sf, sl, order, malformed = COMPONENT_CASES[name]
    n, Ap, Ai = build()
    return n, np.asarray(Ap, np.int32), np.asarray(Ai, np.int32), sf, sl, order, malformed


LU_CASES = [(name, tol) for name, c in CASES.items() if "lu" in c["kinds"] and not c["claims"].get("singular") for tol in c["tols"]]
SINGULAR_CASES = [name for name, c in CASES.items() if c["claims"].get("singular")]
QR_CASES = [name for name, c in CASES.items() if "qr" in c["kinds"]]
TIE_CASES = ["ties"]
