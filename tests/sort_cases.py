"""Constructed inputs for the integer primitives of csx_sort.hip (scan_exclusive_i32, suffix_min_i32, expand_columns,
boundaries_from_sorted, stable_sort_by_key_ex), one named case per edge, and a Python model of the decisions the host code takes
and of the per-tile facts the kernels branch on.  TEST INFRASTRUCTURE, NOT PRODUCT.

Every size comes from the library's own constants (`_csx.prim_limits()`, no device needed), never from a literal.  A case names
the `edge` it sits on (facts the model must give for it) and, where the edge has another side, the `other` case across it and the
fact (`cut`) that differs.  tests/test_sort_cases_cpu.py holds the table to these claims without a device;
tests/test_gpu_sort.py runs every case through the csx_prim_* entry points, compares with numpy bit for bit and holds
csx_prim_sort_info to `sort_model` field for field.

The model: `depth` (levels of the scan / suffix-min recursion), `sort_model` (bits, passes, digit widths, tiles, chunks, record
layout, short-key mode and the k_rs_scatter instance of every pass, as stable_sort_by_key_ex takes them), `tile_starts` (K of
every tile descriptor, as k_rs_tiledesc_head counts it) with `branch_of` (the way the first pass of a transpose derives columns
from K), `hist_paths` (which histogram kernel reads keys on which load path), `boundary_paths`, `expand_grid`.

What no case reaches is listed in NOT_REACHED with the reason."""
import functools

import numpy as np

import _csx

LIM = _csx.prim_limits()
SCAN_TILE, SM_TILE, TILE, BINS, DESC, SEGS, CHUNK_MIN, CHUNK_DIV, GRID_MAX = (LIM[k] for k in _csx.PRIM_LIMITS)
MAXINT = 0x7fffffff
PAYLOADS = {"keys": (False, False), "a": (True, False), "v": (False, True), "av": (True, True)}

NOT_REACHED = {
    "chunk > RS_CHUNK_MIN": "the digit scan's chunk grows past RS_CHUNK_MIN tiles only above RS_CHUNK_MIN * RS_CHUNK_DIV = %d tiles, "
                            "%d records: no test of a few seconds sorts that many" % (CHUNK_MIN * CHUNK_DIV, CHUNK_MIN * CHUNK_DIV * TILE),
    "k_rs_hist16 on a misaligned array": "it reads only the sort's own 16-bit temporaries, which start whole allocations; its "
                                         "key-by-key path is reached through the partial last tile",
}


# ---- the model ----------------------------------------------------------------------------------------------------------------
def depth(n, tile):
    """launch levels of scan_exclusive_i32 / suffix_min_i32 on n elements: 0 for none, one more per recursion on the block results"""
    d = 0
    while n > 0:
        d += 1
        nb = -(-n // tile)
        n = nb if nb > 1 else 0
    return d


def key_bits(key_limit):
    bits = 1
    while bits < 32 and (1 << bits) < key_limit:
        bits += 1
    return bits


def digit_widths(bits):
    passes = (bits + 7) // 8
    return tuple(bits // passes + (1 if ps < bits % passes else 0) for ps in range(passes))


def sort_model(count, key_limit, has_a, has_v, want_key, expand_n=None, want_ptr=False, short_keys=1, misalign=0):
    """the fields of csx_prim_sort_info, by _csx.SORT_INFO, as stable_sort_by_key_ex decides them"""
    if count <= 0:
        return {"bits": 0, "passes": 0, "widths": (), "nblocks": 0, "chunk": 0, "nchunks": 0, "packed": 0, "k16": 0,
                "key_misalign": 0, "instances": (), "count": 0}
    bits = key_bits(key_limit)
    widths = digit_widths(bits)
    passes = len(widths)
    nblocks = -(-count // TILE)
    chunk = max(-(-nblocks // CHUNK_DIV), CHUNK_MIN)
    nchunks = -(-nblocks // chunk)
    expand = expand_n is not None
    has_a = has_a or expand
    packed = has_a and has_v
    w0 = widths[0]
    k16 = bool(expand and packed and passes == 3 and want_ptr and not want_key and bits - w0 <= 16 and
               expand_n <= (1 << (32 - w0)) and short_keys)
    inst = []
    for ps in range(passes):
        last = ps == passes - 1
        if k16:
            inst.append("short_first" if ps == 0 else "short_last" if last else "short_middle")
        elif packed:
            inst.append("av_%s_%s" % ("flat" if ps == 0 else "packed", "flat" if last else "packed"))
        else:
            inst.append("a" if has_a else "v" if has_v else "keys")
    return {"bits": bits, "passes": passes, "widths": widths, "nblocks": nblocks, "chunk": chunk, "nchunks": nchunks,
            "packed": int(packed), "k16": int(k16), "key_misalign": misalign, "instances": tuple(inst), "count": count}


def hist_paths(model):
    """{(kernel, load path)} of a sort: k_rs_hist reads the caller's keys in pass 0 and 16-byte aligned temporaries after it,
    k_rs_hist16 the 16-bit temporaries of the short-key mode; a full tile of an aligned array is read 16 bytes (hist16: 8) at a
    time, a partial last tile and every tile of a misaligned array key by key"""
    out = set()
    full, partial = model["count"] >= TILE, model["count"] % TILE != 0
    for ps in range(model["passes"]):
        kernel = "hist16" if model["k16"] and ps > 0 else "hist"
        aligned = ps > 0 or model["key_misalign"] == 0
        if full and aligned:
            out.add((kernel, "vector"))
        if partial or (full and not aligned):
            out.add((kernel, "scalar"))
    return out


def tile_starts(Ap, count):
    """K of every tile as k_rs_tiledesc_head counts it: the columns that start strictly inside the tile (after its base, at or
    before its last record), empty ones included"""
    P = np.asarray(Ap[:-1], np.int64)
    nb = -(-count // TILE)
    tb = np.arange(nb, dtype=np.int64) * TILE
    te = np.minimum(tb + TILE - 1, count - 1)
    return np.searchsorted(P, te, "right") - np.searchsorted(P, tb, "right")


def branch_of(K):
    return "paint" if K <= DESC else "lds" if K <= TILE else "search"


def desc_half_of_last_start(K):
    """0 / 1: the register (first / second half of the descriptor's words) that holds the last of K painted starts: two words
    of header, then 16 bits a start"""
    words = DESC // 2 + 2
    return int(((K - 1) + 4) >> 1 >= words // 2)


def remap(nblocks):
    """(q, rem) of the tile-to-XCD remap of k_rs_scatter"""
    return nblocks >> 3, nblocks & 7


def remap_tiles(nblocks):
    """the tile every workgroup of k_rs_scatter takes"""
    q, rem = remap(nblocks)
    b = np.arange(nblocks)
    x, kk = b & 7, b >> 3
    return x * q + np.minimum(x, rem) + kk


def boundary_paths(count, misalign):
    """load paths of the threads of k_boundaries: four keys by one 16-byte load; key by key in the last, partial group (which
    also closes the trailing keys); key by key everywhere for a misaligned array"""
    out = {"tail"}
    if count >= 4:
        out.add("vector" if misalign == 0 else "scalar")
    return out


def expand_grid(n):
    """(workgroups, does the grid-stride loop wrap) of expand_columns"""
    blocks = min((n + 3) // 4, GRID_MAX)
    return blocks, n > 4 * blocks


# ---- the table ----------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, prim, name, make, edge, other=None, cut=None, what=""):
        self.prim, self.name, self.make, self.edge, self.other, self.what = prim, name, make, edge, other, what
        self.cut = cut or (next(iter(edge)) if edge else None)


CASES = []


def _add(*args, **kw):
    CASES.append(Case(*args, **kw))


def _seed(name):
    import zlib
    return zlib.crc32(name.encode())


@functools.lru_cache(maxsize=3)
def inputs(name):
    """the case's arrays and arguments (read-only: numpy arrays are locked)"""
    d = BY_NAME[name].make(np.random.default_rng(_seed(name)))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def facts(name):
    """what the model says of the case"""
    c, d = BY_NAME[name], inputs(name)
    if c.prim == "scan":
        n = len(d["values"])
        return {"n": n, "depth": depth(n, SCAN_TILE), "blocks": -(-n // SCAN_TILE)}
    if c.prim == "sufmin":
        n = len(d["values"])
        return {"n": n, "depth": depth(n, SM_TILE), "blocks": -(-n // SM_TILE)}
    if c.prim == "boundaries":
        k = d["key"]
        return {"count": len(k), "rem4": len(k) % 4, "paths": boundary_paths(len(k), d["misalign"]), "nkeys": d["nkeys"],
                "misalign": d["misalign"], "longest_gap": int(np.diff(np.concatenate([[-1], k.astype(np.int64), [d["nkeys"]]])).max()) - 1,
                "closing": d["nkeys"] - (int(k[-1]) if len(k) else -1)}
    if c.prim == "expand":
        Ap = d["Ap"]
        blocks, wraps = expand_grid(len(Ap) - 1)
        return {"n": len(Ap) - 1, "nnz": int(Ap[-1]), "blocks": blocks, "wraps": wraps, "lengths": set(np.unique(np.diff(Ap)).tolist())}
    assert c.prim == "sort"
    xp = d.get("expand_ptr")
    m = sort_model(len(d["key"]), d["key_limit"], d.get("a") is not None, d.get("v") is not None, d.get("want_key", True),
                   None if xp is None else len(xp) - 1, d.get("nkeys") is not None, d.get("short_keys", 1), d.get("misalign", 0))
    m["hist"] = hist_paths(m)
    m["q"], m["rem"] = remap(m["nblocks"])
    m["K"] = tuple(tile_starts(xp, len(d["key"])).tolist()) if xp is not None and len(d["key"]) else ()
    m["branches"] = {branch_of(K) for K in m["K"]}
    m["w0_columns"] = None if xp is None or not m["passes"] else (1 << (32 - m["widths"][0])) - (len(xp) - 1)   # room left for columns
    return m


# -- scan and suffix-min
def _sizes(tile):
    return [("n0", 0), ("n1", 1), ("n2", 2), ("tile_m1", tile - 1), ("tile", tile), ("tile_p1", tile + 1), ("three_tiles", 3 * tile + 5),
            ("sq_m1", tile * tile - 1), ("sq", tile * tile), ("sq_p1", tile * tile + 1)]


_NEIGHBOUR = {"n0": "n1", "n1": "n0", "tile_m1": None, "tile": "tile_p1", "tile_p1": "tile", "sq_m1": None, "sq": "sq_p1", "sq_p1": "sq"}

for _tag, _n in _sizes(SCAN_TILE):
    _add("scan", "scan_" + _tag, (lambda n: lambda rng: {"values": rng.integers(0, 4, n).astype(np.int32)})(_n),
         {"depth": depth(_n, SCAN_TILE), "n": _n}, other=_NEIGHBOUR.get(_tag) and "scan_" + _NEIGHBOUR[_tag],
         what="n = %d: %d level(s)" % (_n, depth(_n, SCAN_TILE)))
_add("scan", "scan_zeros", lambda rng: {"values": np.zeros(3 * SCAN_TILE + 5, np.int32)}, {"depth": 2}, what="every element zero")


def _last_only(rng):
    v = np.zeros(3 * SCAN_TILE + 5, np.int32)
    v[-1] = 7
    return {"values": v}


_add("scan", "scan_last_only", _last_only, {"depth": 2}, what="the only nonzero is the last element: it shows in out[n] alone")


def _sufmin_random(n):
    def make(rng):
        v = rng.integers(-1000, 1000, n).astype(np.int32)
        if n >= 64:                                    # runs of the kernel's own fill value inside real data
            for s in rng.integers(0, n - 40, max(1, n // 3000)):
                v[s:s + int(rng.integers(1, 40))] = MAXINT
        return {"values": v}
    return make


for _tag, _n in _sizes(SM_TILE):
    _add("sufmin", "sufmin_" + _tag, _sufmin_random(_n), {"depth": depth(_n, SM_TILE), "n": _n},
         other=_NEIGHBOUR.get(_tag) and "sufmin_" + _NEIGHBOUR[_tag], what="n = %d: %d level(s)" % (_n, depth(_n, SM_TILE)))
_SMN = 3 * SM_TILE + 5
_add("sufmin", "sufmin_increasing", lambda rng: {"values": np.arange(-5, _SMN - 5, dtype=np.int32)}, {"depth": 2},
     what="strictly increasing: every element is its own answer")
_add("sufmin", "sufmin_decreasing", lambda rng: {"values": np.arange(_SMN, 0, -1, dtype=np.int32)}, {"depth": 2},
     what="strictly decreasing: every answer is the last element")


def _sufmin_maxint_runs(rng):
    v = rng.integers(0, 1000, _SMN).astype(np.int32)
    v[SM_TILE - 3:2 * SM_TILE + 3] = MAXINT             # a whole block of the fill value, and its neighbours' edges
    v[-4:] = MAXINT                                    # and the end of the array
    return {"values": v}


_add("sufmin", "sufmin_maxint_runs", _sufmin_maxint_runs, {"depth": 2}, what="0x7fffffff over a whole block and at the very end")


def _sufmin_min_in(block):
    def make(rng):
        v = rng.integers(0, 1000, _SMN).astype(np.int32)
        v[5 if block == "first" else _SMN - 2] = -12345
        return {"values": v}
    return make


_add("sufmin", "sufmin_min_last_block", _sufmin_min_in("last"), {"depth": 2}, what="the global minimum in the last block only")
_add("sufmin", "sufmin_min_first_block", _sufmin_min_in("first"), {"depth": 2}, what="the global minimum in the first block only")

# -- boundaries
BOUNDARY_COUNTS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 1023, 1024, 1025, 1026)      # every count % 4 below, at and above one and 256 groups


def _bnd(count, kind, mis):
    def make(rng):
        if kind == "one_key":                              # nkeys = 1: every key equal
            key, nkeys = np.zeros(count, np.uint32), 1
        elif kind == "nkeys_eq_count":                     # as many keys as records, duplicates and holes
            key, nkeys = np.sort(rng.integers(0, max(count, 1), count)).astype(np.uint32), count
        else:                                              # far above the largest key present: one thread closes thousands
            key, nkeys = np.sort(rng.integers(0, 50, count)).astype(np.uint32), 10000
        return {"key": key, "nkeys": nkeys, "misalign": mis}
    return make


for _c in BOUNDARY_COUNTS:
    for _kind in ("one_key", "nkeys_eq_count", "far_above"):
        for _mis in range(4):
            _add("boundaries", "bnd_%d_%s_mis%d" % (_c, _kind, _mis), _bnd(_c, _kind, _mis),
                 {"rem4": _c % 4, "count": _c, "misalign": _mis}, what="count %% 4 = %d" % (_c % 4))


def _bnd_equal(mis):
    return lambda rng: {"key": np.full(1025, 7, np.uint32), "nkeys": 20, "misalign": mis}


def _bnd_gap(mis):
    def make(rng):
        key = np.sort(np.concatenate([rng.integers(0, 10, 500), rng.integers(5010, 5100, 525)])).astype(np.uint32)
        key[499], key[500] = 9, 5010
        return {"key": key, "nkeys": 5100, "misalign": mis}
    return make


for _mis in range(4):
    _add("boundaries", "bnd_all_equal_mis%d" % _mis, _bnd_equal(_mis), {"longest_gap": 12, "closing": 13},
         what="every key equal, below nkeys - 1: keys before and after it are closed by one thread each")
    _add("boundaries", "bnd_gap5000_mis%d" % _mis, _bnd_gap(_mis), {"longest_gap": 5000},
         what="5 000 empty keys between two neighbours, filled by one thread")

# -- expand_columns
_EXP_LENGTHS = (0, 1, 63, 64, 65, 200)


def _exp_mixed(rng):
    lens = np.concatenate([np.array(_EXP_LENGTHS), rng.choice(_EXP_LENGTHS, 300)])
    return {"Ap": np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)}


def _exp_short(n):
    def make(rng):
        return {"Ap": np.concatenate([[0], np.cumsum(rng.integers(0, 3, n))]).astype(np.int32)}
    return make


_add("expand", "exp_mixed", _exp_mixed, {"lengths": set(_EXP_LENGTHS)}, what="columns of 0, 1, 63, 64, 65 and 200 entries: no, one, one, one, two and four rounds of a wave")
_add("expand", "exp_n1", lambda rng: {"Ap": np.array([0, 100], np.int32)}, {"n": 1, "blocks": 1}, what="one column")
_add("expand", "exp_grid_full", _exp_short(4 * GRID_MAX), {"wraps": False, "blocks": GRID_MAX}, other="exp_grid_wraps",
     what="4 * EXPAND_GRID_MAX columns: the largest grid, every wave one column")
_add("expand", "exp_grid_wraps", _exp_short(4 * GRID_MAX + 3), {"wraps": True, "blocks": GRID_MAX}, other="exp_grid_full",
     what="three columns more: the first three waves take a second column")
_add("expand", "exp_nnz0", lambda rng: {"Ap": np.zeros(11, np.int32)}, {"nnz": 0}, what="no entries: nothing is launched, col untouched")


# -- the sort without expansion
def _values(rng, n):
    """float64 payloads whose two words both matter: -0.0, +-inf, quiet and signalling NaNs with distinct payloads"""
    v = rng.standard_normal(n)
    special = np.array([0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000001, 0x7ff8000000abcdef,
                        0xfff8000012345678, 0x7ff4000000000001, 0x7ff00000ffffffff], np.uint64).view(np.float64)
    where = np.linspace(0, n - 1, min(n, 3 * len(special))).astype(np.int64)
    v[where] = np.resize(special, len(where))
    return v


def _keys(rng, n, limit):
    """n keys below limit, 0 and limit - 1 among them, every multi-record case with duplicates"""
    pool = max(1, min(limit, n // 3))
    if limit <= pool:
        values = np.arange(limit, dtype=np.uint32)
    else:
        values = np.unique(np.concatenate([[0, limit - 1], rng.integers(0, limit, pool, dtype=np.int64)])).astype(np.uint32)
    key = values[rng.integers(0, len(values), n)]
    if n >= 2 and len(values) >= 2:
        key[[0, -1]] = values[[-1, 0]]
    return key.astype(np.uint32)


def _plain(count, limit, payload, want_key, dist=None, mis=0):
    has_a, has_v = PAYLOADS[payload]

    def make(rng):
        if dist is None:
            key = _keys(rng, count, limit)
        elif dist == "equal":
            key = np.full(count, limit - 2, np.uint32)
        elif dist == "sorted":
            key = np.sort(_keys(rng, count, limit))
        elif dist == "reverse":
            key = np.sort(_keys(rng, count, limit))[::-1].copy()
        elif dist == "runs64":                                  # the clustered last pass the kernel's comments speak of
            key = np.repeat(_keys(rng, -(-count // 64), limit), 64)[:count].copy()
        else:                                                   # only the top digit is used
            assert dist == "top_digit"
            w = digit_widths(key_bits(limit))
            key = (rng.integers(0, 1 << w[-1], count).astype(np.uint32) << np.uint32(sum(w[:-1]))).astype(np.uint32)
        d = {"key": key, "key_limit": limit, "want_key": want_key, "misalign": mis}
        if has_a:
            d["a"] = rng.integers(0, 1 << 32, count, dtype=np.int64).astype(np.uint32)
        if has_v:
            d["v"] = _values(rng, count)
        return d
    return make


GRID_COUNT = 2 * TILE + 904                # "about 5 000": two full tiles and a partial one
KEY_LIMITS = (1, 2, BINS, BINS + 1, BINS * BINS, BINS * BINS + 1, BINS ** 3, BINS ** 3 + 1, 0xFFFFFFFF)
_LIMIT_OTHER = {BINS: BINS + 1, BINS + 1: BINS, BINS * BINS: BINS * BINS + 1, BINS * BINS + 1: BINS * BINS,
                BINS ** 3: BINS ** 3 + 1, BINS ** 3 + 1: BINS ** 3}

for _pay in PAYLOADS:
    for _lim in KEY_LIMITS:
        for _wk in (True, False):
            _nm = lambda lim, pay=_pay, wk=_wk: "sort_%s_lim%d_%s" % (pay, lim, "key" if wk else "nokey")
            _add("sort", _nm(_lim), _plain(GRID_COUNT, _lim, _pay, _wk),
                 {"passes": len(digit_widths(key_bits(_lim))), "widths": digit_widths(key_bits(_lim))},
                 other=_nm(_LIMIT_OTHER[_lim]) if _lim in _LIMIT_OTHER else None,
                 what="%d key bits: digits %s" % (key_bits(_lim), digit_widths(key_bits(_lim))))

_L3 = BINS * BINS + 1                      # 17 key bits: three passes, digits 6 6 5, all four record layouts of a + v
for _tag, _cnt, _oth in (("count1", 1, None), ("tile_m1", TILE - 1, None), ("tile", TILE, "sort_av_tile_p1"), ("tile_p1", TILE + 1, "sort_av_tile")):
    _add("sort", "sort_av_" + _tag, _plain(_cnt, _L3, "av", True), {"nblocks": -(-_cnt // TILE), "count": _cnt}, other=_oth,
         what="%d records" % _cnt)
for _nb in (1, 7, 8, 9, 15):
    _add("sort", "sort_av_blocks%d" % _nb, _plain(_nb * TILE - 37, _L3, "av", True), {"nblocks": _nb, "q": _nb >> 3, "rem": _nb & 7},
         what="tile-to-XCD remap with q = %d, rem = %d" % (_nb >> 3, _nb & 7))
for _tag, _cnt, _nc, _oth in (("tiles64", CHUNK_MIN * TILE, 1, "tiles65"), ("tiles65", CHUNK_MIN * TILE + 1, 2, "tiles64"),
                              ("chunks4", SEGS * CHUNK_MIN * TILE, SEGS, "chunks5"), ("chunks5", SEGS * CHUNK_MIN * TILE + 1, SEGS + 1, "chunks4")):
    _add("sort", "sort_av_" + _tag, _plain(_cnt, _L3, "av", True), {"nchunks": _nc, "chunk": CHUNK_MIN}, other="sort_av_" + _oth,
         what="%d chunk(s) of the digit scan over RS_SEGS = %d segments" % (_nc, SEGS))
_DIST_COUNT = 3 * TILE + 100
for _dist in ("equal", "sorted", "reverse", "runs64"):
    _add("sort", "sort_av_" + _dist, _plain(_DIST_COUNT, _L3, "av", True, dist=_dist), {"passes": 3}, what="keys: " + _dist)
_add("sort", "sort_av_top_digit", _plain(_DIST_COUNT, BINS ** 3, "av", True, dist="top_digit"), {"passes": 3},
     what="keys that use only the top digit: the first two passes move nothing")
for _mis in range(4):
    _add("sort", "sort_av_mis%d" % _mis, _plain(_DIST_COUNT, _L3, "av", True, mis=_mis),
         {"key_misalign": _mis, "hist": {("hist", "vector"), ("hist", "scalar")}}, other="sort_av_mis%d" % (0 if _mis else 1),
         cut="key_misalign", what="key array %d words past a 16-byte boundary" % _mis)
    if _mis:
        _add("sort", "sort_keys_mis%d" % _mis, _plain(_DIST_COUNT, BINS, "keys", True, mis=_mis),
             {"key_misalign": _mis, "hist": {("hist", "scalar")}, "passes": 1}, what="one pass, every tile key by key")
# the argument shapes of the callers
_add("sort", "caller_chol_classes", _plain(GRID_COUNT, 5, "a", True), {"instances": ("a",)}, what="(key, a, -), 5 keys, sorted keys wanted (cs_chol)")
_add("sort", "caller_dmperm_classes", _plain(GRID_COUNT, 5, "a", False), {"instances": ("a",)}, what="(key, a, -), 5 keys, no sorted keys (dmperm)")
_add("sort", "caller_cholsym_values", _plain(GRID_COUNT, 3000, "v", True), {"instances": ("v", "v")}, what="(key, -, v) (cholsym)")
_add("sort", "caller_cholsym_keys", _plain(GRID_COUNT, 3000, "keys", True), {"instances": ("keys", "keys")}, what="(key, -, -) (cholsym)")
_add("sort", "caller_assemble_gaxpy_tiled", _plain(GRID_COUNT, 3000, "av", True), {"instances": ("av_flat_packed", "av_packed_flat")},
     what="(key, a, v) with the sorted keys (assemble, the tiled gaxpy plan)")
_add("sort", "caller_components_cholclique", _plain(GRID_COUNT, 3000, "a", False), {"instances": ("a", "a")},
     what="(key, a, -) without the sorted keys (components, cholclique)")
_add("sort", "sort_empty", _plain(0, 100, "av", True), {"count": 0, "passes": 0}, what="no records: no pass is launched")


# -- the sort with expansion (a transpose)
def _inside(rng, K, distinct):
    """K column starts strictly inside a tile, relative to its base"""
    if distinct:
        return np.sort(rng.choice(np.arange(1, TILE), K, replace=False))
    return np.sort(rng.integers(1, TILE, K))


def _ptr(rels, count, trailing=0):
    """column pointers from the starts of every tile (relative to the tile's base; 0 = on the base), `trailing` empty columns
    at the end"""
    S = np.concatenate([t * TILE + np.asarray(r, np.int64) for t, r in enumerate(rels)] + [np.full(trailing + 1, count, np.int64)])
    assert S[0] == 0 and np.all(np.diff(S) >= 0) and (len(S) < 2 + trailing or S[-2 - trailing] < count)
    return S.astype(np.int32)


def _expand(make_ptr, m, values, short_keys=1, want_key=False, edge_keys=False):
    def make(rng):
        Ap = make_ptr(rng)
        count = int(Ap[-1])
        key = _keys(rng, count, m)
        if edge_keys:          # the first and the last key of every first-pass digit, 0 and m - 1 among them
            w0 = digit_widths(key_bits(m))[0]
            dg = np.arange(1 << w0, dtype=np.int64)
            edges = np.concatenate([dg, ((m - 1 - dg) >> w0 << w0) + dg])
            assert edges.min() == 0 and edges.max() == m - 1 and len(edges) * 2 <= count
            key[rng.choice(count, 2 * len(edges), replace=False)] = np.concatenate([edges, edges]).astype(np.uint32)
        d = {"key": key, "key_limit": m, "want_key": want_key, "expand_ptr": Ap, "nkeys": m, "short_keys": short_keys}
        if values:
            d["v"] = _values(rng, count)
        return d
    return make


_TAIL = 700                                # records of the partial last tile
X_STARTS = (1, DESC // 2 - 3, DESC // 2 - 2, DESC // 2 - 1, DESC, DESC + 1, TILE - 1, TILE, TILE + 1)


def _three_tiles(K, dup=False):
    """a first tile with a few starts, a middle tile with exactly K, a partial last tile; the middle tile's base lies inside a column"""
    return lambda rng: _ptr([np.concatenate([[0], _inside(rng, 10, True)]), _inside(rng, K, K < TILE and not dup),
                             np.sort(rng.integers(1, _TAIL, 3))], 2 * TILE + _TAIL)


def _x_other(K):
    half = DESC // 2 - 2                     # starts whose 16 bits lie in the first half of the descriptor's words
    return {DESC: DESC + 1, DESC + 1: DESC, TILE: TILE + 1, TILE + 1: TILE, half: half + 1, half + 1: half}.get(K)


for _vals in (True, False):
    _sfx = "_v" if _vals else "_pattern"
    for _K in X_STARTS:
        _add("sort", "x_starts%d%s" % (_K, _sfx), _expand(_three_tiles(_K), 1000, _vals), {"K": (10, _K, 3)},
             other="x_starts%d%s" % (_x_other(_K), _sfx) if _x_other(_K) else None, cut="K_branch_or_word",
             what="a tile with K = %d column starts: %s" % (_K, branch_of(_K)))
    _add("sort", "x_empty_run%s" % _sfx, _expand(_three_tiles(3 * TILE, dup=True), 1000, _vals), {"K": (10, 3 * TILE, 3)},
         what="several thousand empty columns inside a tile: the pointer array is searched")
    _add("sort", "x_dups_painted%s" % _sfx, _expand(_three_tiles(DESC - 40, dup=True), 1000, _vals), {"K": (10, DESC - 40, 3)},
         what="empty columns among painted ones: equal starts in the descriptor")
    _add("sort", "x_long_column%s" % _sfx, _expand(lambda rng: _ptr([[0, 100, TILE - 5]] + [[]] * 5 + [[40, 300]], 6 * TILE + _TAIL), 1000, _vals),
         {"K": (2, 0, 0, 0, 0, 0, 2)}, what="one column over five whole tiles: K = 0")
    _add("sort", "x_base_start%s" % _sfx, _expand(lambda rng: _ptr([[0, 50], [0, 10, 900], [0]], 2 * TILE + _TAIL), 1000, _vals),
         {"K": (1, 2, 0)}, what="a column starts exactly on a tile base, none empty before it")
    _add("sort", "x_base_start_after_empties%s" % _sfx,
         _expand(lambda rng: _ptr([[0, 50], [0] * 6 + [10, 900], [0, 0, 0, 5]], 2 * TILE + _TAIL), 1000, _vals),
         {"K": (1, 2, 1)}, what="empty columns on a tile base, then the column that starts there")
    _add("sort", "x_empties_front_end%s" % _sfx,
         _expand(lambda rng: _ptr([[0] * 9 + [300], [77]], TILE + _TAIL, trailing=11), 1000, _vals),
         {"K": (1, 1)}, what="empty columns at the very front and at the very end")
    _add("sort", "x_one_column%s" % _sfx, _expand(lambda rng: _ptr([[0]], 2 * TILE + 17), 1000, _vals), {"K": (0, 0, 0)},
         what="expand_n = 1")


def _random_columns(n, count):
    def make(rng):
        cols = np.sort(rng.integers(n // 10, n - n // 20, count))          # empty columns in front and at the end
        return np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int32)
    return make


# short keys: 17 .. 24 key bits, values, pointers wanted, no sorted keys, at most 2^(32 - w0) columns
for _bits, _m in ((17, BINS * BINS + 1), (24, BINS ** 3)):
    for _sk in (1, 0):
        _add("sort", "x_short%d_%s" % (_bits, "on" if _sk else "off"), _expand(_random_columns(400, GRID_COUNT), _m, True, _sk, edge_keys=True),
             {"k16": _sk, "bits": _bits}, other="x_short%d_%s" % (_bits, "off" if _sk else "on"),
             what="sort.short_keys = %d at %d key bits" % (_sk, _bits))
_add("sort", "x_bits16", _expand(_random_columns(400, GRID_COUNT), BINS * BINS, True), {"k16": 0, "passes": 2}, other="x_short17_on",
     what="16 key bits: two passes, no short keys")
_add("sort", "x_bits25", _expand(_random_columns(400, GRID_COUNT), BINS ** 3 + 1, True), {"k16": 0, "passes": 4}, other="x_short24_on",
     what="25 key bits: four passes, no short keys")
_add("sort", "x_short_pattern", _expand(_random_columns(400, GRID_COUNT), _L3, False), {"k16": 0, "passes": 3}, other="x_short17_on",
     what="no values: no packed records, no short keys")
_add("sort", "x_short_with_keys", _expand(_random_columns(400, GRID_COUNT), _L3, True, want_key=True), {"k16": 0, "passes": 3},
     other="x_short17_on", what="the sorted keys wanted: no short keys")
_M22 = 1 << 22                             # 22 key bits: digits 8 7 7, so the column must fit 24 bits
_W0 = digit_widths(22)[0]
_add("sort", "x_columns_fit", _expand(_random_columns(1 << (32 - _W0), GRID_COUNT), _M22, True), {"k16": 1, "w0_columns": 0},
     other="x_columns_one_more", what="2^(32 - w0) columns: the largest column still fits beside the first digit")
_add("sort", "x_columns_one_more", _expand(_random_columns((1 << (32 - _W0)) + 1, GRID_COUNT), _M22, True), {"k16": 0, "w0_columns": -1},
     other="x_columns_fit", what="one column more: 32-bit keys")

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = {prim: [c.name for c in CASES if c.prim == prim] for prim in ("scan", "sufmin", "boundaries", "expand", "sort")}


def differs(name, other):
    """the fact by which a case and its neighbour lie on two sides of a cut"""
    a, b, cut = facts(name), facts(other), BY_NAME[name].cut
    if cut == "K_branch_or_word":
        Ka, Kb = a["K"][1], b["K"][1]
        # two branches of the expansion, or the last start in the first / second half of the descriptor's words (two registers)
        return branch_of(Ka) != branch_of(Kb) or desc_half_of_last_start(Ka) != desc_half_of_last_start(Kb)
    return a[cut] != b[cut]
