"""Constructed inputs for cs_multiply on the device (csx_spgemm.hip), one named case per accumulator bin, table and staging
edge, and a Python model of what multiply_device and the ordered pass decide.  TEST INFRASTRUCTURE, NOT PRODUCT.

Every size comes from the library's own constants (`_csx.spgemm_limits()`, no device needed), never from a literal.  A case
names the `edge` it sits on: facts (`facts`) the model must give for it; where the edge has another side the neighbour is a
column of the same matrix and the edge holds both.  tests/test_spgemm_cases_cpu.py holds the table to these claims without a
device; tests/test_gpu_multiply_edges.py runs every case, compares C with the plain-C oracle and csx_spgemm_info with `model`
field for field.

The model: `column_bins` (k_sg_products: products, longest named column of A, bin), `slots_one_pass` / `slots_two_pass`,
`hash_two_pass` / `hash_one_pass` / `hash_ordered` with `insert` (linear probing as the kernels wrap it), `one_pass_grid`,
`model` (the whole info vector as _csx.spgemm_info returns it).

`tables(cus)` builds the cases for a device of `cus` compute units: the hand-over cases need more columns in a bin than the
persistent grids hold workgroups, which depends on it.  What no case reaches is listed in NOT_REACHED with the reason."""
import collections
import functools
import math
from fractions import Fraction

import numpy as np

import _csx

LIM = _csx.spgemm_limits()
SEG, THREADS, DENSE_MAX, GLOBAL_WGS, HASH_MAXP = (LIM[k] for k in ("SG_SEG", "SG_THREADS", "SG_DENSE_MAX", "SG_GLOBAL_WGS",
                                                                   "SG_HASH_MAXP"))
NHASH, NNARROW = LIM["SG_HASH_BINS"], LIM["SG_NARROW_BINS"]
HASH_LIMIT = tuple(LIM["HASH_LIMIT%d" % b] for b in range(NHASH))
H2_MAXSEG, H2_MAXLEN, H2_MAXP, H1_SEG, H1_MAXP, H1_UN = (LIM[k] for k in ("H2_MAXSEG", "H2_MAXLEN", "H2_MAXP", "H1_SEG", "H1_MAXP",
                                                                          "H1_UN"))
SGO_MAX, DENSE_WAVES, GRID_PER_CU, UN = LIM["SGO_MAX"], LIM["SGO_DENSE_WAVES"], LIM["SG_GRID_PER_CU"], LIM["SG_UN"]
ORD_CLASSES = tuple((LIM["SGO_SLOTS%d" % c], LIM["SGO_CNT%d" % c], LIM["SGO_WAVES%d" % c]) for c in range(3))
MIN_SLOTS, LDS_BUDGET, WGS_PER_CU_MAX = LIM["SG_MIN_SLOTS"], LIM["SG_LDS_BUDGET"], LIM["SG_WGS_PER_CU_MAX"]
STEP = UN * THREADS                       # products a step of the two-pass kernel takes
BIN_DENSE, BIN_HASH0, BIN_NARROW0, BIN_GLOBAL, BIN_EMPTY, NBINS = 0, 1, 1 + NHASH, 1 + NHASH + NNARROW, 31, 32
TOO_BIG = 0xFFFFFFF0                      # a column with more products than this is refused
GOLDEN = 0x9E3779B1
M_HASH = DENSE_MAX + 1                    # the smallest m on the hash side
M_CHAIN = 65536

NOT_REACHED = {
    "P just below 2^32": "a column with 2^32 - 16 products or fewer that is not refused needs some 4e9 products to be walked: "
                         "minutes, not seconds; the refusal on the other side of that cut is the case `too-big`",
    "more than 2^31 entries in C": "the int32 overflow message of multiply_device needs 2^31 entries of C: 24 GB of results",
    "more than 2^31 products over the hash bins": "big[1] >= 0x7FFFFFF0 turns the one-pass path off: 2^31 products in columns of "
                                                  "at most SG_HASH_MAXP each are half a million columns of B and 2^31 products of work",
    "the memory-pressure fallback from one-pass": "needs the device nearly full (12 bytes a product against a third of the free "
                                                  "memory); a test cannot arrange that without holding the memory of a shared machine",
}


# ---- the model ----------------------------------------------------------------------------------------------------------------
def column_bins(m, Ap, Bp, Bi):
    """k_sg_products: per column of B the products P, the longest column of A it names, its entries, its bin"""
    Ap, Bp, Bi = (np.asarray(v, np.int64) for v in (Ap, Bp, Bi))
    alen = np.diff(Ap)
    n = len(Bp) - 1
    P, maxlen, bins = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j in range(n):
        ln = alen[Bi[Bp[j]:Bp[j + 1]]]
        P[j] = int(ln.sum())
        maxlen[j] = int(ln.max()) if ln.size else 0
        if P[j] == 0:
            bins[j] = BIN_EMPTY
        elif m <= DENSE_MAX:
            bins[j] = BIN_DENSE
        elif P[j] > HASH_MAXP:
            bins[j] = BIN_GLOBAL
        else:
            hb = 0
            while HASH_LIMIT[hb] < P[j]:
                hb += 1
            narrow = Bp[j + 1] - Bp[j] <= H2_MAXSEG and maxlen[j] <= H2_MAXLEN and P[j] <= H2_MAXP
            bins[j] = (BIN_NARROW0 if narrow else BIN_HASH0) + hb
    return P, maxlen, np.diff(Bp), bins


def slots_one_pass(hb):
    return HASH_LIMIT[hb] * 3 // 2


def slots_two_pass(hb):
    s = MIN_SLOTS
    while s < 2 * HASH_LIMIT[hb]:
        s <<= 1
    return s


def _mix(rows):
    return (np.asarray(rows, np.uint64) * np.uint64(GOLDEN)) & np.uint64(0xFFFFFFFF)


def hash_two_pass(rows, slots):
    """acc_slot / acc_find: the top log2(slots) bits of row * GOLDEN in 32 bits; the probe wraps by & (slots - 1)"""
    assert slots & (slots - 1) == 0
    return (_mix(rows) >> np.uint64(32 - (slots.bit_length() - 1))).astype(np.int64)


def hash_one_pass(rows, slots):
    """h1_insert / h2_insert: __umulhi(row * GOLDEN, slots); the probe wraps by s + 1 == slots ? 0 : s + 1"""
    return ((_mix(rows) * np.uint64(slots)) >> np.uint64(32)).astype(np.int64)


hash_ordered = hash_one_pass              # sgo_slot<SLOTS>: the same high half, of a compile-time table size


def insert(rows, slots, home):
    """linear probing of distinct rows in the given order: {row: slot}; every kernel wraps from the last slot to slot 0"""
    table, where = {}, {}
    for r, s in zip(rows, home(np.asarray(rows), slots).tolist()):
        if r in where:
            continue
        while s in table:
            s = 0 if s + 1 == slots else s + 1
        table[s] = r
        where[r] = s
    return where


def _per_cu(lds):
    return max(1, min(WGS_PER_CU_MAX, LDS_BUDGET // (lds + 256)))


def one_pass_grid(kernel, slots, values, ncols, cus):
    """launch_hash1 / launch_hash2: the workgroups that are resident at once, at most one per column"""
    even = slots + (slots & 1)
    if kernel == 1:
        lds = even * (16 if values else 8) + H1_SEG * (8 + 4 + 4 + 4) + (H1_MAXP // 32) * 8 + 64 + (slots * 2 // 3) * 2 + 16
    else:
        lds = even * (16 if values else 8) + H2_MAXSEG * 4 + 64
    return min(ncols, cus * _per_cu(lds))


def ordered_class(cnt):
    for c, (_, maxcnt, _) in enumerate(ORD_CLASSES):
        if cnt <= maxcnt:
            return c
    return 3


def model(m, k, n, Ap, Bp, Bi, values, cus, one_pass=True, ordered=False, Cp=None):
    """what _csx.spgemm_info() reports after the product of an m x k and a k x n matrix with these patterns; Cp: the column
    pointers of C (asked for only with ordered)"""
    info = {"bins": (0,) * NBINS, "one_pass": 0, "global_wgs": 0, "cus": cus, "ordered": 0, "classes": (0, 0, 0, 0),
            "launches": {}, "grids": {}}

    def ran(site, grid):
        info["launches"][site] = info["launches"].get(site, 0) + 1
        info["grids"][site] = grid

    if n == 0 or m == 0 or int(Ap[-1]) == 0 or int(Bp[-1]) == 0:
        return info
    P, _, _, bins = column_bins(m, Ap, Bp, Bi)
    cnt = np.bincount(bins, minlength=NBINS)
    info["bins"] = tuple(int(c) for c in cnt)
    ran("products", (n + 3) // 4)
    if (P > TOO_BIG).any():
        return info
    hashed = range(BIN_HASH0, BIN_GLOBAL)
    nhash = int(sum(cnt[b] for b in hashed))
    hprod = int(sum(P[j] for j in range(n) if bins[j] in hashed))
    onep = bool(nhash > 0 and hprod < 0x7FFFFFF0 and one_pass)
    info["one_pass"] = int(onep)
    v = "values" if values else "pattern"
    if onep:
        for hb in range(NHASH):
            if cnt[BIN_HASH0 + hb]:
                ran("hash1_%s_%d" % (v, hb), one_pass_grid(1, slots_one_pass(hb), values, int(cnt[BIN_HASH0 + hb]), cus))
        for hb in range(NNARROW):
            if cnt[BIN_NARROW0 + hb]:
                ran("hash2_%s_%d" % (v, hb), one_pass_grid(2, slots_one_pass(hb), values, int(cnt[BIN_NARROW0 + hb]), cus))
    if cnt[BIN_GLOBAL]:
        info["global_wgs"] = int(min(cnt[BIN_GLOBAL], GLOBAL_WGS))
    if onep:
        ran("compact", (nhash + 3) // 4)           # (enqueued between the two runs of the bins; the counters keep no order)
    for run in ("symbolic", v):
        if cnt[BIN_DENSE]:
            ran("spgemm_%s_dense" % run, int(min(cnt[BIN_DENSE], cus * GRID_PER_CU)))
        if not onep:
            for b in hashed:
                if cnt[b]:
                    ran("spgemm_%s_hash" % run, int(min(cnt[b], cus * GRID_PER_CU)))
        if cnt[BIN_GLOBAL]:
            ran("spgemm_%s_global" % run, int(min(cnt[BIN_GLOBAL], GLOBAL_WGS)))
    if ordered and values and Cp is not None and int(Cp[-1]) > 0:
        info["ordered"] = 1
        ran("dup_cols", (k + 3) // 4)
        cls = [0, 0, 0, 0]
        for c in np.diff(np.asarray(Cp, np.int64)).tolist():
            if c:
                cls[ordered_class(c)] = 1
        info["classes"] = tuple(cls)
        for c in range(3):
            if cls[c]:
                ran("ordered2_%d" % c, min(n, cus * ORD_CLASSES[c][2]))
        if cls[3]:
            ran("ordered_dense", min(n, DENSE_WAVES))
    return info


# ---- building blocks ------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name family m k n Ap Ai Bp Bi edge two_pass_too note")


class Build:
    """columns of A (lists of rows, in storage order) and of B (lists of columns of A), then CSC arrays"""

    def __init__(self, m, seed):
        self.m, self.A, self.B = m, [], []
        self.rng = np.random.default_rng(seed)
        self.perm = self.rng.permutation(m)

    def rows(self, count, start=0):
        """count distinct rows, unsorted: a stretch of one fixed permutation of 0 .. m-1 (stretches that overlap share rows)"""
        assert count <= self.m
        idx = (start + np.arange(count)) % self.m
        return self.perm[idx].tolist()

    def a(self, rows):
        self.A.append([int(r) for r in rows])
        return len(self.A) - 1

    def a_split(self, rows, lens):
        """the rows dealt to consecutive new columns of A of the given lengths"""
        assert sum(lens) == len(rows)
        ids, at = [], 0
        for ln in lens:
            ids.append(self.a(rows[at:at + ln]))
            at += ln
        return ids

    def b(self, cols):
        self.B.append([int(c) for c in cols])
        return len(self.B) - 1

    def case(self, name, family, edge, two_pass_too=None, note=""):
        m, k, n = self.m, len(self.A), len(self.B)
        Ap = np.zeros(k + 1, np.int32)
        Ap[1:] = np.cumsum([len(c) for c in self.A])
        Bp = np.zeros(n + 1, np.int32)
        Bp[1:] = np.cumsum([len(c) for c in self.B])
        Ai = np.asarray([r for c in self.A for r in c], np.int32)
        Bi = np.asarray([r for c in self.B for r in c], np.int32)
        assert (Ai >= 0).all() and (Ai < m).all() and (Bi >= 0).all() and (Bi < max(k, 1)).all()
        if two_pass_too is None:
            two_pass_too = m > DENSE_MAX
        return Case(name, family, m, k, n, Ap, Ai, Bp, Bi, edge, two_pass_too, note)


def split(total, piece):
    """total as pieces of `piece` and a last shorter one"""
    out = [piece] * (total // piece)
    if total % piece:
        out.append(total % piece)
    return out


def general_lens(P):
    """lengths of columns of A with P entries in all, the first of H2_MAXLEN + 1: one too long for a narrow column"""
    assert P > H2_MAXLEN
    return [H2_MAXLEN + 1] + split(P - H2_MAXLEN - 1, 97)


def narrow_lens(P):
    lens = split(P, H2_MAXLEN)
    assert len(lens) <= H2_MAXSEG
    return lens


def values_for(case, kind):
    """(Ax, Bx): "dyadic" = non-zero integers in [-8, 8] times 2^-3, every product and partial sum exact; "mixed" = uniform
    in (-1, 1)"""
    rng = np.random.default_rng([len(case.name), sum(map(ord, case.name)), 0 if kind == "dyadic" else 1])
    out = []
    for cnt in (len(case.Ai), len(case.Bi)):
        if kind == "dyadic":
            out.append(rng.integers(1, 9, size=cnt) * rng.choice([-1.0, 1.0], size=cnt) / 8.0)
        else:
            x = rng.uniform(-1.0, 1.0, size=cnt)
            x[x == 0.0] = 0.5
            out.append(x)
    return out[0], out[1]


# ---- facts of a case, by the model ----------------------------------------------------------------------------------------------
def first_touch(case):
    """(Cp, Ci, per entry the number of products) in the reference's order, in plain Python"""
    Cp, Ci, terms = [0], [], []
    Ap, Ai, Bp, Bi = case.Ap.tolist(), case.Ai.tolist(), case.Bp.tolist(), case.Bi.tolist()
    for j in range(case.n):
        seen = {}
        for p in range(Bp[j], Bp[j + 1]):
            c = Bi[p]
            for r in Ai[Ap[c]:Ap[c + 1]]:
                if r in seen:
                    terms[seen[r]] += 1
                else:
                    seen[r] = len(Ci)
                    Ci.append(r)
                    terms.append(1)
        Cp.append(len(Ci))
    return np.asarray(Cp, np.int64), np.asarray(Ci, np.int64), np.asarray(terms, np.int64)


def facts(case):
    P, maxlen, blen, bins = column_bins(case.m, case.Ap, case.Bp, case.Bi)
    Cp, _, _ = first_touch(case)
    alen = np.diff(case.Ap.astype(np.int64))
    seg = lambda j, S: [int(alen[case.Bi[s0:min(s0 + S, case.Bp[j + 1])]].sum()) for s0 in range(case.Bp[j], case.Bp[j + 1], S)]
    return {"P": P.tolist(), "maxlen": maxlen.tolist(), "blen": blen.tolist(), "bins": bins.tolist(),
            "cnt": np.diff(Cp).tolist(), "alen": alen.tolist(), "m": case.m, "k": case.k, "n": case.n,
            "seg_products": lambda j: seg(j, SEG), "h1_seg_products": lambda j: seg(j, H1_SEG),
            "classes": sorted({ordered_class(c) for c in np.diff(Cp).tolist() if c}),
            "col_class": [ordered_class(c) for c in np.diff(Cp).tolist()]}


def exact_entries(case, Ax, Bx):
    """per entry of C in first-touch order: (the exact sum of its products, the exact sum of their magnitudes, their number),
    the first two as fractions.Fraction over the float64 inputs"""
    def scaled(x):                           # x = mant * 2^exp exactly, mant an integer of at most 53 bits
        mant, exp = np.frexp(np.asarray(x, np.float64))
        return (mant * 2.0 ** 53).astype(np.int64).tolist(), (exp.astype(np.int64) - 53).tolist()
    am, ae = scaled(Ax)
    bm, be = scaled(Bx)
    emin = (min(ae) if ae else 0) + (min(be) if be else 0)
    Ap, Ai, Bp, Bi = case.Ap.tolist(), case.Ai.tolist(), case.Bp.tolist(), case.Bi.tolist()
    sums, mags, terms = [], [], []
    for j in range(case.n):
        seen = {}
        for p in range(Bp[j], Bp[j + 1]):
            c, mb, eb = Bi[p], bm[p], be[p]
            for q in range(Ap[c], Ap[c + 1]):
                t = (am[q] * mb) << (ae[q] + eb - emin)
                r = Ai[q]
                e = seen.get(r)
                if e is None:
                    seen[r] = len(sums)
                    sums.append(t)
                    mags.append(abs(t))
                    terms.append(1)
                else:
                    sums[e] += t
                    mags[e] += abs(t)
                    terms[e] += 1
    unit = Fraction(2) ** emin
    return [Fraction(s) * unit for s in sums], [Fraction(s) * unit for s in mags], terms


U = Fraction(1, 2 ** 53)


def gamma(c):
    """the textbook bound of c rounded products and c - 1 rounded additions in any order: c u / (1 - c u)"""
    return c * U / (1 - c * U)


def within_bound(x, exact, mag, c):
    """|x - exact| <= gamma_c * sum|a b| + ulp(exact) / 2, in exact arithmetic; also the ratio |x - exact| / (gamma_c sum|a b|)"""
    err = abs(Fraction(x) - exact)
    g = gamma(c) * mag
    half_ulp = Fraction(math.ulp(float(exact))) / 2
    return err <= g + half_ulp, (float(err / g) if g else 0.0)


# ---- the case families -------------------------------------------------------------------------------------------------------
def _bins_cases():
    out = []
    for hb, L in enumerate(HASH_LIMIT):
        for form in ("general", "narrow"):
            if form == "narrow" and L > H2_MAXP:
                continue
            for rows in ("distinct", "same-row"):
                g = Build(M_HASH, 100 + hb)
                cols = []
                for P in (L, L + 1):
                    r = g.rows(P, start=7 * P) if rows == "distinct" else [g.rows(1, start=P)[0]] * P
                    if form == "general":
                        lens = general_lens(P)
                    elif P <= H2_MAXP:
                        lens = narrow_lens(P)
                    else:                                    # P = H2_MAXP + 1: 63 columns of 32 and the last of 33 entries
                        lens = narrow_lens(P - 1)[:-1] + [H2_MAXLEN + 1]
                    cols.append(g.a_split(r, lens))
                empty_a = g.a([])
                g.b(cols[0])
                g.b([])                                      # an empty column of B
                g.b([empty_a, empty_a])                      # a column of B that names only an empty column of A
                g.b(cols[1])
                base = BIN_NARROW0 if form == "narrow" else BIN_HASH0
                over = (BIN_GLOBAL if hb == NHASH - 1 else
                        BIN_HASH0 + hb + 1 if (form == "general" or L + 1 > H2_MAXP) else BIN_NARROW0 + hb + 1)
                edge = {"P": [L, 0, 0, L + 1], "bins": [base + hb, BIN_EMPTY, BIN_EMPTY, over],
                        "cnt": [L, 0, 0, L + 1] if rows == "distinct" else [1, 0, 0, 1]}
                out.append(g.case("bin%d-%s-%s" % (hb, form, rows), "bins", edge))
    # the narrow cuts: H2_MAXSEG | + 1 entries of B, H2_MAXLEN | + 1 entries of the longest column of A, P = H2_MAXP as 64 x 32
    g = Build(M_HASH, 120)
    ones = [g.a(g.rows(1, start=c)) for c in range(H2_MAXSEG + 1)]
    g.b(ones[:H2_MAXSEG])
    g.b(ones)
    out.append(g.case("narrow-cut-entries", "bins", {"blen": [H2_MAXSEG, H2_MAXSEG + 1], "bins": [BIN_NARROW0, BIN_HASH0]}))
    g = Build(M_HASH, 121)
    g.b([g.a(g.rows(H2_MAXLEN, start=5)), g.a(g.rows(3, start=50))])
    g.b([g.a(g.rows(H2_MAXLEN + 1, start=9)), g.a(g.rows(2, start=60))])
    out.append(g.case("narrow-cut-length", "bins", {"maxlen": [H2_MAXLEN, H2_MAXLEN + 1], "bins": [BIN_NARROW0, BIN_HASH0]}))
    g = Build(M_HASH, 122)
    full = [g.a(g.rows(H2_MAXLEN, start=29 * c)) for c in range(H2_MAXSEG)]
    g.b(full)
    g.b(full[:-1] + [g.a(g.rows(H2_MAXLEN + 1, start=3))])
    hb = HASH_LIMIT.index(H2_MAXP)
    out.append(g.case("narrow-cut-products", "bins", {"P": [H2_MAXSEG * H2_MAXLEN, H2_MAXP + 1], "blen": [H2_MAXSEG, H2_MAXSEG],
                                                      "bins": [BIN_NARROW0 + hb, BIN_HASH0 + hb + 1]}))
    # m = SG_DENSE_MAX | + 1 with the same pattern of A
    for m in (DENSE_MAX, DENSE_MAX + 1):
        g = Build(DENSE_MAX, 123)                            # (rows below SG_DENSE_MAX either way)
        g.m = m
        big = g.a_split(g.rows(HASH_MAXP + 40, start=11), general_lens(HASH_MAXP + 40))
        small = g.a_split(g.rows(300, start=4000), general_lens(300))
        g.b(big)
        g.b(small)
        g.b([small[0], small[0]])
        kind = [BIN_DENSE] * 3 if m <= DENSE_MAX else [BIN_GLOBAL, BIN_HASH0 + 1, BIN_HASH0]
        out.append(g.case("dense-cut-m%d" % m, "bins", {"m": m, "bins": kind, "P": [HASH_MAXP + 40, 300, 2 * H2_MAXLEN + 2]}))
    return out


def _narrow_cases():
    g = Build(M_HASH, 200)
    acols = [g.a(g.rows(ln, start=13 * ln)) for ln in range(H2_MAXLEN + 1)]          # lengths 0 .. 32
    dup = g.a([5, 9, 5, 5, 700, 9])                                                  # duplicate rows inside a column of A
    for ln in range(1, H2_MAXSEG + 1):                                               # columns of B of every length 1 .. 64
        ids = [acols[(3 * ln + 5 * t) % len(acols)] for t in range(ln)]
        if ln % 4 == 0:
            ids[0] = ids[-1] = dup                                                   # the same column of A twice
        if ln % 8 == 3:
            ids[ln // 2] = dup
        g.b(ids)
    P, _, _, bins = column_bins(g.m, np.cumsum([0] + [len(c) for c in g.A]), np.cumsum([0] + [len(c) for c in g.B]),
                                [c for col in g.B for c in col])
    assert (bins >= BIN_NARROW0).all() and (bins < BIN_GLOBAL).all()
    return [g.case("narrow-every-length", "narrow", {"blen": list(range(1, H2_MAXSEG + 1)),
                                                     "alen": list(range(H2_MAXLEN + 1)) + [6]})]


def _h1_cases():
    out = []
    g = Build(M_HASH, 300)
    wide = g.a(g.rows(H2_MAXLEN + 1, start=1))                                       # keeps a column out of the narrow bins
    short = [g.a(g.rows(1 + c % 7, start=17 * c)) for c in range(40)]                # 1 .. 7 entries: P stays <= SG_HASH_MAXP
    blens = [1, 8, 9, 32, 33, H1_SEG - 1, H1_SEG, H1_SEG + 1, 2 * H1_SEG, 2 * H1_SEG + 1]
    for bl in blens:
        g.b([wide] + [short[(bl + 3 * t) % len(short)] for t in range(bl - 1)])
    out.append(g.case("h1-b-lengths", "hash1", {"blen": blens}))
    g = Build(M_HASH, 301)
    alens = [0, 1, 31, 32, 33, 63, 64, 65, 97]
    ac = [g.a(g.rows(ln, start=101 * i)) for i, ln in enumerate(alens)]
    for i in range(len(alens)):
        g.b([ac[4]] + ac[i:] + ac[:i])                                               # every length first, last and in between
    twice = g.rows(70, start=900)
    for pos in (0, 5, 31):
        twice[pos + 32] = twice[pos]                                                 # the same row at positions g and g + 32
    g.b([g.a(twice), ac[1]])
    out.append(g.case("h1-a-lengths", "hash1", {"alen": alens + [70]}))
    g = Build(M_HASH, 302)
    ones = [g.a(g.rows(2, start=2 * c)) for c in range(H1_SEG)]
    wide = g.a(g.rows(H2_MAXLEN + 1, start=3000))
    zero = g.a([])
    g.b([zero, wide] + ones[:20])                                                    # a zero-length column of A named first
    g.b([wide] + ones[:20] + [zero])                                                 # named last
    g.b([wide] + ones[:H1_SEG - 1] + [zero] * H1_SEG + ones[5:9])                    # a whole middle segment of them
    g.b([zero] * 3 + [wide] + ones[:H1_SEG - 5] + [zero, zero] + ones[:3] + [zero])  # first / last in a segment, ties in seg_off
    out.append(g.case("h1-zero-lengths", "hash1", {"blen": [22, 22, 2 * H1_SEG + 4, H1_SEG + 5]}))
    return out


def _two_pass_staging(m, name, seed):
    """columns of B whose staging sits on the cuts of the two-pass kernel, for any m (the kind follows from m and the option)"""
    g = Build(m, seed)
    span = min(m, 4000)
    one = [g.a(g.rows(1, start=c % span)) for c in range(70)]                        # columns of one entry
    zero = g.a([])
    blens = [1, 63, 64, 65, SEG - 1, SEG, SEG + 1, 2 * SEG + 1]
    for bl in blens:
        g.b([one[(bl + 3 * t) % len(one)] for t in range(bl)])
    # segments of STEP - 1, STEP and STEP + 1 products (a segment of SG_SEG entries of one entry each, the last of them of 0 / 1 /
    # 2 entries), then one of zero products between two live ones
    two = g.a(g.rows(min(2, m), start=77 % span)) if m >= 2 else one[0]
    for last in (zero, one[3], two):
        g.b([one[(5 * t) % len(one)] for t in range(SEG - 1)] + [last] + [one[1]])
    g.b([one[t % len(one)] for t in range(SEG)] + [zero] * SEG + [one[9], one[10]])
    # leading and trailing zero-length columns in a segment
    g.b([zero, zero] + [one[t % len(one)] for t in range(SEG - 4)] + [zero, zero] + [zero, one[2], zero])
    edge = {"blen": blens + [SEG + 1] * 3 + [2 * SEG + 2, SEG + 3]}
    return g.case(name, "two-pass", edge, two_pass_too=m > DENSE_MAX)


def _two_pass_cases():
    out = [_two_pass_staging(m, "staging-dense-m%d" % m, 400 + i) for i, m in enumerate((1, 2, DENSE_MAX - 1, DENSE_MAX))]
    out.append(_two_pass_staging(M_HASH, "staging-hash", 410))
    # the global kind: more than SG_HASH_MAXP products, over more than two segments and with an idle one between
    g = Build(M_HASH, 411)
    four = [g.a(g.rows(4, start=31 * c)) for c in range(90)]
    zero = g.a([])
    g.b([four[t % len(four)] for t in range(SEG + 5)])
    g.b([four[(7 * t) % len(four)] for t in range(SEG)] + [zero] * SEG + [four[1], zero, four[2]])
    g.b([zero] + [four[(3 * t) % len(four)] for t in range(SEG - 2)] + [zero] + [four[(5 * t) % len(four)] for t in range(40)])
    out.append(g.case("staging-global", "two-pass", {"bins": [BIN_GLOBAL] * 3, "blen": [SEG + 5, 2 * SEG + 3, SEG + 40]}))
    return out


def _handover_windows(ncols, G, length, ring):
    """per column a window (start, length) on a ring of `ring` rows: the columns a workgroup of a grid of G takes one after
    the other (j, j + G, j + 2 G, ...) share half of the shorter of the two windows, at least one row, and never all of either"""
    out = []
    for j in range(ncols):
        L = length(j)
        if j < G:
            start = (7 * j) % ring
        else:
            s0, L0 = out[j - G]
            shared = max(1, min(L0, L) // 2)
            assert 0 < shared < min(L0, L) and L0 + L - shared < ring
            start = (s0 + L0 - shared) % ring
        out.append((start, L))
    return out


def _handover_cases(cus):
    out = []
    # narrow bin 0: 3 G + 2 columns, alternately of 1 and of H2_MAXSEG entries of B (on a workgroup too, which takes columns
    # j, j + G, j + 2 G, ...); the one entry names a column of A of two rows, one of them the predecessor's
    G = cus * _per_cu((slots_one_pass(0) + (slots_one_pass(0) & 1)) * 16 + H2_MAXSEG * 4 + 64)
    g = Build(M_HASH, 500)
    R = 2 * H2_MAXSEG
    ring = g.rows(R)
    one = [g.a([ring[c]]) for c in range(R)]
    two = [g.a([ring[c], ring[(c + 1) % R]]) for c in range(R)]
    n = 3 * G + 2
    for start, L in _handover_windows(n, G, lambda j: 2 if (j + j // G) % 2 == 0 else H2_MAXSEG, R):
        g.b([two[start]] if L == 2 else [one[(start + t) % R] for t in range(L)])
    out.append(g.case("handover-narrow", "hand-over", {"n": n, "bins": [BIN_NARROW0] * n, "grid": ("hash2", 0, G),
                                                       "blen": [1 if (j + j // G) % 2 == 0 else H2_MAXSEG for j in range(n)]}))
    # general hash bin 0: 2 G + 2 columns, each with one column of A of H2_MAXLEN + 1 entries, first or last, of alternating shape
    G = one_pass_grid(1, slots_one_pass(0), True, 1 << 30, cus)
    g = Build(M_HASH, 501)
    R, W = 120, H2_MAXLEN + 1
    ring = g.rows(R)
    one = [g.a([ring[c]]) for c in range(R)]
    wide = [g.a([ring[(c + t) % R] for t in range(W)]) for c in range(R)]
    n = 2 * G + 2
    for start, L in _handover_windows(n, G, lambda j: W + 1 if (j + j // G) % 2 == 0 else W + 9, R):
        if L == W + 1:
            g.b([wide[start], one[(start + W) % R]])
        else:
            g.b([one[(start + t) % R] for t in range(9)] + [wide[(start + 9) % R]])
    out.append(g.case("handover-general", "hand-over", {"n": n, "bins": [BIN_HASH0] * n, "grid": ("hash1", 0, G)}))
    # the two-pass kernel: 2 x grid + 1 columns through the dense kind (m ~ 100) and through the hash kind
    grid = cus * GRID_PER_CU
    for m, nm in ((101, "dense"), (M_HASH, "two-pass-hash")):
        g = Build(m, 502)
        R = 96
        ring = g.rows(R)
        one = [g.a([ring[c]]) for c in range(R)]
        three = [g.a([ring[(c + t) % R] for t in range(3)]) for c in range(R)]
        n = 2 * grid + 1
        for start, L in _handover_windows(n, grid, lambda j: 4 + 3 * ((j + j // grid) % 3), R):
            g.b([three[(start + 3 * t) % R] for t in range(L // 3)] + [one[(start + L - 1) % R]])
        out.append(g.case("handover-" + nm, "hand-over", {"n": n, "grid": ("spgemm", 0 if m <= DENSE_MAX else 1, grid)}))
    return out


def column_rows(case, j):
    """the set of rows the products of column j of C fall on"""
    return {int(r) for c in case.Bi[case.Bp[j]:case.Bp[j + 1]] for r in case.Ai[case.Ap[c]:case.Ap[c + 1]]}


def _global_reuse_cases():
    g = Build(M_HASH, 600)
    width, count = 64, 160
    ac = [g.a(g.rows(width, start=51 * c)) for c in range(count)]                  # stretches of 64 rows, 13 shared with the next
    tails = [g.a(g.rows(t, start=4000 + 9 * t)) for t in range(1, 65)]
    ncols = 2 * GLOBAL_WGS + 2
    per = HASH_MAXP // width
    for c in range(ncols):
        start = (5 * c + (c // GLOBAL_WGS) * (per // 2)) % count                     # column c + 64: half of column c's window
        win = [ac[(start + t) % count] for t in range(per)]
        rot = (11 * c) % per                                                         # shared rows first met at other product numbers
        g.b(win[rot:] + win[:rot] + [tails[c % 64]])
    edge = {"n": ncols, "bins": [BIN_GLOBAL] * ncols, "P": [HASH_MAXP + 1 + c % 64 for c in range(ncols)]}
    return [g.case("global-reuse", "global-reuse", edge)]


@functools.lru_cache(maxsize=None)
def chain_rows(slots, which, count=24, m=M_CHAIN):
    """the first `count` rows below m whose home in a table of `slots` is one of its last 8 slots, then 3 whose home is slot 0"""
    home = (hash_two_pass if which == "two" else hash_one_pass)(np.arange(m), slots)
    last = np.flatnonzero(home >= slots - 8)[:count].tolist()
    zero = np.flatnonzero(home == 0)[:3].tolist()
    assert len(last) == count and len(zero) >= 1, (slots, which, len(last), len(zero))
    return last + zero


def _chain_cases():
    out = []
    for hb, L in enumerate(HASH_LIMIT):
        for form in ("general", "narrow"):
            if form == "narrow" and L > H2_MAXP:
                continue
            rows = []
            for r in chain_rows(slots_one_pass(hb), "one") + chain_rows(slots_two_pass(hb), "two"):
                if r not in rows:
                    rows.append(r)
            c = ordered_class(L)
            if c < 3:
                rows += [r for r in chain_rows(ORD_CLASSES[c][0], "one") if r not in rows]
            g = Build(M_CHAIN, 700 + hb)
            have = set(rows)
            rows += [r for r in g.rows(2 * L) if r not in have][:L - len(rows)]      # fill up to P = L, all rows distinct
            ids = g.a_split(rows, narrow_lens(L) if form == "narrow" else general_lens(L))
            g.b(ids)
            g.b(ids[::-1])                                                           # the chain rows last
            base = BIN_NARROW0 if form == "narrow" else BIN_HASH0
            out.append(g.case("chain-bin%d-%s" % (hb, form), "chains", {"P": [L, L], "cnt": [L, L], "bins": [base + hb] * 2,
                                                                         "classes": [c]}))
    return out


def _ordered_cases():
    out = []
    for m in (DENSE_MAX, M_HASH):
        tag = "m%d" % m
        # C(:,j) of SGO_CNTc | + 1 distinct rows
        g = Build(m, 800)
        cnts = []
        for _, maxcnt, _ in ORD_CLASSES:
            for cnt in (maxcnt, maxcnt + 1):
                ids = g.a_split(g.rows(cnt, start=3 * cnt), split(cnt, 129))
                g.b(ids + ids[:2] + ids[:1] + ids[:1])                               # (some rows two and four times)
                cnts.append(cnt)
        out.append(g.case("ordered-classes-" + tag, "ordered", {"cnt": cnts, "classes": [0, 1, 2, 3],
                                                                 "col_class": [0, 1, 1, 2, 2, 3]}))
        # columns of B of 1, 8, 9, 64, 65 entries over columns of A of 64, 65 and 129 entries, rows shared between them
        g = Build(m, 801)
        ac = [g.a(g.rows(ln, start=40 * i)) for i, ln in enumerate([64, 65, 129, 3, 1, 64, 65, 129, 2, 7])]
        blens = [1, 8, 9, 64, 65]
        for bl in blens:
            g.b([ac[(bl + 3 * t) % len(ac)] for t in range(bl)])                     # the same row through different entries of B
        out.append(g.case("ordered-lengths-" + tag, "ordered", {"blen": blens, "alen": [64, 65, 129, 3, 1, 64, 65, 129, 2, 7]}))
        # one column of A holding a row at positions (0, 1), (0, 63), (63, 64), three times in a batch, 64 times
        g = Build(m, 802)
        cols = []
        for pairs in ([(0, 1)], [(0, 63)], [(63, 64)], [(2, 9), (2, 40)]):
            r = g.rows(70, start=100 * len(cols))
            for a, b in pairs:
                r[b] = r[a]
            cols.append(g.a(r))
        cols.append(g.a([g.rows(1, start=999)[0]] * 64))
        other = g.a(g.rows(9, start=3))
        for c in cols:
            g.b([other, c, c, other])
        g.b(cols)
        out.append(g.case("ordered-equal-rows-" + tag, "ordered", {"alen": [70, 70, 70, 70, 64, 9]}))
        # DENSE_WAVES + 2 columns in the dense-map class
        g = Build(m, 803)
        ids = g.a_split(g.rows(SGO_MAX + 70, start=0), split(SGO_MAX + 70, 129))
        for j in range(DENSE_WAVES + 2):
            rot = j % len(ids)
            g.b(ids[rot:] + ids[:rot] + ids[j % 3:j % 3 + 2] + ids[j % 3:j % 3 + 1])
        out.append(g.case("ordered-dense-map-" + tag, "ordered", {"n": DENSE_WAVES + 2, "cnt": [SGO_MAX + 70] * (DENSE_WAVES + 2),
                                                                  "classes": [3]}))
    return out


def too_big_case():
    """one column with 2^32 products: A is m x 1 with 65 536 entries, B is 1 x 1 with 65 536 entries that all name column 0"""
    g = Build(M_CHAIN, 900)
    a = g.a(g.rows(M_CHAIN))
    g.b([a] * M_CHAIN)
    return g.case("too-big", "degenerate", {"P": [M_CHAIN * M_CHAIN]}, two_pass_too=False)


def degenerate_shapes():
    """(name, m, k, n, columns of A, columns of B): the empty shapes the Python layer admits"""
    return [("n0", 5, 3, 0, [[0], [1, 2], []], []),
            ("k0", 5, 0, 3, [], [[], [], []]),
            ("m0", 0, 3, 2, [[], [], []], [[0], [1, 2]]),
            ("nnzA0", 5, 3, 2, [[], [], []], [[0, 1], [2]]),
            ("nnzB0", 5, 3, 2, [[0], [1, 2], [4]], [[], []]),
            ("all0", 0, 0, 0, [], []),
            ("m0k0", 0, 0, 2, [], [[], []])]


@functools.lru_cache(maxsize=None)
def tables(cus):
    cases = (_bins_cases() + _narrow_cases() + _h1_cases() + _two_pass_cases() + _handover_cases(cus) + _global_reuse_cases() +
             _chain_cases() + _ordered_cases())
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)


def names():
    """the names of the cases (they do not depend on cus)"""
    return [c.name for c in tables(4)]


def by_name(cus, name):
    return next(c for c in tables(cus) if c.name == name)
