"""Inputs of tests/test_gpu_chol_edges.py: matrices constructed to sit on the constants that cut the general cs_chol numeric
(csparse.py_amd/csrc/csx_chol.hip, chol_analysis_run), and a model of its schedule written from its rules.

Every matrix is a weighted graph Laplacian plus a small diagonal: off-diagonals -(1 + 0.1 u), u uniform in [0, 1), the diagonal
the sum of the magnitudes of its row plus DELTA.  So it is symmetric positive definite and diagonally dominant whatever the
pattern, every entry of L off the diagonal is negative, every update l_ik l_jk has the same sign (nothing cancels but the
diagonal against its own sum) and none is negligible: tests/test_chol_cases_cpu.py holds every update of every case to at
least 100 x the bound the device is compared at, so an update lost or applied twice cannot pass.

The constants come from the library (`_csx.chol_limits()`, no device needed); NB and WB_PANEL_ROWS of csx_cholband.hip are not
among them and are written down here.

`schedule(parent, cp, ...)` restates what chol_analysis_schedule / chol_analysis_run decide from the elimination tree and the
column counts alone: the small trees, the level lists without the members of supernodes, the supernode groups by level and the
launch list of the level walk; `band_decision` restates chol_analysis_map's gates.  tests/test_chol_cases_cpu.py shows without
a device that every case sits on the edge it is named for; the GPU tests hold refactor_info() to the model."""
import functools

import numpy as np
import scipy.sparse as sp

import _csx
import c_oracle as CO
from chol_refactor_cases import Case

LIM = _csx.chol_limits()
CH_ACC, CH_NARROW, CH_SMALL_TREE, CD_MAX = LIM["CH_ACC"], LIM["CH_NARROW"], LIM["CH_SMALL_TREE"], LIM["CD_MAX"]
CC_ACC, CC_MAP, CC_RUN_MIN, CC_RUN_MAX, CC_WAVES = LIM["CC_ACC"], LIM["CC_MAP"], LIM["CC_RUN_MIN"], LIM["CC_RUN_MAX"], LIM["CC_WAVES"]
SN_MIN_WIDTH, WINDOWS, MAX_NEED = LIM["SN_MIN_WIDTH"], LIM["windows"], LIM["max_need"]
SN_NB = 16             # csx_cholband.hip chol_supernodes: columns per panel
WB_PANEL_ROWS = 256    # csx_cholband.hip: rows below the diagonal block per workgroup of role A
UQ = 8                 # csx_chol.hip chol_column / k_chol_coop (CC_Q): update descriptors fetched per round trip
WBAND_MIN_NEED = 80    # chol_analysis_map: under "chol.wband" = 1 the blocked dense band takes need > 80
DELTA = 0.05

COLUMN_KERNELS = (("chol.band", 0),)
NO_WBAND = (("chol.wband", 0),)


# ---- patterns: lists of off-diagonal ties (i, j), any orientation ----------------------------------------------------

def upper_laplacian(n, ties, seed, delta=DELTA):
    """(n, p, i, x) of the upper triangle, rows ascending, of the weighted Laplacian of `ties` plus delta I"""
    t = np.asarray(sorted(set((min(a, b), max(a, b)) for a, b in ties)), np.int64).reshape(-1, 2)
    assert len(t) == 0 or (t[:, 0] != t[:, 1]).all() and t.min() >= 0 and t.max() < n
    w = 1.0 + 0.1 * np.random.default_rng(seed).uniform(0.0, 1.0, len(t))
    diag = np.full(n, delta)
    np.add.at(diag, t[:, 0], w)
    np.add.at(diag, t[:, 1], w)
    U = sp.csc_matrix((np.concatenate([-w, diag]), (np.concatenate([t[:, 0], np.arange(n)]), np.concatenate([t[:, 1], np.arange(n)]))),
                      shape=(n, n))
    U.sort_indices()
    return n, U.indptr.astype(np.int32), U.indices.astype(np.int32), U.data.astype(np.float64)


def band_ties(gx, gy=12):
    """five-point grid, natural order (x fastest): a chain tree, the factor full inside half-width gx"""
    ties = []
    for j in range(gx * gy):
        if j % gx:
            ties.append((j - 1, j))
        if j >= gx:
            ties.append((j - gx, j))
    return gx * gy, ties


def dense_band_ties(hb, n=600):
    """every (i, j) with 0 < j - i <= hb: a chain tree and a full band in which nothing is fill"""
    return n, [(j - d, j) for j in range(n) for d in range(1, hb + 1) if j - d >= 0]


def band_holes_ties(n=600, reach=100, at=(150, 151, 260, 399, 599)):
    """a tridiagonal plus a handful of entries (i, i - reach): a chain tree, half-width `reach`, rows that are nearly empty"""
    return n, [(j - 1, j) for j in range(1, n)] + [(i - reach, i) for i in at]


def hub_ties(children, long_len, childless=1, scattered=100):
    """Columns: the leaves a (those of b_0 first; the very first is a_0), then the b's -- `childless` ones without a leaf, then
    b_0 .. b_{p-1} with children[t] leaves each --, then q_0 .. q_{K-1}, K = long_len - 1.  Ties a - its b, every b - q_0,
    b_0 - every q, a_0 - `scattered` of the q's.  Returns (n, ties, where): where = first column of the a's (0), of the childless
    b's, of b_0 and of q_0."""
    p, K = len(children), long_len - 1
    assert children[0] >= 1 and scattered > 64 and K >= scattered
    na = int(sum(children))
    bc, b0 = na, na + childless
    q0 = b0 + p
    ties, a = [], 0
    for t, c in enumerate(children):
        for _ in range(c):
            ties.append((a, b0 + t))
            a += 1
    for b in range(bc, q0):
        ties.append((b, q0))
    for s in range(K):
        ties.append((b0, q0 + s))
    for s in np.unique(np.linspace(0, K - 1, scattered).astype(np.int64)):
        ties.append((0, q0 + int(s)))
    return q0 + K, ties, {"a": 0, "childless": bc, "b": b0, "q": q0}


def comb_ties(c, leaves=520):
    """leaves under t_0; the chain t_0 .. t_{c-1}; before every t_i, i > 0, a leaf u_i tied to t_i and to every later t"""
    ties = [(k, leaves) for k in range(leaves)]
    t = [leaves] + [leaves + 2 * i for i in range(1, c)]
    for i in range(1, c):
        ties.append((t[i - 1], t[i]))
        for j in range(i, c):
            ties.append((t[i] - 1, t[j]))
    return leaves + 2 * c - 1, ties, t


def arrow_ties(n):
    return n, [(j - 1, j) for j in range(1, n)] + [(j, n - 1) for j in range(n - 2)]


def bintree_ties(n, depth=9):
    """a complete binary tree of 2^depth - 1 columns in postorder, every column tied to its parent and its grandparent, and a
    chain on top of the root up to n columns: level widths 256, 128, 64, 32, ... 1, 1, ..."""
    ties, counter = [], [0]

    def walk(d):
        """numbers the subtree, returns (root, its children)"""
        kids = [walk(d - 1) for _ in range(2)] if d > 1 else []
        me = counter[0]
        counter[0] += 1
        for k, grand in kids:
            ties.append((k, me))
            for g in grand:
                ties.append((g, me))
        return me, [k for k, _ in kids]

    root, kids = walk(depth)
    assert counter[0] == 2 ** depth - 1 <= n
    prev, prev2 = root, kids
    for j in range(counter[0], n):
        ties.append((prev, j))
        for g in prev2:
            ties.append((g, j))
        prev, prev2 = j, [prev]
    return n, ties


def cliques_ties(sizes):
    ties, c0 = [], 0
    for m in sizes:
        ties += [(c0 + a, c0 + b) for a in range(m) for b in range(a + 1, m)]
        c0 += m
    return c0, ties


def sn_ties(specs, leaves=520):
    """one tree per (w, r) of specs, one after the other: `leaves` leaves under s_0, a clique s_0 .. s_{w-1} every column of
    which is tied to the r columns that follow, those r a clique of their own; a leaf under the first of the r keeps the two
    cliques from joining into one supernode.  Returns (n, ties, [(first column of s, first column of the r rows)])."""
    ties, c0, where = [], 0, []
    for w, r in specs:
        nl = leaves + (1 if r else 0)
        s0 = c0 + nl
        r0 = s0 + w
        ties += [(c0 + k, s0) for k in range(leaves)]
        if r:
            ties.append((c0 + leaves, r0))
        ties += [(s0 + a, s0 + b) for a in range(w) for b in range(a + 1, w)]
        ties += [(s0 + a, r0 + b) for a in range(w) for b in range(r)]
        ties += [(r0 + a, r0 + b) for a in range(r) for b in range(a + 1, r)]
        where.append((s0, r0))
        c0 = r0 + r
    return c0, ties, where


# ---- the model ----------------------------------------------------------------------------------------------------------

def schedule(parent, cp, supernodes=True, dense_trees=True):
    """chol_analysis_schedule and the level walk of chol_analysis_run, from the elimination tree and the column counts.
    Returns a dict: trees / dense (small trees by kernel), big_cols, nlev (levels of the big trees, supernode members counted),
    widths (columns per level without the members), sns ([(level, a, w, r)] in the library's order: by level, then by column),
    launches (the walk: ("level", l, grid), ("coop", mode, l0, l1, grid) and -- not counted by refactor_info()["levels"] --
    ("sn", l, [(a, w, r), ...])) and levels (the count refactor_info() reports)."""
    parent = np.asarray(parent, np.int64)
    cp = np.asarray(cp, np.int64)
    n = len(parent)
    root = np.arange(n)
    for j in range(n - 1, -1, -1):
        if parent[j] >= 0:
            root[j] = root[parent[j]]
    size = np.bincount(root, minlength=n)
    big = size[root] > CH_SMALL_TREE
    trees = dense = 0
    for r in np.flatnonzero(parent < 0):
        if size[r] > CH_SMALL_TREE:
            continue
        cols = np.flatnonzero(root == r)
        m = len(cols)
        is_dense = (m <= CD_MAX and np.array_equal(cols, cols[0] + np.arange(m))
                    and np.array_equal(np.diff(cp)[cols], m - np.arange(m)))
        if is_dense and dense_trees:
            dense += 1
        else:
            trees += 1
    level = np.zeros(n, np.int64)
    nlev = 0
    for j in range(n):
        if big[j]:
            nlev = max(nlev, level[j] + 1)
            if parent[j] >= 0:
                level[parent[j]] = max(level[parent[j]], level[j] + 1)
    member = np.zeros(n, bool)
    sns = []
    if supernodes and nlev:
        nchild = np.bincount(parent[parent >= 0], minlength=n)
        cnt = np.diff(cp)
        j = 0
        while j < n:
            if not big[j]:
                j += 1
                continue
            a = j
            while j + 1 < n and parent[j] == j + 1 and nchild[j + 1] == 1 and cnt[j + 1] == cnt[j] - 1:
                j += 1
            w = j - a + 1
            if w >= SN_MIN_WIDTH:
                sns.append((int(level[a]), a, w, int(cnt[a] - w)))
                member[a:j + 1] = True
            j += 1
        sns.sort(key=lambda s: s[0])          # (stable: by column inside a level)
    widths = np.bincount(level[big & ~member], minlength=nlev)[:nlev] if nlev else np.zeros(0, np.int64)
    group_at = {}
    for s in sns:
        group_at.setdefault(s[0], []).append(s[1:])
    launches, l = [], 0
    while l < nlev:
        if l in group_at:
            launches.append(("coop", 1, l, l + 1, sum(w for _, w, _ in group_at[l])))
            launches.append(("sn", l, group_at[l]))
        if widths[l] == 0:
            l += 1
            continue
        if widths[l] > CH_NARROW:
            launches.append(("level", l, int(widths[l])))
            l += 1
            continue
        e = l + 1
        while e < nlev and e - l < CC_RUN_MAX and widths[e] <= CH_NARROW and e not in group_at:
            e += 1
        two_phase = e - l >= CC_RUN_MIN
        if two_phase:
            launches.append(("coop", 1, l, e, int(widths[l:e].sum())))
        a = l
        while a < e:
            if widths[a] == 0:
                a += 1
                continue
            b = a + 1
            if widths[a] == 1:
                while b < e and widths[b] == 1:
                    b += 1
            launches.append(("coop", 2 if two_phase else 0, a, b, int(widths[a])))
            a = b
        l = e
    return {"trees": trees, "dense": dense, "big_cols": int(big.sum()), "nlev": int(nlev), "widths": widths, "sns": sns,
            "level": np.where(big, level, -1), "launches": launches, "levels": sum(1 for k in launches if k[0] != "sn")}


def band_decision(n, Lp, Li, sched, band=1, wband=1):
    """chol_analysis_map's gates -> (band kind: 0 none, 1 register window, 2 blocked dense band; window; half-bandwidth or
    None where the gates never look).  The free-memory test of the blocked band is taken to pass."""
    if not band or not (sched["big_cols"] * 2 > n and sched["nlev"] * 4 > sched["big_cols"]):
        return 0, 0, None
    hb = int(np.max(Li[np.asarray(Lp[1:]) - 1] - np.arange(n)))
    need = hb + 1
    full = float(Lp[n]) >= 0.5 * n * (hb + 1.0)
    if (wband == 2 or (wband == 1 and need > WBAND_MIN_NEED)) and full:
        return 2, 0, hb
    if need <= MAX_NEED:
        return 1, min(w for w in WINDOWS if need <= w), hb
    return 0, 0, hb


# ---- the cases ----------------------------------------------------------------------------------------------------------

class EdgeCase(Case):
    """Case plus: bytes_upto (the leading columns whose L.x must equal the oracle's byte for byte: n on the exact routes, 0 on
    the rounding routes), bad_at (columns whose negated diagonal makes further value sets that are not positive definite),
    marks (what the CPU test checks the geometry against) and twin (the case it must agree with across routes)."""

    def __init__(self, name, n, p, i, x, options=(), expect=None, seed=1, exact_route=False, bytes_upto=None, bad_at=(), marks=None,
                 twin=None):
        Case.__init__(self, name, n, p, i, x, order=0, options=options, expect=expect, seed=seed)
        self.bytes_upto = (self.n if exact_route else 0) if bytes_upto is None else bytes_upto
        self.bad_at = tuple(bad_at) or (self.n // 2,)
        self.marks = dict(marks or {})
        self.twin = twin

    def bad_values(self, j):
        bad = self.x.copy()
        on_diag = (self.cols == j) & (self.i == j)
        assert on_diag.sum() == 1
        bad[on_diag] = -bad[on_diag]
        return bad

    def option(self, name, default=1):
        return dict(self.options).get(name, default)


def _build():
    cases = []
    seed = [100]

    def add(name, n, ties, delta=DELTA, **kw):
        seed[0] += 1
        cases.append(EdgeCase(name, *upper_laplacian(n, ties, seed[0], delta), seed=seed[0], **kw))

    general = {"route": "general", "trees": 0, "dense_trees": 0}
    # -- the register window: both sides of every class, under "chol.wband" = 0
    for gx in (47, 48, 79, 80, 111, 112, 143, 144, 175):
        need = gx + 1
        bw = min(w for w in WINDOWS if need <= w)
        n, ties = band_ties(gx)
        add("band%d" % gx, n, ties, options=NO_WBAND, exact_route=True, bad_at=(0, n - 1, n // 2),
            expect=dict(general, band=1, window=bw, supernodes=0, levels=0), marks={"need": need, "window": bw})
    # ... and the same windows on full bands without fill, where no update is small (the fill of a grid decays geometrically
    # across its band: see test_chol_cases_cpu.py)
    for hb in (47, 48, 79, 80, 111, 112, 143, 144, 175):
        bw = min(w for w in WINDOWS if hb + 1 <= w)
        n, ties = dense_band_ties(hb)
        add("dband%d" % hb, n, ties, options=NO_WBAND, exact_route=True, bad_at=(0, n - 1, n // 2),
            expect=dict(general, band=1, window=bw, supernodes=0, levels=0), marks={"need": hb + 1, "window": bw})
    n, ties = dense_band_ties(176)
    add("dband176-no-window", n, ties, options=NO_WBAND, expect=dict(general, band=0, window=0, supernodes=1), marks={"need": MAX_NEED + 1, "window": 0})
    n, ties = band_ties(176)
    add("band176-no-window", n, ties, options=NO_WBAND, expect=dict(general, band=0, window=0, supernodes=1),
        marks={"need": MAX_NEED + 1, "window": 0})
    n, ties = band_ties(79)
    add("band79-default", n, ties, exact_route=True, expect=dict(general, band=1, window=80, levels=0), marks={"need": 80, "window": 80})
    n, ties = band_ties(80)
    add("band80-default", n, ties, exact_route=True, expect=dict(general, band=2, window=0, levels=0), marks={"need": 81, "window": 0})
    n, ties = band_holes_ties()
    add("band-holes", n, ties, delta=1e-4, options=NO_WBAND, exact_route=True, bad_at=(0, n - 1, n // 2),
        expect=dict(general, band=1, window=112, levels=0), marks={"need": 101, "window": 112, "holes": True})
    # -- hubs: a long column one level above the leaves, then a clique
    batch = [9, 1, 7, 8, 9, 16, 17]                      # leaf children of b_0 .. b_6: the UQ / CC_Q batch edges (0: the childless b)
    for pairs, long_len, kind in ((CH_NARROW + 1, CH_ACC + 1, "level"), (CH_NARROW + 1, CH_ACC, "level"),
                                  (CH_NARROW, CC_ACC // CC_WAVES + 1, "coop"), (CH_NARROW, CC_ACC // CC_WAVES, "coop"),
                                  (4, CC_ACC // 8 + 1, "coop"), (4, CC_ACC // 8, "coop")):
        children = (batch + [1] * pairs)[:pairs] if pairs > 4 else [9, 1, 7, 8]
        n, ties, where = hub_ties(children, long_len)
        marks = {"hub": where, "children": children, "long_len": long_len, "kind": kind, "level1": pairs}
        nm = "hub%d-%d" % (pairs, long_len)
        add(nm, n, ties, options=COLUMN_KERNELS, expect=dict(general, band=0, window=0, supernodes=1), marks=marks)
        seed[0] -= 1                                      # the same values: the two routes are compared with each other
        add(nm + "-no-supernodes", n, ties, options=COLUMN_KERNELS + (("chol.supernodes", 0),),
            expect=dict(general, band=0, window=0, supernodes=0), marks=marks, twin=nm)
    # -- combs: the two-phase run rule
    for c in (CC_RUN_MIN - 1, CC_RUN_MIN, CC_RUN_MAX, CC_RUN_MAX + 1, CC_RUN_MAX + CC_RUN_MIN):
        n, ties, t = comb_ties(c)
        add("comb%d" % c, n, ties, options=COLUMN_KERNELS, expect=dict(general, band=0, window=0, supernodes=0), marks={"comb": c, "t": t})
    # -- arrows: either side of the LDS row map
    for n in (CC_MAP, CC_MAP + 1):
        add("arrow%d" % n, *arrow_ties(n), expect=dict(general, band=0, window=0, supernodes=0), marks={"arrow": n})
    # -- small trees
    for n in (CH_SMALL_TREE, CH_SMALL_TREE + 1):
        small = n <= CH_SMALL_TREE
        add("bintree%d" % n, *bintree_ties(n), options=COLUMN_KERNELS,
            expect={"route": "general", "trees": 1 if small else 0, "dense_trees": 0, "band": 0, "window": 0, "supernodes": 0},
            marks={"bintree": n})
    sizes = (1, 2, CD_MAX - 1, CD_MAX, CD_MAX + 1)
    add("cliques", *cliques_ties(sizes), options=(("chol.clique", 0), ("chol.forest", 0)), bytes_upto=sum(sizes[:-1]),
        expect={"route": "general", "trees": 1, "dense_trees": 4, "band": 0, "window": 0, "supernodes": 0, "levels": 0},
        marks={"cliques": sizes})
    # -- supernodes
    m = SN_MIN_WIDTH
    for w, r in ((m - 1, 0), (m, 0), (SN_NB - 1, 0), (SN_NB, 0), (SN_NB + 1, 0), (2 * SN_NB + 1, 0), (SN_NB, WB_PANEL_ROWS),
                 (SN_NB, WB_PANEL_ROWS + 1)):
        n, ties, where = sn_ties([(w, r)])
        want = [(where[0][0], w, r)] if w >= m else []
        if r >= m:
            want.append((where[0][1], r, 0))
        add("sn%d-%d" % (w, r), n, ties, options=COLUMN_KERNELS, expect=dict(general, band=0, window=0, supernodes=len(want)),
            marks={"sns": want})
    n, ties, where = sn_ties([(8, 300), (40, 0)])
    add("sn-pair", n, ties, options=COLUMN_KERNELS, expect=dict(general, band=0, window=0, supernodes=3),
        marks={"sns": [(where[0][0], 8, 300), (where[1][0], 40, 0), (where[0][1], 300, 0)], "group": 2, "forest": 2})
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
ROUNDING = [c.name for c in CASES if c.bytes_upto < c.n]


# ---- the oracle, once per (case, value set) -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def symbolic(name):
    c = BY_NAME[name]
    return CO.schol(c.n, c.p, c.i)


def values(case, which):
    """which: "A", 0 / 1 (the congruent sets), ("bad", column)"""
    if which == "A":
        return case.x
    if isinstance(which, tuple):
        return case.bad_values(which[1])
    return case.A2[which]


@functools.lru_cache(maxsize=None)
def oracle(name, which="A"):
    """the plain-C oracle's (Lp, Li, Lx) of the case's value set, or None where it is not positive definite; read-only arrays"""
    c = BY_NAME[name]
    parent, cp = symbolic(name)
    out = CO.chol(c.n, c.p, c.i, values(c, which), parent, cp)
    if out is not None:
        for a in out:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    c = BY_NAME[name]
    parent, cp = symbolic(name)
    return schedule(parent, cp, supernodes=bool(c.option("chol.supernodes")), dense_trees=bool(c.option("chol.dense_trees")))


@functools.lru_cache(maxsize=None)
def decision(name):
    c = BY_NAME[name]
    Lp, Li, _ = oracle(name)
    return band_decision(c.n, Lp, Li, model(name), band=c.option("chol.band"), wband=c.option("chol.wband"))


def expected_levels(name):
    """what refactor_info()["levels"] must say: the model's launch count, 0 under a band kernel or without level lists"""
    return 0 if decision(name)[0] else model(name)["levels"]


# ---- the measure ----------------------------------------------------------------------------------------------------------

def lower_of(case, x, Lp, Li):
    """|a_ij| on the slots of L (0 for fill)"""
    n = case.n
    up = case.i <= case.cols
    A = sp.csc_matrix((np.abs(x[up]), (case.cols[up], case.i[up])), shape=(n, n))      # the transpose of the upper triangle
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(Lp)) * n + Li
    A = A.tocoo()
    out = np.zeros(len(Li))
    out[np.searchsorted(keys, A.col.astype(np.int64) * n + A.row)] = A.data
    return out


@functools.lru_cache(maxsize=None)
def terms(name, which="A"):
    """tol.chol_terms of the oracle's factor of the case's value set"""
    import tol as TOL
    c = BY_NAME[name]
    Lp, Li, Lx = oracle(name, which)
    t = TOL.chol_terms(c.n, Lp, Li, Lx, lower_of(c, values(c, which), Lp, Li))
    t.setflags(write=False)
    return t


def rounding_units(name, which, got):
    """max |got - L_oracle| / (EPS * terms) over the entries of L (got: float64 or longdouble)"""
    import tol as TOL
    return float(np.max(np.abs(np.asarray(got, np.longdouble) - oracle(name, which)[2]) / (TOL.EPS * terms(name, which))))


def longdouble_factor(case, x, Lp, Li):
    """L.x of the value set x on the pattern (Lp, Li), left-looking in numpy.longdouble"""
    n = case.n
    up = case.i <= case.cols
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(Lp)) * n + Li
    Lx = np.zeros(len(Li), np.longdouble)
    Lx[np.searchsorted(keys, case.i[up].astype(np.int64) * n + case.cols[up])] = x[up]    # (i, j) upper -> slot (j, i)
    cols = np.repeat(np.arange(n), np.diff(Lp))
    R = sp.csr_matrix((np.arange(1, len(Li) + 1), (Li, cols)), shape=(n, n))            # row view: slot + 1
    R.sort_indices()
    where = np.zeros(n, np.int64)
    Li = np.asarray(Li)
    for j in range(n):
        b, e = int(Lp[j]), int(Lp[j + 1])
        where[Li[b:e]] = np.arange(b, e)
        for q in range(R.indptr[j], R.indptr[j + 1] - 1):          # the row ends with the diagonal
            pos, kend = int(R.data[q]) - 1, int(Lp[R.indices[q] + 1])
            Lx[where[Li[pos:kend]]] -= Lx[pos] * Lx[pos:kend]
        assert Lx[b] > 0
        Lx[b] = np.sqrt(Lx[b])
        Lx[b + 1:e] /= Lx[b]
    return Lx


def smallest_update(name, which="A", sample=1000000, seed=7):
    """(min over updates (i, j, k) of |l_ik l_jk| / (EPS (|a_ij| + sum_k |l_ik l_jk|)), updates looked at, updates in all).
    Every update where there are at most `sample`; a seeded sample of that many otherwise (dealt to the columns by their
    share of the updates)."""
    import tol as TOL
    case = BY_NAME[name]
    n = case.n
    Lp, Li, Lx = oracle(name, which)
    den = terms(name, which) * np.repeat(Lx[Lp[:-1]], np.diff(Lp))      # |a_ij| + sum_k |l_ik l_jk|
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(Lp)) * n + Li
    m = np.diff(Lp).astype(np.int64) - 1                              # entries below the diagonal of every column
    per = m * (m + 1) // 2
    total = int(per.sum())
    rng = np.random.default_rng(seed)
    best, seen = np.inf, 0
    absx = np.abs(Lx)
    for k in np.flatnonzero(m > 0):
        b = int(Lp[k]) + 1
        rows, v = Li[b:b + m[k]].astype(np.int64), absx[b:b + m[k]]
        if total <= sample:
            a, c = np.tril_indices(int(m[k]))
        else:
            take = max(1, int(round(sample * per[k] / total)))
            if take >= per[k]:
                a, c = np.tril_indices(int(m[k]))
            else:
                a = rng.integers(0, m[k], take)
                c = rng.integers(0, m[k], take)
                a, c = np.maximum(a, c), np.minimum(a, c)
        slot = np.searchsorted(keys, rows[c] * n + rows[a])           # (i, j) = (rows[a], rows[c]), i >= j
        best = min(best, float(np.min(v[a] * v[c] / (TOL.EPS * den[slot]))))
        seen += len(a)
    return best, seen, total
