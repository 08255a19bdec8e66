"""Constructed triangular systems for the generic triangular solve (csx_trisolve.hip), one per side of every cut of tri_route,
make_segments, walk_levels and analyse, and a Python model of those three functions.  TEST INFRASTRUCTURE, NOT PRODUCT.

A case is built as an ABSTRACT system first: unknowns 0 .. n-1 in solve order, each with the list of the earlier unknowns it
takes a term from.  `to_matrix` turns it into the matrix of a kind: L for cs_lsolve (unknown a is row a; the terms of a row come
out in ascending column order whatever the storage order, so the rows of a column are stored shuffled), L for cs_ltsolve
(unknown a is column n-1-a, its sources stored in the list's order behind the diagonal), U for cs_usolve and cs_utsolve (the
mirror images, diagonal last).  Values: |diagonal| in [1, 2] with a random sign, an off-diagonal entry at most 0.5 over the
larger of its row's and its column's entry count, so that every row and every column is diagonally dominant by a factor 2.

The model (`model`) is written from the rules in the source and reads every constant from the library (`_csx.tri_limits()`, no
device needed).  For a matrix, a kind, a number of right-hand sides and the options in force it predicts what a FRESH plan's
first solve does: every field of csx_tri_route_info and every counter of csx_tri_launches.  tests/test_tri_cases_cpu.py shows
without a device that each case sits on the edge it is named for, by the model; tests/test_gpu_tri_edges.py holds the library's
read-backs to the model field for field and the results to the plain-C oracle byte for byte.

What the issue of this table names and no case reaches is listed with the reason in NOT_REACHED at the end."""
import functools
import zlib

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import _csx

LIM = _csx.tri_limits()
KINDS = ("lsolve", "ltsolve", "usolve", "utsolve")
KIND_ID = {"lsolve": _csx.TRI_L, "ltsolve": _csx.TRI_LT, "usolve": _csx.TRI_U, "utsolve": _csx.TRI_UT}
PUSH = ("lsolve", "usolve")
NOT_A_TRIANGLE = 0x7fffffff
DEFAULT_OPTIONS = {"tri.components": 1, "tri.columns": 1, "tri.push": 1, "tri.chain_walker": 1, "tri.row_waves": 1,
                   "tri.levels_where": 0}


# ---- abstract systems ---------------------------------------------------------------------------------------------------------
class System:
    """unknowns in solve order; src[a]: the earlier unknowns a takes a term from, in the order a gather kind subtracts them"""

    def __init__(self, src):
        self.n = len(src)
        self.src = [np.asarray(s, np.int64) for s in src]


def banded(n, band, avg=0, terms=None, long_lists=(), fans=()):
    """a chain of half-width `band`: every unknown takes its predecessor and the unknown `band` back; avg: also the `avg` nearest
    ones (a full band of that width); long_lists: (a, count) -- unknown a takes its `count` nearest (a long column of L', U');
    fans: (s, count) -- unknown s is taken by the `count` next ones (a long column of L, U); terms: the total, met exactly by
    giving up or adding near terms at the far end"""
    src = [set() for _ in range(n)]
    for a in range(n):
        near = range(max(0, a - avg), a) if avg else ()
        src[a].update(near)
        if a >= 1:
            src[a].add(a - 1)
        if a >= band:
            src[a].add(a - band)
    for a, count in long_lists:
        assert count <= band and a >= count
        src[a] = set(range(a - count, a))              # exactly `count`: not the one `band` back
    for s, count in fans:
        assert count <= band and s + count < n
        for a in range(s + 1, s + count + 1):
            src[a].add(s)
        if count < band and s + band < n:              # exactly `count`
            src[s + band].discard(s)
    if terms is not None:
        have = sum(len(s) for s in src)
        a = n - 1
        while have != terms:                      # near the end, away from the long lists and fans
            a -= 1
            assert a > max([band] + [x for x, _ in long_lists] + [s + c for s, c in fans])
            if have > terms:
                extra = sorted(src[a] - {a - 1, a - band})
                drop = extra[:min(len(extra), have - terms)]
                src[a].difference_update(drop)
                have -= len(drop)
            else:
                add = [s for s in range(a - band + 1, a - 1) if s not in src[a]][:terms - have]
                src[a].update(add)
                have += len(add)
    return System([sorted(s) for s in src])


def layered(widths, count, specials=None, terms=None):
    """level sets of the given widths, the unknowns numbered level by level; an unknown of level l > 0 takes the unknown of level
    l - 1 at its own offset (cyclically: that fixes its level) and count(l, i) - 1 more from all earlier levels, dealt round robin
    so that together they cover them; specials: {(l, i): explicit list} (indices as (level, offset) pairs or plain unknowns);
    terms: the total, met exactly by the last level giving up or adding terms"""
    first = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    src, deal = [], 0
    specials = specials or {}
    for l, w in enumerate(widths):
        for i in range(w):
            if (l, i) in specials:
                src.append([first[s[0]] + s[1] if isinstance(s, tuple) else s for s in specials[(l, i)]])
                continue
            if l == 0:
                src.append([])
                continue
            forced = int(first[l - 1] + i % widths[l - 1])
            got, want, pool = [], min(count(l, i), int(first[l])) - 1, int(first[l])
            while len(got) < want:
                s = deal % pool
                deal += 1
                if s != forced and s not in got:
                    got.append(s)
            src.append(sorted(got + [forced]))
    if terms is not None:
        have, a = sum(len(s) for s in src), len(src)
        lo = int(first[-2])
        while have != terms:
            a -= 1
            assert a >= lo and (len(widths) - 1, a - lo) not in specials
            forced = int(first[-2] + (a - lo) % widths[-2])
            if have > terms:
                keep = max(1, len(src[a]) - (have - terms))
                rest = [s for s in src[a] if s != forced][:keep - 1]
                have -= len(src[a]) - (len(rest) + 1)
                src[a] = sorted(rest + [forced])
            else:
                had = set(src[a])
                add = [s for s in range(lo) if s not in had][:terms - have]
                have += len(add)
                src[a] = sorted(src[a] + add)
    return System(src)


def forest(sizes, dense=(), density=0.3, seed=0, twice=None):
    """independent components of the given sizes on consecutive unknowns: inside one a path (so that it is one component) and
    each earlier unknown of the component with probability `density`; dense: the indices of components that are full triangles;
    twice: (component, unknown inside, source inside) -- that term is there twice (a row twice in a column of L)"""
    rng = np.random.default_rng(seed)
    src, base = [], 0
    for c, m in enumerate(sizes):
        for a in range(m):
            if c in dense:
                pick = np.arange(a)
            else:
                pick = np.flatnonzero(rng.random(a) < density)
                if a:
                    pick = np.union1d(pick, [a - 1])
            lst = (pick + base).tolist()
            if twice and twice[0] == c and twice[1] == a:
                lst = sorted([s for s in lst if s != base + twice[2]] + [base + twice[2]] * 2)
            src.append(lst)
        base += m
    return System(src)


def to_matrix(S, kind, seed):
    """(n, Tp, Ti, Tx) of the kind's matrix for the system S (see the module text)"""
    rng = np.random.default_rng(seed)
    n = S.n
    cnt = np.array([len(s) for s in S.src], np.int64)
    unk = np.repeat(np.arange(n, dtype=np.int64), cnt)
    s = np.concatenate(S.src) if cnt.sum() else np.zeros(0, np.int64)
    pos = np.arange(len(s)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    if kind in ("ltsolve", "utsolve"):                 # a column per unknown, the list's order
        col, row, key = unk, s, pos.astype(np.float64)
    else:                                              # a column per source, its rows shuffled
        col, row, key = s, unk, rng.random(len(s))
    if kind in ("ltsolve", "usolve"):                  # the backward kinds: mirrored
        col, row = n - 1 - col, n - 1 - row
    lower = kind in ("lsolve", "ltsolve")
    order = np.lexsort((key, col))
    col, row = col[order], row[order]
    per_col = np.bincount(col, minlength=n)
    per_row = np.bincount(row, minlength=n)
    scale = 0.5 / np.maximum(per_row[row], per_col[col])
    off = rng.uniform(-1.0, 1.0, len(row)) * scale
    diag = rng.uniform(1.0, 2.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    Tp = np.concatenate([[0], np.cumsum(per_col + 1)]).astype(np.int64)
    Ti, Tx = np.empty(Tp[-1], np.int64), np.empty(Tp[-1], np.float64)
    dpos = Tp[:-1] if lower else Tp[1:] - 1
    mask = np.ones(Tp[-1], bool)
    mask[dpos] = False
    Ti[dpos], Tx[dpos] = np.arange(n), diag
    Ti[mask], Tx[mask] = row, off
    return n, Tp.astype(np.int32), Ti.astype(np.int32), Tx


def misplace(T, lower, column, to_row):
    """T with the row of one off-diagonal entry of `column` replaced by `to_row` on the wrong side of the diagonal, in a slot that
    is not the diagonal's: what the reference's loop runs through without noticing"""
    n, Tp, Ti, Tx = T
    b, e = int(Tp[column]), int(Tp[column + 1])
    assert e - b >= 3 and (to_row < column if lower else to_row > column)
    Ti = Ti.copy()
    Ti[b + 1 if lower else b] = to_row
    return n, Tp, Ti, Tx


# ---- the model ----------------------------------------------------------------------------------------------------------------
def few_lds_bytes(rows, terms, G):
    return (terms if terms > 0 else 1) * 16 + rows * (16 + 8 * G) + 64


def tile_waves_per_workgroup(per_wave, maxw):
    cu, best, best_total = 160 * 1024 - 1024, 1, 0
    for w in range(1, maxw + 1):
        if per_wave * w > cu:
            break
        total = (cu // (per_wave * w)) * w
        if total > best_total:
            best_total, best = total, w
    return best


class PlanModel:
    """the host state of a fresh TriPlan and the lazy analyses tri_route runs on it"""

    def __init__(self, n, Tp, Ti, kind):
        self.n, self.kind = n, kind
        self.Tp, self.Ti = np.asarray(Tp, np.int64), np.asarray(Ti, np.int64)
        self.push = kind in PUSH
        self.forward = kind in ("lsolve", "utsolve")
        self.lower = kind in ("lsolve", "ltsolve")
        nnz = int(self.Tp[n])
        self.gnnz = nnz - n if self.push else nnz
        self.band, self.links, self.col_state = -1, 0, 0
        self.scheduled, self.nlevels, self.sequential, self.chain_ok, self.schedule = False, 0, False, False, 0
        self.comp_tried, self.comp_ok, self.ncomp, self.comp_max = False, False, 0, 0
        self.comps_found = self.comp_rows_found = 0
        self.push_terms = self.few_cpw = self.few_rows = self.few_terms = 0
        self.level_of_made = False
        self._gather()

    def _gather(self):
        n, Tp, Ti = self.n, self.Tp, self.Ti
        col = np.repeat(np.arange(n, dtype=np.int64), np.diff(Tp))
        keep = np.ones(len(Ti), bool)
        keep[Tp[:-1] if self.lower else Tp[1:] - 1] = False
        row, col = Ti[keep], col[keep]
        self.diag_at = Tp[:-1] if self.lower else Tp[1:] - 1
        at = np.flatnonzero(keep)             # where in T each term's value is
        if not self.push:                     # the column itself
            self.ptr = Tp - np.arange(n + 1)
            self.idx, self.val_at = row, at
            return
        seq = np.arange(len(row))
        if self.kind == "usolve":             # columns taken in reverse, storage order inside one
            seq = np.lexsort((seq, -col))
        order = seq[np.argsort(row[seq], kind="stable")]
        self.idx, self.val_at = col[order], at[order]
        self.ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)

    def malformed(self):
        unk = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.ptr))
        return bool(np.any(self.idx >= unk if self.forward else self.idx <= unk))

    def ensure_col_state(self):
        if self.col_state:
            return
        dup = False
        if self.push:
            unk = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.ptr))
            same = (self.idx[1:] == self.idx[:-1]) & (unk[1:] == unk[:-1])
            dup = bool(np.any(same))
        self.col_state = 2 if dup else 1

    def analyse_components(self):
        if self.comp_tried:
            return
        self.comp_tried = True
        n = self.n
        if n < LIM["COMP_MIN_COUNT"] or self.malformed():
            return
        unk = np.repeat(np.arange(n, dtype=np.int64), np.diff(self.ptr))
        G = sp.coo_matrix((np.ones(len(unk)), (unk, self.idx)), shape=(n, n)).tocsr()
        ncomp, lab = connected_components(G, directed=False)
        _, firsts = np.unique(lab, return_index=True)          # components in the order of their smallest unknown
        rank = np.empty(ncomp, np.int64)
        rank[lab[np.sort(firsts)]] = np.arange(ncomp)
        lab = rank[lab]
        sizes = np.bincount(lab, minlength=ncomp)
        self.comps_found, self.comp_rows_found = int(ncomp), int(sizes.max())
        if ncomp < LIM["COMP_MIN_COUNT"] or sizes.max() > LIM["COMP_MAX_ROWS"]:
            return
        self.ncomp, self.comp_max = int(ncomp), int(sizes.max())
        row_terms = np.diff(self.ptr)
        if self.push:
            self.ensure_col_state()
            if self.col_state == 1:
                col_terms = np.diff(self.Tp) - 1
                self.push_terms = max(1, int(np.bincount(lab, weights=col_terms, minlength=ncomp).max()))
        cpw = LIM["FEW_CPW"]
        group = np.arange(ncomp) // cpw
        rows = int(np.bincount(group, weights=sizes).max())
        terms = int(np.bincount(group, weights=np.bincount(lab, weights=row_terms, minlength=ncomp)).max())
        if few_lds_bytes(rows, terms, 64 // cpw) <= LIM["COMP_LDS_MAX"]:
            self.few_cpw, self.few_rows, self.few_terms = cpw, rows, terms
        self.comp_ok = True

    def measure_band(self):
        if self.band >= 0:
            return
        col = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.Tp))
        d = self.Ti - col
        is_diag = np.zeros(len(d), bool)
        is_diag[self.Tp[:-1] if self.lower else self.Tp[1:] - 1] = True
        bad = np.any(np.where(is_diag, d != 0, d <= 0 if self.lower else d >= 0))
        self.band = NOT_A_TRIANGLE if bad else int(np.abs(d).max())
        self.links = int(len(np.unique(col[np.abs(d) == 1])))
        if not bad and self.push:
            self.ensure_col_state()

    def levels(self):
        """level of every unknown, or None for a malformed triangle (compute_levels)"""
        n, ptr, idx = self.n, self.ptr, self.idx
        level = np.zeros(n, np.int64)
        for r in (range(n) if self.forward else range(n - 1, -1, -1)):
            s = idx[ptr[r]:ptr[r + 1]]
            if len(s):
                if (s.max() >= r) if self.forward else (s.min() <= r):
                    return None
                level[r] = level[s].max() + 1
        return level

    def ensure_schedule(self, where):
        if self.scheduled or self.n == 0:
            return
        self.scheduled = True
        level = self.levels()
        deep = level is not None and int(level.max()) + 1 > LIM["LV_MAX_ROUNDS"]
        on_device = where == 2 or (where == 0 and self.gnnz >= LIM["LV_DEVICE_MIN_TERMS"])
        self.schedule = 3 if not on_device else 4 if deep else 2
        if level is None:
            self.sequential, self.nlevels = True, self.n
            return
        self.level = level
        self.nlevels = int(level.max()) + 1
        self.order = np.argsort(level, kind="stable")
        self.level_ptr = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=self.nlevels))]).astype(np.int64)
        # the chain walker's tables: per position the leading terms from before the row's block of CHB positions
        pos_of = np.empty(self.n, np.int64)
        pos_of[self.order] = np.arange(self.n)
        unk = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.ptr))
        inside = pos_of[self.idx] >= (pos_of[unk] & ~(LIM["CHB"] - 1))
        self.inside = inside
        self.npre = np.zeros(self.n, np.int64)
        for r in np.unique(unk[inside]):
            self.npre[r] = int(np.argmax(inside[self.ptr[r]:self.ptr[r + 1]]))
        none = np.ones(self.n, bool)
        none[unk[inside]] = False
        self.npre[none] = np.diff(self.ptr)[none]
        all_terms = int(len(self.idx))
        suffix = all_terms - int(self.npre.sum())
        self.chain_ok = all_terms > 0 and suffix * 4 <= all_terms

    def segments(self, nrhs):
        """make_segments: (first level, end level, one workgroup)"""
        w = np.diff(self.level_ptr) * nrhs
        segs, l = [], 0
        while l < self.nlevels:
            if w[l] > LIM["NARROW"]:
                segs.append((l, l + 1, False))
                l += 1
                continue
            e = l + 1
            while e < self.nlevels and w[e] <= LIM["NARROW"]:
                e += 1
            segs.append((l, e, True))
            l = e
        return segs

    def runs(self, nrhs):
        """the pieces walk_levels cuts the one-workgroup segments into when a wave takes a row: (first level, end level, two phases)"""
        out = []
        for l0, l1, one_wg in self.segments(nrhs):
            a = l0
            while one_wg and a < l1:
                b = min(l1, a + LIM["TR64_RUN"])
                out.append((a, b, b - a >= LIM["TR64_RUN_MIN"]))
                a = b
        return out

    def prefix_stops(self, a, b):
        """for the rows of levels [a, b): (row, leading terms whose source lies below level a, all terms) -- where
        k_tri_run_prefix_rows / k_tri_run_prefix64 stop"""
        out = []
        for r in self.order[self.level_ptr[a]:self.level_ptr[b]]:
            lv = self.level[self.idx[self.ptr[r]:self.ptr[r + 1]]]
            inside = np.flatnonzero(lv >= a)
            out.append((int(r), int(inside[0]) if len(inside) else len(lv), len(lv)))
        return out


def model(T, kind, nrhs, options=None, guard=0):
    """what a fresh plan's first solve of nrhs right-hand sides does: ({field of csx_tri_route_info: value}, {kernel instance:
    launches}, the plan's model) -- tri_route, make_segments and walk_levels in the exact order; guard: not 0 for a plan in the
    rounding-equal order (csx_tri_set_order(plan, 0)) -- what the matrix-core guard will say once it is asked (1 passes, 2
    refuses, 3 NaN), which the model takes from the case: the guard's measure is the device's"""
    opt = dict(DEFAULT_OPTIONS, **(options or {}))
    n, Tp, Ti = T[0], T[1], T[2]
    P = PlanModel(n, Tp, Ti, kind)
    R = dict(route="Levels", lds=0, grid=0, G=0, waves=0, tile_rows=0, chunks=0, window=0, threads=0, rounds=0, mate=0)
    d = "fwd" if P.forward else "bwd"
    launches, asked = {}, [0]

    def done():
        info = dict(R, band=P.band, links=P.links, col_state=P.col_state, levels=P.nlevels if P.scheduled else 0,
                    sequential=int(P.sequential), chain_ok=int(P.chain_ok), ncomp=P.ncomp if P.comp_ok else 0,
                    comp_max=P.comp_max if P.comp_ok else 0, push_terms=P.push_terms, few_cpw=P.few_cpw, few_rows=P.few_rows,
                    few_terms=P.few_terms, guard=asked[0], schedule=P.schedule, comps_found=P.comps_found,
                    comp_rows_found=P.comp_rows_found, kind=KIND_ID[kind], n=n, terms=P.gnnz)
        return info, launches, P

    if opt["tri.components"]:
        P.analyse_components()
    if P.comp_ok and opt["tri.components"]:
        if guard and nrhs > LIM["PUSH_MAX_RHS"]:
            asked[0] = guard
            if guard == 1:
                R["route"] = "Ragged"
                launches["ragged"] = 1
                return done()
        G = 1
        while G < nrhs:
            G <<= 1
        R["G"] = G
        if nrhs <= LIM["PUSH_MAX_RHS"] and P.push_terms > 0 and opt["tri.push"]:
            R["lds"] = P.push_terms * 16 + P.comp_max * (16 + 8 * G) + 64
            if R["lds"] <= LIM["COMP_LDS_MAX"]:
                R.update(route="CompPush", grid=P.ncomp)
                launches["push_" + d] = 1
                return done()
        if nrhs <= LIM["FEW_MAX_RHS"] and P.few_cpw:
            R.update(route="FewLds", lds=few_lds_bytes(P.few_rows, P.few_terms, 64 // P.few_cpw),
                     grid=(P.ncomp + P.few_cpw - 1) // P.few_cpw)
            launches["few_lds_" + d] = 1
            return done()
        if nrhs <= LIM["FEW_MAX_RHS"]:
            cpw = 64 // G
            tile_rows = P.comp_max | 1
            per_wave = 64 * tile_rows * 8
            waves = max(1, min(4, LIM["FEW_TILE_LDS"] // per_wave))
            needed = (P.ncomp + cpw - 1) // cpw
            R.update(route="Few", tile_rows=tile_rows, waves=waves, lds=per_wave * waves, grid=(needed + waves - 1) // waves)
            launches["few_" + d] = 1
            return done()
        per_wave = P.comp_max * 64 * 8
        waves = tile_waves_per_workgroup(per_wave, LIM["TL_WAVES_MAX"])
        chunks = (nrhs + 63) // 64
        R.update(route="Local", waves=waves, chunks=chunks, lds=per_wave * waves, grid=(P.ncomp * chunks + waves - 1) // waves)
        launches["local_" + d] = 1
        return done()
    chain, small = False, n <= LIM["TC_MAX_N"]
    if opt["tri.columns"]:
        P.measure_band()
        chain = P.band != NOT_A_TRIANGLE and P.links * LIM["CHAIN_LINKS_NUM"] > n * LIM["CHAIN_LINKS_DEN"]
        Wn = 64
        while chain and Wn < P.band + LIM["WINDOW_SLACK"] and Wn < (1 << 20):
            Wn <<= 1
        if chain and Wn * 8 <= LIM["WINDOW_LDS_MAX"]:
            R.update(window=Wn, lds=Wn * 8)
            if not small and P.push and P.col_state == 1:
                R.update(route="WColumns", threads=1024 if P.gnnz > LIM["WCOL_WIDE_ENTRIES"] * n else 256)
                launches["wcolumns_%d" % R["threads"]] = 1
                return done()
            if not small and not P.push:
                R.update(route="WColChain", rounds=12 if P.gnnz > LIM["WCHAIN_WIDE_ENTRIES"] * n else 2)
                launches["wcolchain_%s_%d" % (kind[:2], R["rounds"])] = 1
                return done()
    where = opt["tri.levels_where"]
    if not (chain and small):
        P.ensure_schedule(where)
        if P.sequential:
            R["route"] = "Sequential"
            launches["sequential"] = 1
            return done()
    if opt["tri.columns"] and small and (chain or P.nlevels * LIM["CHAIN_LEVELS_NUM"] > n):
        P.ensure_col_state()
        if P.col_state == 1 and (n + 8) * 8 <= LIM["COLUMNS_LDS_MAX"]:
            R.update(route="Columns" if P.push else "ColChain", lds=(n + (8 if P.push else 0)) * 8,
                     threads=LIM["TC_THREADS"] if P.push else 64)
            launches[("columns_" + kind[0]) if P.push else ("colchain_" + kind[:2])] = 1
            return done()
    P.ensure_schedule(where)
    if P.sequential:
        R["route"] = "Sequential"
        launches["sequential"] = 1
        return done()
    # walk_levels
    long_rows = P.gnnz >= LIM["TRW_MIN_ROW"] * n and bool(opt["tri.row_waves"])
    by_rows = long_rows and nrhs <= LIM["TRW_MAX_RHS"]
    by_rows64 = long_rows and nrhs >= LIM["TR64_MIN_RHS"]
    names = ("level_rows64", "run_prefix64", "levels_rows64_one_wg") if by_rows64 else \
        ("level_rows", "run_prefix_rows", "levels_rows_one_wg")

    def bump(k):
        launches[k] = launches.get(k, 0) + 1

    for l0, l1, one_wg in P.segments(nrhs):
        if (by_rows or by_rows64) and one_wg:
            if not P.level_of_made and l1 - l0 >= LIM["TR64_RUN_MIN"]:
                P.level_of_made = True
                bump("level_of")
            a = l0
            while a < l1:
                b = min(l1, a + LIM["TR64_RUN"])
                if b - a >= LIM["TR64_RUN_MIN"]:
                    bump(names[1])
                bump(names[2])
                a = b
        elif by_rows or by_rows64:
            bump(names[0])
        elif one_wg and opt["tri.chain_walker"] and P.chain_ok:
            bump("chain")
        elif one_wg:
            bump("levels_one_wg")
        else:
            bump("level")
    return done()


# ---- the table ----------------------------------------------------------------------------------------------------------------
class Case:
    """one (matrix, kind, right-hand sides, options) and what it must do: `route` and the kernel instances `must` it launches;
    `edge`: what it sits on; `other`: the case on the other side; `alt`: options under which another route must give the same
    bytes; `facts`: fields of the model's route info the CPU test holds to these values (that is what 'sits on its edge' means)"""

    def __init__(self, name, system, kind, nrhs, route, must, edge, other=None, options=None, alt=(), facts=None, spoil=None,
                 check=None):
        self.name, self.system, self.kind, self.nrhs, self.route, self.must = name, system, kind, nrhs, route, tuple(must)
        self.edge, self.other, self.options, self.alt, self.facts = edge, other, dict(options or {}), tuple(alt), dict(facts or {})
        self.spoil, self.check = spoil, check
        self.id = "%s-%s-%d" % (name, kind, nrhs)
        self.seed = zlib.crc32(name.encode())

    @property
    def proper(self):
        return self.spoil is None


@functools.lru_cache(maxsize=None)
def _system(key):
    return SYSTEMS[key]()


@functools.lru_cache(maxsize=8)
def _matrix(key, kind, seed, spoil):
    T = to_matrix(_system(key), kind, seed)
    return misplace(T, kind in ("lsolve", "ltsolve"), *spoil) if spoil else T


def matrix(case):
    return _matrix(case.system, case.kind, case.seed, case.spoil)


@functools.lru_cache(maxsize=None)
def predicted(case_id):
    c = BY_ID[case_id]
    info, launches, P = model(matrix(c), c.kind, c.nrhs, c.options)
    return info, launches


def plan_model(case):
    return model(matrix(case), case.kind, case.nrhs, case.options)[2]


def rhs(case, nrhs=None):
    """the n-by-nrhs block of right-hand sides of a case"""
    rng = np.random.default_rng(case.seed + 1)
    return rng.uniform(-1.0, 1.0, (_system(case.system).n, nrhs or case.nrhs))


@functools.lru_cache(maxsize=8)
def oracle(case_id):
    """the plain-C oracle's solution of the case's block, column by column (computed once, shared, read-only)"""
    import c_oracle as CO
    c = BY_ID[case_id]
    n, Tp, Ti, Tx = matrix(c)
    B = rhs(c)
    X = np.stack([getattr(CO, c.kind)(n, Tp, Ti, Tx, B[:, r]) for r in range(c.nrhs)], axis=1)
    X.setflags(write=False)
    return X


NW = LIM["TC_MAX_N"] + 1                     # the smallest n whose x does not fit LDS
_W = LIM["NARROW"] + 1                       # a wide level at one right-hand side
_RUNS = (LIM["TR64_RUN_MIN"] - 1, LIM["TR64_RUN_MIN"], LIM["TR64_RUN"], LIM["TR64_RUN"] + 1)


def _rows_widths():
    """wide levels around runs of narrow ones of 7, 8, 64 and 65 levels; narrow at up to 65 right-hand sides, wide at one"""
    w = [_W]
    for k, run in enumerate(_RUNS):
        w += [3 if k < 2 else 2] * run + [_W]
    return w


def _rows_system(total_per_row):
    """average row length TRW_MIN_ROW (or one term short of it), rows of 1, 8, 9, 16, 17, 48, 49, 64, 65, 128 and 129 terms in the
    wide levels, and in the run of 8 narrow levels (levels 9 .. 16) the three outcomes of the prefix phase: a row of level 10
    whose only term is inside the run (it resumes at its start), the rows of level 9 (no term inside: the walker only
    divides) and a row of level 10 that stops after exactly 64 terms"""
    widths = _rows_widths()
    odd = (1, 8, 9, 16, 17, 48, 49, 64, 65, 128, 129)
    first_run = 1 + _RUNS[0] + 1                   # the first level of the run of 8
    specials = {(first_run + 1, 0): [(first_run, 0)],
                (first_run + 1, 1): [(0, i) for i in range(64)] + [(first_run, 1)]}

    def count(l, i):
        if widths[l] == _W and i < len(odd):
            return odd[i]
        return 26
    n = sum(widths)
    return layered(widths, count, specials, terms=total_per_row(n))


def _chain_system(remainder=None, far=12, extra=0):
    """a wide level of 520 rows (not a multiple of CHB), then ten narrow levels of 3: the chain walker's segment starts inside
    a block of 16 whose first 8 positions were solved by the wide level's launch.  Rows of the run take 12 rows from far
    back first and rows of their own block last.  remainder: the row (2, 0) takes a row of its block FIRST and then
    remainder - 1 rows from far back: a remainder of that many terms (gather kinds only); far, extra: every row of the run takes
    `far` rows from far back, the row (3, 0) `extra` more"""
    widths = [520] + [3] * 10
    specials = {}
    for l in range(1, 11):
        for i in range(3):
            a = 520 + 3 * (l - 1) + i
            near = sorted({(l - 1, i), (l - 1, (i + 1) % 3)}) if l > 1 else [512 + 2 * i, 513 + 2 * i]
            take = far + (extra if (l, i) == (3, 0) else 0)
            specials[(l, i)] = sorted(((a - 520) * 12 + t) % 500 for t in range(take)) + near
    if remainder:
        specials[(2, 0)] = [(1, 0)] + [(0, 3 * t) for t in range(remainder - 1)]
    return layered(widths, lambda l, i: 0, specials)


# columns of L' and U' on both sides of every count at which tch_chain_lds leaves its loop or wraps its prefetch, and of the two
# rounds k_tri_colchain and k_tri_wcolchain<., 2> fetch ahead (the common column has 2 entries)
_LISTS = tuple((1000 + 200 * k, c) for k, c in enumerate((15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193)))

_NO_COMPONENTS = {"tri.components": 0}     # (with 2 far rows a row the run and what it reads are one component of under 256 rows)


def _chain_ok_system(short):
    """the chain walker's own cut: terms from a row's first in-block source on, times 4, against all terms -- equal (the walker
    runs), or one term short of that (k_tri_levels_one_wg)"""
    P = model(to_matrix(_chain_system(far=2), "utsolve", 0), "utsolve", 1, _NO_COMPONENTS)[2]
    all_terms = len(P.idx)
    suffix = all_terms - int(P.npre.sum())
    assert 4 * suffix > all_terms
    return _chain_system(far=2, extra=4 * suffix - all_terms - short)


SYSTEMS = {
    "wband60": lambda: banded(NW, 64 - LIM["WINDOW_SLACK"]),
    "wband61": lambda: banded(NW, 64 - LIM["WINDOW_SLACK"] + 1),
    "wband124": lambda: banded(NW, 128 - LIM["WINDOW_SLACK"]),
    "wband125": lambda: banded(NW, 128 - LIM["WINDOW_SLACK"] + 1),
    "wband16380": lambda: banded(16400, LIM["WINDOW_LDS_MAX"] // 8 - LIM["WINDOW_SLACK"]),
    "wband16381": lambda: banded(16400, LIM["WINDOW_LDS_MAX"] // 8 - LIM["WINDOW_SLACK"] + 1),
    "col15360": lambda: banded(NW - 1, 508, long_lists=_LISTS, fans=((6000, 256), (8000, 257))),
    "wlong": lambda: banded(NW, 508, long_lists=_LISTS, fans=((6000, 256), (8000, 257))),
    "wheavy_push_above": lambda: banded(NW, 2044, avg=192, terms=LIM["WCOL_WIDE_ENTRIES"] * NW + 1,
                                        fans=((3000, 1024), (6000, 1025)), long_lists=((9000, 768), (11000, 769))),
    "wheavy_push_at": lambda: banded(NW, 508, avg=192, terms=LIM["WCOL_WIDE_ENTRIES"] * NW, fans=((3000, 256), (6000, 257))),
    "wheavy_gather_above": lambda: banded(NW, 1020, avg=159, terms=(LIM["WCHAIN_WIDE_ENTRIES"] - 1) * NW + 1,
                                          long_lists=((9000, 768), (11000, 769))),
    "wheavy_gather_at": lambda: banded(NW, 508, avg=159, terms=(LIM["WCHAIN_WIDE_ENTRIES"] - 1) * NW,
                                       long_lists=((9000, 128), (11000, 129))),
    # a chain by its links, 1 200 unknowns in runs of 12, a run's first unknown taking the first of the run two back (one component,
    # few levels): 1 101 links against 1 100 (12 * links > 11 * n)
    "links1101": lambda: System([[a - 1] if a % 12 or a > 12 * 98 else [a - 24] if a >= 24 else [] for a in range(1200)]),
    "links1100": lambda: System([[a - 1] if a % 12 else [a - 24] if a >= 24 else [] for a in range(1200)]),
    # a chain by its levels only: no links, every unknown takes the one 12 back: 21 levels of 241 against 20 of 240
    "bylevels241": lambda: System([[a - 12] if a >= 12 else [] for a in range(241)]),
    "bylevels240": lambda: System([[a - 12] if a >= 12 else [] for a in range(240)]),
    "chain_twice": lambda: System([[a - 1] * (2 if a == 100 else 1) if a else [] for a in range(240)]),
    "narrow512": lambda: layered([LIM["NARROW"]] * 3, lambda l, i: 3),
    "narrow513": lambda: layered([LIM["NARROW"] + 1] * 3, lambda l, i: 3),
    "narrow170x3": lambda: layered([170] * 3 + [300], lambda l, i: 3),
    "narrow171x3": lambda: layered([171] * 3 + [300], lambda l, i: 3),
    "rows24": lambda: _rows_system(lambda n: LIM["TRW_MIN_ROW"] * n),
    "rows23": lambda: _rows_system(lambda n: LIM["TRW_MIN_ROW"] * n - 1),
    "rows24_gather": lambda: _rows_system(lambda n: (LIM["TRW_MIN_ROW"] - 1) * n),
    "rows23_gather": lambda: _rows_system(lambda n: (LIM["TRW_MIN_ROW"] - 1) * n - 1),
    "chain_unaligned": lambda: _chain_system(),
    "chain_suf32": lambda: _chain_system(LIM["CH_SUF"]),
    "chain_suf33": lambda: _chain_system(LIM["CH_SUF"] + 1),
    "chain_ok_at": lambda: _chain_ok_system(0),
    "chain_ok_short": lambda: _chain_ok_system(1),
    "deep512": lambda: System([[a - 1] if a else [] for a in range(LIM["LV_MAX_ROUNDS"])]),
    "deep513": lambda: System([[a - 1] if a else [] for a in range(LIM["LV_MAX_ROUNDS"] + 1)]),
    "comps63": lambda: forest([5] * (LIM["COMP_MIN_COUNT"] - 1), density=0.5, seed=1),
    "comps64": lambda: forest([5] * LIM["COMP_MIN_COUNT"], density=0.5, seed=1),
    "comp256": lambda: forest([LIM["COMP_MAX_ROWS"]] + [3] * 63, density=0.02, seed=2),
    "comp257": lambda: forest([LIM["COMP_MAX_ROWS"] + 1] + [3] * 63, density=0.02, seed=2),
    "comp256_dense": lambda: forest([3] * 40 + [LIM["COMP_MAX_ROWS"]] + [3] * 40, dense=(40,), seed=3),
    "comp100x2_dense": lambda: forest([1] * 40 + [100, 100] + [1] * 40, dense=(40, 41), seed=4),
    "comps_twice": lambda: forest([9] * 80, density=0.4, seed=5, twice=(7, 5, 2)),
    "comps65_and_1": lambda: forest([65, 1] * 40, density=0.1, seed=6),
    "comps_mixed": lambda: forest([67, 1, 5, 130, 64, 2] * 14, density=0.15, seed=7),
    "one_chain": lambda: System([[a - 1] if a else [] for a in range(sum([67, 1, 5, 130, 64, 2] * 14))]),
    "strip_short": lambda: layered([300, 300], lambda l, i: 6, terms=(LIM["STRIP_SHORT_COLS"] - 1) * 600 - 1),
    "strip_long": lambda: layered([300, 300], lambda l, i: 6, terms=(LIM["STRIP_SHORT_COLS"] - 1) * 600),
    "malformed": lambda: layered([40, 40, 40], lambda l, i: 4),
}

LARGE = {k for k in SYSTEMS if k.startswith("w") or k == "col15360"}     # more than 15 000 unknowns

_FWD = {"lsolve": "fwd", "utsolve": "fwd", "ltsolve": "bwd", "usolve": "bwd"}


def _each(name, system, kinds, nrhs, route, must, edge, **kw):
    """a case per kind; route and must: one value, or (push kinds, gather kinds); in a kernel's name {d} is the direction, {k} the
    kind's letters"""
    out = []
    for kind in kinds:
        g = 0 if kind in PUSH else 1
        r = route if isinstance(route, str) else route[g]
        m = must if must and isinstance(must[0], str) else must[g]
        m = [s.format(d=_FWD[kind], k=kind[0] if kind in PUSH else kind[:2]) for s in m]
        out.append(Case(name, system, kind, nrhs, r, m, edge, **kw))
    return out


_WIN = ("WColumns", "WColChain")
_COL = ("Columns", "ColChain")
CASES = []
# -- the window of x
CASES += _each("wband60", "wband60", KINDS, 2, _WIN, (["wcolumns_256"], ["wcolchain_{k}_2"]),
               "band + WINDOW_SLACK = 64: the smallest window", other="wband61", facts={"window": 64},
               alt=({"tri.columns": 0},))
CASES += _each("wband61", "wband61", KINDS, 2, _WIN, (["wcolumns_256"], ["wcolchain_{k}_2"]),
               "band + WINDOW_SLACK = 65: the window doubles", other="wband60", facts={"window": 128})
CASES += _each("wband124", "wband124", KINDS, 1, _WIN, (["wcolumns_256"], ["wcolchain_{k}_2"]),
               "band + WINDOW_SLACK = 128", other="wband125", facts={"window": 128})
CASES += _each("wband125", "wband125", KINDS, 1, _WIN, (["wcolumns_256"], ["wcolchain_{k}_2"]),
               "band + WINDOW_SLACK = 129", other="wband124", facts={"window": 256})
CASES += _each("wband16380", "wband16380", KINDS, 1, _WIN, (["wcolumns_256"], ["wcolchain_{k}_2"]),
               "the largest window: exactly WINDOW_LDS_MAX", other="wband16381", facts={"window": LIM["WINDOW_LDS_MAX"] // 8})
CASES += _each("wband16381", "wband16381", KINDS, 1, "Levels", ["levels_one_wg"],
               "one more: no window fits and x does not fit LDS: the level schedule", other="wband16380", facts={"window": 0})
CASES += _each("wlong", "wlong", KINDS, 1, _WIN, (["wcolumns_256"], ["wcolchain_{k}_2"]),
               "columns of 256 / 257 entries in k_tri_wcolumns<256>, of 128 / 129 in k_tri_wcolchain<., 2>")
CASES += _each("wheavy_push_above", "wheavy_push_above", ("lsolve",), 1, _WIN, (["wcolumns_1024"], []),
               "one entry more than WCOL_WIDE_ENTRIES a column: 1 024 threads; columns of 1 024 / 1 025 entries",
               other="wheavy_push_at", facts={"threads": (1024, 0)})
CASES += _each("wheavy_push_above", "wheavy_push_above", ("ltsolve",), 1, _WIN, ([], ["wcolchain_{k}_12"]),
               "the same matrix as L': 12 rounds, columns of 768 / 769 entries", other="wheavy_gather_at", facts={"rounds": (0, 12)})
CASES += _each("wheavy_push_at", "wheavy_push_at", ("lsolve",), 1, _WIN, (["wcolumns_256"], []),
               "WCOL_WIDE_ENTRIES a column exactly: 256 threads", other="wheavy_push_above", facts={"threads": (256, 0)})
CASES += _each("wheavy_gather_above", "wheavy_gather_above", ("utsolve",), 1, _WIN, ([], ["wcolchain_{k}_12"]),
               "one entry more than WCHAIN_WIDE_ENTRIES a column: 12 rounds; columns of 768 / 769 entries",
               other="wheavy_gather_at", facts={"rounds": (0, 12)})
CASES += _each("wheavy_gather_above", "wheavy_gather_above", ("usolve",), 1, _WIN, (["wcolumns_256"], []),
               "the same matrix pushed, far below WCOL_WIDE_ENTRIES: 256 threads", facts={"threads": (256, 0)})
CASES += _each("wheavy_gather_at", "wheavy_gather_at", ("utsolve", "ltsolve"), 1, _WIN, ([], ["wcolchain_{k}_2"]),
               "WCHAIN_WIDE_ENTRIES a column exactly: 2 rounds", other="wheavy_gather_above", facts={"rounds": (0, 2)})
# -- x in LDS
CASES += _each("col15360", "col15360", KINDS, 2, _COL, (["columns_{k}"], ["colchain_{k}"]),
               "n = TC_MAX_N: x fits LDS (n + 1 is wlong); columns of 256 / 257 and of 128 / 129 entries", other="wlong",
               facts={"levels": 0}, alt=({"tri.columns": 0},))
CASES += _each("links1101", "links1101", KINDS, 1, _COL, (["columns_{k}"], ["colchain_{k}"]),
               "12 * links > 11 * n by one link: a chain without a schedule", other="links1100", facts={"levels": 0, "links": 1101})
CASES += _each("links1100", "links1100", KINDS, 1, "Levels", ["chain"],
               "12 * links = 11 * n: no chain, 61 levels: the level schedule", other="links1101",
               facts={"levels": 61, "links": 1100})
CASES += _each("bylevels241", "bylevels241", KINDS, 1, _COL, (["columns_{k}"], ["colchain_{k}"]),
               "no links, 12 * levels > n: a chain by its levels", other="bylevels240", facts={"levels": 21, "links": 0})
CASES += _each("bylevels240", "bylevels240", KINDS, 1, "Levels", ["levels_one_wg"],
               "no links, 12 * levels = n: the level schedule", other="bylevels241", facts={"levels": 20, "links": 0})
CASES += _each("chain_twice", "chain_twice", KINDS, 1, ("Levels", "ColChain"), (["levels_one_wg"], ["colchain_{k}"]),
               "a row twice in a column: L and U may not push it, L' and U' walk it in order", facts={"col_state": (2, 1)})
# -- the level schedule
CASES += _each("narrow512", "narrow512", KINDS, 1, "Levels", ["chain"], "rows * nrhs = NARROW: the levels join a run",
               other="narrow513")
CASES += _each("narrow513", "narrow513", KINDS, 1, "Levels", ["level"], "rows * nrhs = NARROW + 1: a launch each",
               other="narrow512", alt=({"tri.levels_where": 2},))
CASES += _each("narrow170x3", "narrow170x3", ("lsolve", "utsolve"), 3, "Levels", ["chain", "level"],
               "170 rows x 3 right-hand sides = 510: a run", other="narrow171x3")
CASES += _each("narrow171x3", "narrow171x3", ("lsolve", "utsolve"), 3, "Levels", ["level"],
               "171 rows x 3 right-hand sides = 513: wide", other="narrow170x3")
for _nrhs, _names in ((1, ("level_rows", "run_prefix_rows", "levels_rows_one_wg", "level_of")),
                      (LIM["TRW_MAX_RHS"], ("level_rows", "run_prefix_rows", "levels_rows_one_wg", "level_of")),
                      (LIM["TR64_MIN_RHS"], ("level_rows64", "run_prefix64", "levels_rows64_one_wg", "level_of")),
                      (64, ("level_rows64", "run_prefix64", "levels_rows64_one_wg", "level_of")),
                      (65, ("level_rows64", "run_prefix64", "levels_rows64_one_wg", "level_of"))):
    CASES += _each("rows24", "rows24", ("lsolve", "usolve"), _nrhs, "Levels", _names,
                   "TRW_MIN_ROW terms a row exactly: a wave a row; runs of 7, 8, 64 and 65 narrow levels", other="rows23",
                   check="runs")
    CASES += _each("rows24_gather", "rows24_gather", ("ltsolve", "utsolve"), _nrhs, "Levels", _names,
                   "the same for L' and U', whose count includes the diagonals", other="rows23_gather", check="runs")
for _nrhs in (1, LIM["TRW_MAX_RHS"], LIM["TR64_MIN_RHS"], 64, 65):
    CASES += _each("rows23", "rows23", ("lsolve", "usolve"), _nrhs, "Levels", ["level", "chain"],
                   "one term short of TRW_MIN_ROW a row: a thread per (row, right-hand side)", other="rows24")
    CASES += _each("rows23_gather", "rows23_gather", ("ltsolve", "utsolve"), _nrhs, "Levels", ["level", "chain"],
                   "one term short, L' and U'", other="rows24_gather")
CASES += _each("rows24_no_row_waves", "rows24", ("lsolve",), 1, "Levels", ["level", "chain"],
               "tri.row_waves = 0 on the same matrix: k_tri_level and the chain walker", options={"tri.row_waves": 0})
CASES += _each("rows24_no_chain_walker", "rows24", ("lsolve",), 1, "Levels", ["level", "levels_one_wg"],
               "tri.row_waves = 0, tri.chain_walker = 0: k_tri_levels_one_wg", options={"tri.row_waves": 0, "tri.chain_walker": 0})
CASES += _each("chain_unaligned", "chain_unaligned", KINDS, 1, "Levels", ["level", "chain"],
               "a chain walker's segment that starts at position 520 = 32 * 16 + 8, its first rows reading rows 512 .. 519",
               check="unaligned")
CASES += _each("chain_unaligned_64", "chain_unaligned", ("lsolve", "utsolve"), 64, "Levels", ["level", "chain"],
               "64 right-hand sides: one chunk of the walker's lanes", other="chain_unaligned_65")
CASES += _each("chain_unaligned_65", "chain_unaligned", ("lsolve", "utsolve"), 65, "Levels", ["level", "chain"],
               "65 right-hand sides: a second chunk with one live lane", other="chain_unaligned_64")
CASES += _each("chain_suf32", "chain_suf32", ("ltsolve", "utsolve"), 1, "Levels", ["level", "chain"],
               "a remainder of CH_SUF terms: all staged in LDS", other="chain_suf33", check="remainder")
CASES += _each("chain_suf33", "chain_suf33", ("ltsolve", "utsolve"), 1, "Levels", ["level", "chain"],
               "a remainder of CH_SUF + 1 terms: the last one from memory", other="chain_suf32", check="remainder")
CASES += _each("chain_ok_at", "chain_ok_at", KINDS, 1, "Levels", ["level", "chain"],
               "4 * (terms behind the first in-block source) = all terms: the chain walker", other="chain_ok_short",
               facts={"chain_ok": 1}, options=_NO_COMPONENTS)
CASES += _each("chain_ok_short", "chain_ok_short", KINDS, 1, "Levels", ["level", "levels_one_wg"],
               "one term fewer: the plain walker", other="chain_ok_at", facts={"chain_ok": 0}, options=_NO_COMPONENTS)
# -- where the schedule comes from
CASES += _each("deep512", "deep512", ("lsolve", "ltsolve"), 1, "Levels", ["levels_one_wg"],
               "LV_MAX_ROUNDS levels on the device pass", other="deep513", facts={"schedule": 2, "levels": LIM["LV_MAX_ROUNDS"]},
               options={"tri.columns": 0, "tri.levels_where": 2})
CASES += _each("deep513", "deep513", ("lsolve", "ltsolve"), 1, "Levels", ["levels_one_wg"],
               "one level more: the device pass gives up and the host pass says so", other="deep512",
               facts={"schedule": 4, "levels": LIM["LV_MAX_ROUNDS"] + 1}, options={"tri.columns": 0, "tri.levels_where": 2})
CASES += _each("deep512_host", "deep512", ("lsolve",), 1, "Levels", ["levels_one_wg"], "the host pass", facts={"schedule": 3},
               options={"tri.columns": 0})
# -- forests of small components
CASES += _each("comps63", "comps63", KINDS, 1, "Levels", ["chain"],
               "COMP_MIN_COUNT - 1 components: no component sweep", other="comps64", facts={"ncomp": 0, "comps_found": 63})
CASES += _each("comps64", "comps64", KINDS, 1, ("CompPush", "FewLds"), (["push_{d}"], ["few_lds_{d}"]),
               "COMP_MIN_COUNT components", other="comps63", facts={"ncomp": 64},
               alt=({"tri.components": 0}, {"tri.push": 0}))
CASES += _each("comp256", "comp256", KINDS, 1, ("CompPush", "FewLds"), (["push_{d}"], ["few_lds_{d}"]),
               "a largest component of COMP_MAX_ROWS rows", other="comp257", facts={"comp_max": 256})
CASES += _each("comp257", "comp257", KINDS, 1, _COL, (["columns_{k}"], ["colchain_{k}"]),
               "one row more: no component sweep", other="comp256", facts={"ncomp": 0, "comp_rows_found": 257})
for _nrhs, _route, _must in ((8, ("CompPush", "FewLds"), (["push_{d}"], ["few_lds_{d}"])), (9, "FewLds", ["few_lds_{d}"]),
                             (32, "FewLds", ["few_lds_{d}"]), (33, "Local", ["local_{d}"]), (64, "Local", ["local_{d}"]),
                             (65, "Local", ["local_{d}"]), (128, "Local", ["local_{d}"]), (129, "Local", ["local_{d}"])):
    CASES += _each("comps_mixed", "comps_mixed", KINDS if _nrhs in (8, 33) else ("lsolve", "ltsolve"), _nrhs, _route, _must,
                   "PUSH_MAX_RHS / FEW_MAX_RHS / blocks of 64 right-hand sides, on both sides",
                   facts={"chunks": (_nrhs + 63) // 64 if _nrhs > LIM["FEW_MAX_RHS"] else 0},
                   alt=({"tri.components": 0},) if _nrhs in (8, 33) else ())
CASES += _each("comp256_dense", "comp256_dense", KINDS, 1, "Few", ["few_{d}"],
               "a full component of COMP_MAX_ROWS rows: the push program and the all-in-LDS programs exceed COMP_LDS_MAX; a wave's "
               "tile of 257 rows exceeds FEW_TILE_LDS: one wave", facts={"tile_rows": 257, "waves": 1, "few_cpw": 0})
CASES += _each("comp100x2_dense_8", "comp100x2_dense", PUSH, 8, "CompPush", ["push_{d}"],
               "two full components of 100 rows side by side: one fits the push program", other="comp100x2_dense_9")
CASES += _each("comp100x2_dense_9", "comp100x2_dense", PUSH, 9, "Few", ["few_{d}"],
               "... a group of four does not fit the all-in-LDS kernel: k_tri_few, two waves", other="comp100x2_dense_8",
               facts={"few_cpw": 0, "tile_rows": 101, "waves": 2})
CASES += _each("comp100x2_dense_9", "comp100x2_dense", ("ltsolve", "utsolve"), 9, "Few", ["few_{d}"],
               "the same for L' and U' (no push program at any count)", facts={"few_cpw": 0, "tile_rows": 101, "waves": 2})
CASES += _each("comps_twice", "comps_twice", PUSH, 1, "FewLds", ["few_lds_{d}"],
               "a row twice in a column: no push program", facts={"col_state": 2, "push_terms": 0})
CASES += _each("comps65_and_1", "comps65_and_1", KINDS, 64, "Local", ["local_{d}"],
               "components of 65 rows alternating with singletons: launched biggest first")
# -- not a triangle
CASES += _each("malformed", "malformed", ("lsolve",), 3, "Sequential", ["sequential"],
               "an entry above the diagonal in a slot of L that is not the first", spoil=(10, 7), facts={"sequential": 1})
CASES += _each("malformed", "malformed", ("usolve",), 3, "Sequential", ["sequential"],
               "an entry below the diagonal in a slot of U that is not the last", spoil=(109, 112), facts={"sequential": 1})
CASES += _each("malformed_device", "malformed", ("lsolve",), 1, "Sequential", ["sequential"],
               "the same, found by the device pass", spoil=(10, 7), facts={"sequential": 1, "schedule": 2},
               options={"tri.levels_where": 2})
# -- analyse: the diagonals of L stripped 4 lanes a column, or 64
CASES += _each("strip_short", "strip_short", ("lsolve",), 1, "Levels", ["chain"], "nnz = STRIP_SHORT_COLS * n - 1: k_strip_first<4>",
               other="strip_long", check="strip")
CASES += _each("strip_long", "strip_long", ("lsolve",), 1, "Levels", ["chain"], "nnz = STRIP_SHORT_COLS * n: k_strip_first<64>",
               other="strip_short", check="strip")

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
IDS = [c.id for c in CASES]

# the pairs of csx_lusol_solve / csx_lusol_solve_trans: (name, system of L, system of U, nrhs, fused)
LU_PAIRS = (("local+local", "comps_mixed", "comps_mixed", 33, True),
            ("local+chain", "comps_mixed", "one_chain", 33, False),
            ("chain+local", "one_chain", "comps_mixed", 40, False),
            ("few+few", "comps_mixed", "comps_mixed", 32, False))

# ---- the rounding-equal order ---------------------------------------------------------------------------------------------------
# csx_tri_set_order(plan, 0) with more than PUSH_MAX_RHS right-hand sides on a forest of components of at most 80 rows: the
# matrix-core sweep, equal to the oracle to rounding (tests/tol.py TRI_EPS_UNITS), unless the growth guard refuses; then, and at
# PUSH_MAX_RHS right-hand sides, the exact routes with the oracle's bytes.
class Rounding:
    """guard: what the matrix-core guard must say (0: not asked, 1 passes, 2 refuses, 3 NaN); spoil: "growth" -- two components get
    off-diagonals of 4 (deliberately NOT dominant: inverses of their diagonal tiles grow like 4^k), "nan" -- a NaN next to the
    diagonal in the first tile of the first and of the last component (the guard measures diagonal tiles only)"""

    def __init__(self, name, system, kind, nrhs, guard, route, must, spoil=None):
        self.name, self.system, self.kind, self.nrhs, self.guard, self.route, self.must = name, system, kind, nrhs, guard, route, must
        self.spoil, self.options = spoil, {}
        self.id = "%s-%s-%d" % (name, kind, nrhs)
        self.seed = zlib.crc32(name.encode())


_RAG_SIZES = [67, 1, 5, 16, 17, 64, 2, 80, 33, 48, 49, 32, 65] * 7
SYSTEMS["rag"] = lambda: forest(_RAG_SIZES, density=0.2, seed=8)
SYSTEMS["rag81"] = lambda: forest([81] + [5] * 70, density=0.2, seed=9)
ROUNDING = []
for _k in KINDS:
    _d = _FWD[_k]
    ROUNDING += [Rounding("rag", "rag", _k, LIM["PUSH_MAX_RHS"] + 1, 1, "Ragged", ["ragged"]),
                 Rounding("rag", "rag", _k, 70, 1, "Ragged", ["ragged"]),
                 Rounding("rag_few", "rag", _k, LIM["PUSH_MAX_RHS"], 0, "CompPush" if _k in PUSH else "FewLds",
                          ["push_" + _d if _k in PUSH else "few_lds_" + _d]),
                 Rounding("rag81", "rag81", _k, 40, 2, "Local", ["local_" + _d]),
                 Rounding("rag_growth", "rag", _k, 9, 2, "FewLds", ["few_lds_" + _d], spoil="growth"),
                 Rounding("rag_nan", "rag", _k, 9, 3, "FewLds", ["few_lds_" + _d], spoil="nan")]
ROUNDING_BY_ID = {r.id: r for r in ROUNDING}
ROUNDING_MEASURED = [r.id for r in ROUNDING if r.route == "Ragged"]


@functools.lru_cache(maxsize=8)
def rounding_matrix(rid):
    r = ROUNDING_BY_ID[rid]
    n, Tp, Ti, Tx = to_matrix(_system(r.system), r.kind, r.seed)
    Tx = Tx.copy()
    col = np.repeat(np.arange(n), np.diff(Tp.astype(np.int64)))
    if r.spoil == "growth":
        near = (np.abs(Ti - col) == 1) & (((Ti < 20) & (col < 20)) | ((Ti >= n - 20) & (col >= n - 20)))
        assert near.sum() >= 19
        Tx[near] = 4.0
    elif r.spoil == "nan":
        ends = ((Ti + col == 1) | (Ti + col == 2 * n - 3)) & (np.abs(Ti - col) == 1)     # inside the first diagonal tile of a component
        assert ends.sum() == 1 + (_RAG_SIZES[-1] > 1)
        Tx[ends] = np.nan
    return n, Tp, Ti, Tx


def rounding_rhs(r):
    return np.random.default_rng(r.seed + 1).uniform(-1.0, 1.0, (_system(r.system).n, r.nrhs))


def substitution(T, kind, B, x=None):
    """x is None: the solution of the kind's system for the block B by substitution in numpy.longdouble, the unknowns in solve
    order.  With x (a solution): sum|terms| of the substitution that formed each of its components,
    (|b_a| + sum_s |t_as x_s|) / |t_aa| -- tol.cholsolve_terms' measure for any kind.  x = "carry": what an error of size B in
    the right-hand side can become in the solution, z_a = (|b_a| + sum_s |t_as| z_s) / |t_aa| (|inv(T)| v <= inv(M(T)) v)"""
    n, Tp, Ti, Tx = T
    P = PlanModel(n, Tp, Ti, kind)
    wide = np.longdouble if x is None else np.float64
    val, dg = Tx.astype(wide)[P.val_at], Tx.astype(wide)[P.diag_at]
    out = np.array(B, dtype=wide)
    if x is not None:
        val, dg, out = np.abs(val), np.abs(dg), np.abs(out)
        x = out if isinstance(x, str) else np.abs(x)
    for a in (range(n) if P.forward else range(n - 1, -1, -1)):
        b, e = P.ptr[a], P.ptr[a + 1]
        if x is None:
            if e > b:
                out[a] -= val[b:e] @ out[P.idx[b:e]]
            out[a] /= dg[a]
        else:
            if e > b:
                out[a] += val[b:e] @ x[P.idx[b:e]]
            out[a] /= dg[a]
    return out


@functools.lru_cache(maxsize=8)
def rounding_reference(rid):
    """(the oracle's solution, the longdouble one, sum|terms|) of a rounding case, computed once"""
    import c_oracle as CO
    r = ROUNDING_BY_ID[rid]
    T, B = rounding_matrix(rid), rounding_rhs(r)
    n, Tp, Ti, Tx = T
    X = np.stack([getattr(CO, r.kind)(n, Tp, Ti, Tx, B[:, c]) for c in range(r.nrhs)], axis=1)
    if r.spoil == "nan":
        return X, None, None
    return X, substitution(T, r.kind, B), substitution(T, r.kind, B, X)


def eps_units(rid, got):
    """the largest |got - oracle| / (EPS * sum|terms|) over the block"""
    X, _, terms = rounding_reference(rid)
    return float(np.max(np.abs(np.asarray(got, np.float64) - X) / (2.0 ** -52 * terms)))


def oracle_eps_units(rid):
    """the plain-C oracle's own distance from the longdouble solution, in the same units"""
    X, exact, terms = rounding_reference(rid)
    return float(np.max(np.abs(X.astype(np.longdouble) - exact) / (np.longdouble(2.0 ** -52) * terms)))


# ---- two solves in a row in the rounding-equal order ----------------------------------------------------------------------------
# PAIRS: csx_lusol_solve / csx_lusol_solve_trans on two forests with both plans in the rounding-equal order (the fused ragged tier),
# and cholsol_factor(exact=False) on a band of half-width CHOL_BAND (its plan's two triangular plans in the relaxed order: L' on
# the rows of L -- k_tri_wcolumns, mate -- or, with "tri.columns" = 0, both on the level walk with the schedule from the
# elimination tree's hint and k_tri_chain in the relaxed order).  Held to TRI_EPS_UNITS of the terms of both substitutions
# (two_solves).
PAIR_NRHS = 33
CHOL_N, CHOL_BAND, CHOL_NRHS = 2000, 20, 12      # (under TRW_MIN_ROW terms a row: no wave per row)
PAIRS = ("lu_rag-lusol", "lu_rag-lusol_trans", "cholband-mate", "cholband-levels")


def lu_rag():
    """(L, U, pinv, q, B) of the fused ragged pair"""
    L, U = to_matrix(_system("rag"), "lsolve", 1), to_matrix(_system("rag"), "usolve", 2)
    rng = np.random.default_rng(12)
    n = L[0]
    return L, U, rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32), rng.uniform(-1.0, 1.0, (n, PAIR_NRHS))


def chol_band():
    """(n, p, i, x) of a symmetric positive definite band matrix (both triangles, rows ascending) and its block of right-hand sides"""
    rng = np.random.default_rng(13)
    offs = [rng.uniform(-1.0, 1.0, CHOL_N - d) / (2.5 * CHOL_BAND) for d in range(1, CHOL_BAND + 1)]
    A = sp.diags([rng.uniform(1.0, 2.0, CHOL_N)] + offs + offs, [0] + list(range(1, CHOL_BAND + 1)) + [-d for d in range(1, CHOL_BAND + 1)],
                 format="csc")
    A.sort_indices()
    return (CHOL_N, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()), rng.uniform(-1.0, 1.0, (CHOL_N, CHOL_NRHS))


def two_solves(T1, kind1, T2, kind2, B):
    """(the oracle's result of solve 1 then solve 2 on the block B, the same in numpy.longdouble, the terms): sum|terms| of the
    last substitution, as tol.cholsolve_terms takes them, plus what the roundings of the first solve -- so many of ITS terms --
    can become on their way through the second: an error dy in y moves x by |inv(T2)| dy <= inv(M(T2)) dy.  In these units two
    solves in a row are held to the same number of roundings as one."""
    import c_oracle as CO
    Y = np.stack([getattr(CO, kind1)(T1[0], *T1[1:], B[:, c]) for c in range(B.shape[1])], axis=1)
    X = np.stack([getattr(CO, kind2)(T2[0], *T2[1:], Y[:, c]) for c in range(B.shape[1])], axis=1)
    terms = substitution(T2, kind2, Y, X) + substitution(T2, kind2, substitution(T1, kind1, B, Y), "carry")
    return X, substitution(T2, kind2, substitution(T1, kind1, B)), terms


def pair_units(got, X, terms):
    return float(np.max(np.abs(np.asarray(got, np.longdouble) - X) / (np.longdouble(2.0 ** -52) * terms)))


def pair_oracle_units(name):
    """the plain-C oracle's own distance from the longdouble result of a pair, in roundings of the last substitution's terms (for
    the band: on the oracle's own factor)"""
    import c_oracle as CO
    if name.startswith("lu_rag"):
        L, U, pinv, q, B = lu_rag()
        if name.endswith("trans"):
            X, exact, terms = two_solves(U, "utsolve", L, "ltsolve", B[q])
        else:
            Bp = np.empty_like(B)
            Bp[pinv] = B
            X, exact, terms = two_solves(L, "lsolve", U, "usolve", Bp)
    else:
        (n, Ap, Ai, Ax), B = chol_band()
        parent, cp = CO.schol(n, Ap, Ai)
        L = (n,) + tuple(CO.chol(n, Ap, Ai, Ax, parent, cp))
        X, exact, terms = two_solves(L, "lsolve", L, "ltsolve", B)
    return pair_units(exact, X, terms)


# kernel instances of csx_tri_launches that no case launches, with the reason
UNREACHED = {}
# what the issue names and no case here reaches, with the reason
NOT_REACHED = {}
