"""Inputs shared by the Householder QR tests: for every case the matrix A (m x n) as raw CSC arrays, the order
given to cs_sqr, two new value sets on A's pattern and one with a NaN for the breaking refactor; and, without a device, the
matrix that is factored (A, or A' when m < n) with cs_sqr's analysis of it.

New values are A2 = D1 A D2 with D = diag(1 + 1e-3 u), u uniform in [-1, 1] from a committed seed, applied entry by entry, so of
duplicate entries the last still wins and an exact zero stays one.  The breaking set (Case.breaking) has a NaN in the last stored
entry of the column of the factored matrix that is eliminated first: every row of that column is a slot of V(:,0), so R(0,0) is
not finite.  (A NaN elsewhere can land in a slot of R whose reflection touches no other row, and break nothing.)

The analysis is made here from the host functions alone (csx_order_nd_host on the pattern of A'A formed with numpy, then
csx_sqr_host), so that the CPU tests need no device; the GPU tests take the solver's own `symbolic` instead, whatever column
order the product's cs_amd gives."""
import os

import numpy as np

import _csx
from slu_cases import CONVECTION, SIGMA, csc, grid, with_dups

WINDOW, RUN_LEVELS = _csx.hqr_window()   # LDS window in slots and levels per walker launch, asked of the library (no GPU needed)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Analysis(object):
    """the factored matrix F (mf x nf, mf >= nf) as CSC arrays, `perm` (F's storage order as positions of A's), and cs_sqr's
    q / parent / pinv / leftmost / m2 / vnz / rnz of it"""


class Case(object):
    def __init__(self, name, m, n, p, i, x, order=0, seed=1, solvable=True):
        self.name, self.m, self.n, self.order, self.solvable = name, int(m), int(n), order, solvable
        self.p = np.asarray(p, np.int32)
        self.i = np.asarray(i, np.int32)
        self.x = np.asarray(x, np.float64)
        self.cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.p))
        self.A2 = [self.scaled(seed * 100 + k) for k in (1, 2)]
        self._analysis = None

    def scaled(self, seed):
        rng = np.random.default_rng(seed)
        d1 = 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, self.m)
        d2 = 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, self.n)
        return d1[self.i] * self.x * d2[self.cols]

    def values(self, which):
        return self.x if which == "A" else self.A2[which]

    def breaking(self, col0=None):
        """A's values with a NaN in the last stored entry of column col0 of the factored matrix (default: the column this
        file's analysis eliminates first)"""
        if col0 is None:
            S = self.analysis
            col0 = 0 if S.q is None else int(S.q[0])
        bad = self.x.copy()
        bad[self.p[col0 + 1] - 1 if self.m >= self.n else np.flatnonzero(self.i == col0)[-1]] = np.nan
        return bad

    def matrix(self, mod, x=None):
        """a `cs` of module mod with A's pattern and the values x (default A's own)"""
        x = self.x if x is None else x
        A = mod.cs_spalloc(self.m, self.n, max(len(self.i), 1), True, False)
        A.p, A.i, A.x = self.p.tolist(), (self.i.tolist() or [0]), (np.asarray(x, np.float64).tolist() or [0.0])
        return A

    def dense(self, x=None):
        """the matrix the factorisation sees: of duplicates the last"""
        x = self.x if x is None else x
        D = np.zeros((self.m, self.n))
        for k in range(len(self.i)):
            D[self.i[k], self.cols[k]] = x[k]
        return D

    @property
    def analysis(self):
        if self._analysis is None:
            self._analysis = analyse(self)
        return self._analysis


def analyse(case, order=None):
    lib = _csx.load()
    S = Analysis()
    order = case.order if order is None else order
    if case.m >= case.n:
        S.m, S.n, S.p, S.i, S.perm = case.m, case.n, case.p, case.i, np.arange(len(case.i))
    else:                                       # A' as cs_transpose stores it: rows become columns, stable
        S.m, S.n = case.n, case.m
        S.perm = np.argsort(case.i, kind="stable")
        S.i = np.ascontiguousarray(case.cols[S.perm].astype(np.int32))
        S.p = np.concatenate([[0], np.cumsum(np.bincount(case.i, minlength=case.m))]).astype(np.int32)
    m, n = S.m, S.n
    fcols = np.repeat(np.arange(n), np.diff(S.p))
    S.q = None
    cp, ci = S.p, S.i
    if order:
        assert order == 3
        B = np.zeros((m, n), np.int64)
        B[S.i, fcols] = 1
        G = (B.T @ B) > 0
        gp = np.concatenate([[0], np.cumsum(G.sum(axis=0))]).astype(np.int32)
        gi = np.ascontiguousarray(np.nonzero(G.T)[1].astype(np.int32))        # column by column, rows ascending
        q = np.empty(max(n, 1), np.int32)
        assert lib.csx_order_nd_host(n, _csx.pi(gp), _csx.pi(gi), _csx.pi(q)) == _csx.OK
        S.q = q[:n]
        assert sorted(S.q.tolist()) == list(range(n))
        counts = np.diff(S.p)[S.q]
        cp = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        ci = np.ascontiguousarray(np.concatenate([S.i[S.p[c]:S.p[c + 1]] for c in S.q] or [np.zeros(0, np.int32)]).astype(np.int32))
    parent, cnt = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
    pinv, leftmost = np.empty(max(m + n, 1), np.int32), np.empty(max(m, 1), np.int32)
    m2, vnz, rnz = _csx.C.c_int32(0), _csx.C.c_int64(0), _csx.C.c_int64(0)
    ci_arg = ci if len(ci) else np.zeros(1, np.int32)
    assert lib.csx_sqr_host(m, n, _csx.pi(cp), _csx.pi(ci_arg), _csx.pi(parent), _csx.pi(cnt), _csx.pi(pinv), _csx.pi(leftmost),
                            m2, vnz, rnz) == _csx.OK
    S.parent, S.pinv, S.leftmost = parent[:n].copy(), pinv[:m].copy(), leftmost[:m].copy()
    S.m2, S.vnz, S.rnz = int(m2.value), int(vnz.value), int(rnz.value)
    return S


def dense_cols(m, ncols, seed):
    """a dense m x ncols matrix, entries uniform in [-1, 1] from a committed seed"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, m * ncols)
    return m, ncols, np.arange(0, m * ncols + 1, m), np.tile(np.arange(m), ncols), x


def rect(m, n, entries):
    """CSC arrays (rows ascending) of {(i, j): v} for an m x n matrix"""
    _, p, i, x = csc(n, entries)
    return m, n, p, i, x


def _blocks(count, seed):
    rng = np.random.default_rng(seed)
    e = {}
    for b in range(count):
        for r in range(3):
            for c in range(2):
                e[(3 * b + r, 2 * b + c)] = float(rng.uniform(-1.0, 1.0))
    return rect(3 * count, 2 * count, e)


def _bidiagonal(n):
    e = {(j, j): 0.5 + 0.01 * (j % 7) for j in range(n)}
    e.update({(j + 1, j): -1.0 + 0.02 * (j % 5) for j in range(n)})
    return rect(n + 1, n, e)


def _chains(count, length=3):
    """block diagonal: `count` disjoint bidiagonal blocks of length + 1 rows and `length` columns, so every height level of the
    column elimination tree has `count` columns"""
    e = {}
    for c in range(count):
        for t in range(length):
            i, j = c * (length + 1) + t, c * length + t
            e[(i, j)] = 0.5 + 0.125 * c + 0.01 * t
            e[(i + 1, j)] = -1.0 + 0.02 * t
    return rect(count * (length + 1), count * length, e)


def _long(rows, second):
    """a dense first column of `rows` rows; second: a second column with entries in rows 0 and 1"""
    rng = np.random.default_rng(rows)
    e = {(r, 0): float(rng.uniform(0.5, 1.5)) for r in range(rows)}
    if second:
        e[(0, 1)], e[(1, 1)] = 2.0, -1.5
    return rect(rows, 2 if second else 1, e)


def _stacked(g):
    """the shifted g x g grid with the plain one stacked under it: 2 g^2 x g^2"""
    n, p, i, x = grid(g, sigma=SIGMA)
    _, p2, i2, x2 = grid(g)
    e = {}
    for src, off in (((p, i, x), 0), ((p2, i2, x2), n)):
        sp, si, sx = src
        for j in range(n):
            for t in range(sp[j], sp[j + 1]):
                e[(si[t] + off, j)] = sx[t]
    return rect(2 * n, n, e)


def _golden(name, key="A"):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return int(g[key + "_mn"][0]), int(g[key + "_mn"][1]), g[key + "_p"], g[key + "_i"], g[key + "_x"]


def _square(t):
    n, p, i, x = t
    return n, n, p, i, x


def _build():
    cases = []
    add = cases.append
    add(Case("one", 1, 1, [0, 1], [0], [-3.0], seed=1))                                   # head <= 0, tail2 == 0: beta 2
    add(Case("three-by-one", 3, 1, [0, 3], [0, 1, 2], [1.0, 2.0, -2.0], seed=2))
    add(Case("diagonal", 5, 5, np.arange(6), np.arange(5), [1.0, -2.0, 0.0, -4.0, 5.0], seed=3, solvable=False))
    for k, m in enumerate((64, 65, 66, 130)):                                            # tails of 63, 64, 65, 129
        add(Case("dense%d" % m, *dense_cols(m, 2, 20241000 + m), seed=4 + k))
    add(Case("blocks", *_blocks(300, 20241003), seed=8))
    add(Case("bidiagonal", *_bidiagonal(RUN_LEVELS + 1), seed=9))                        # 257 levels of one column
    add(Case("long-column", *_long(WINDOW + 1, False), seed=10))
    add(Case("long-column-updated", *_long(WINDOW + 2, True), seed=11))
    add(Case("empty-row", *rect(3, 3, {(0, 0): 1.0, (1, 0): 1.0, (0, 1): 1.0, (1, 1): 2.0, (0, 2): 1.0, (1, 2): 3.0}), seed=12,
             solvable=False))
    add(Case("dups", *_square(with_dups(*grid(6, sigma=SIGMA), 14)), seed=13))
    add(Case("ash219", *_golden("ash219"), seed=14))
    add(Case("lp_afiro", *_golden("lp_afiro"), seed=15))
    add(Case("west", *_golden("west0067", "C"), order=0, seed=16))
    add(Case("west-nd", *_golden("west0067", "C"), order=3, seed=17))
    add(Case("grid24-shift-natural", *_square(grid(24, sigma=SIGMA)), order=0, seed=18))
    add(Case("grid24-shift", *_square(grid(24, sigma=SIGMA)), order=3, seed=19))
    add(Case("stacked", *_stacked(24), order=0, seed=20))
    add(Case("chains4", *_chains(4), seed=21))       # three levels of 4 columns: the widest the walker takes
    add(Case("chains5", *_chains(5), seed=22))       # ... of 5: a wave per column
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
VALUE_SETS = ("A", 0, 1)
SQUARE = [c.name for c in CASES if c.m == c.n and c.solvable]
assert CONVECTION == 0.3

# Right-hand sides: BASE columns uniform in [-1, 1] from a committed seed, as rows of the returned array; wider blocks repeat them
# scaled by powers of two (exact: every operation of a solve scales with it), so every column of every block is one the CPU
# test has held to its condition, and a column that lands in the wrong place is still seen.
RHS_SEED, BASE = 20241017, 3


def rhs(case, k=BASE, rows=None):
    rows = case.m if rows is None else rows
    base = np.random.default_rng(RHS_SEED).uniform(-1.0, 1.0, (BASE, rows))
    return np.stack([base[c % BASE] * 2.0 ** (c // BASE) for c in range(k)])
