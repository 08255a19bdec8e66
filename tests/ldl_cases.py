"""Inputs shared by the LDL' tests: for every case the symmetric indefinite matrix A as raw CSC arrays (the upper
triangle; in `dups` stray duplicates and a lower triangle too), the order, the perturbation, two new value sets on A's pattern
and one that breaks down.

New values are A2 = D A D with D = diag(1 + 1e-3 u), u uniform in [-1, 1] from a committed seed: a congruence keeps the inertia,
and the formula is applied entry by entry, so of duplicate entries the last still wins and lower entries stay ignored.
The breaking value set has the diagonal entry of ONE column set to 0.0 (every stored copy of it), the column otherwise kept:
the column that is eliminated first -- column 0 in natural order, perm[0] under an ordering (Case.breaking(j0)) -- so that its
pivot is that entry itself.  Where the case runs with a perturbation a zero pivot is perturbed, not a breakdown: the entry is
+inf there (so is |S|_1 and with it the threshold), which no perturbation mends."""
import numpy as np

import _csx
from chol_refactor_cases import arrow_blocks, grid_upper, with_dups_and_lower

SIGMA = 3.7
WINDOW = _csx.ldl_window()   # entries of a column that the column kernels keep in LDS, asked of the library (no GPU needed)


class Case(object):
    def __init__(self, name, n, p, i, x, order=0, perturb=0.0, seed=1, breaks=False):
        self.name, self.n, self.order, self.perturb = name, int(n), order, perturb
        self.breaks = breaks                   # A itself breaks down at perturb = 0
        self.p = np.asarray(p, np.int32)
        self.i = np.asarray(i, np.int32)
        self.x = np.asarray(x, np.float64)
        self.cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.p))
        self.A2 = [self.congruent(seed * 100 + k) for k in (1, 2)]

    def congruent(self, seed):
        d = 1.0 + 1e-3 * np.random.default_rng(seed).uniform(-1.0, 1.0, self.n)
        return d[self.i] * self.x * d[self.cols]

    def values(self, which):
        return self.x if which == "A" else self.A2[which]

    def breaking(self, j0=0):
        bad = self.x.copy()
        on = (self.cols == j0) & (self.i == j0)
        assert on.any()
        bad[on] = np.inf if self.perturb > 0.0 else 0.0
        return bad

    def matrix(self, mod, x=None):
        """a `cs` of module mod with A's pattern and the values x (default A's own)"""
        x = self.x if x is None else x
        A = mod.cs_spalloc(self.n, self.n, max(len(self.i), 1), True, False)
        A.p, A.i, A.x = self.p.tolist(), (self.i.tolist() or [0]), (np.asarray(x, np.float64).tolist() or [0.0])
        return A

    def dense(self, x=None):
        """the symmetric matrix the factorisation sees: entries with row <= column, of duplicates the last, mirrored"""
        x = self.x if x is None else x
        U = np.zeros((self.n, self.n))
        for k in range(len(self.i)):
            if self.i[k] <= self.cols[k]:
                U[self.i[k], self.cols[k]] = x[k]
        return U + np.triu(U, 1).T


def upper_csc(n, entries):
    """CSC arrays (rows ascending) of the upper triangle given as {(i, j): v}, i <= j"""
    cols = [[] for _ in range(n)]
    for (i, j), v in entries.items():
        assert i <= j
        cols[j].append((i, v))
    p, ii, x = [0], [], []
    for j in range(n):
        for i, v in sorted(cols[j]):
            ii.append(i)
            x.append(v)
        p.append(len(ii))
    return n, p, ii, x


def shifted(n, p, i, x, sigma=SIGMA):
    """every stored diagonal entry less sigma"""
    x = np.asarray(x, np.float64).copy()
    cols = np.repeat(np.arange(n), np.diff(p))
    x[np.asarray(i) == cols] -= sigma
    return n, p, i, x


def kkt(nh, nc, seed, g, perm=None):
    """[[H, A'], [A, -g I]]: H tridiagonal and diagonally dominant (diagonal in [4, 5], off-diagonal in [-1, 1]), every
    constraint row three entries of size <= 0.25; under the symmetric permutation perm (new index of old i = perm[i]) or none"""
    rng = np.random.default_rng(seed)
    e = {}
    for j in range(nh):
        e[(j, j)] = float(rng.uniform(4.0, 5.0))
        if j:
            e[(j - 1, j)] = float(rng.uniform(-1.0, 1.0))
    for c in range(nc):
        for r in sorted(rng.choice(nh, 3, replace=False).tolist()):
            e[(r, nh + c)] = float(rng.uniform(-0.25, 0.25))
        e[(nh + c, nh + c)] = -float(g)
    if perm is not None:
        e = {(min(perm[i], perm[j]), max(perm[i], perm[j])): v for (i, j), v in e.items()}
    return upper_csc(nh + nc, e)


KKT_NH, KKT_NC, KKT_SEED, KKT_PERM_SEED = 200, 80, 20240701, 20240702
KKT_PERM = np.random.default_rng(KKT_PERM_SEED).permutation(KKT_NH + KKT_NC).tolist()


def _leaves(blocks, seed):
    rng = np.random.default_rng(seed)
    e = {}
    for b in range(blocks):
        e[(2 * b, 2 * b)] = float(rng.uniform(0.5, 1.5))
        e[(2 * b, 2 * b + 1)] = 2.0
        e[(2 * b + 1, 2 * b + 1)] = float(rng.uniform(0.5, 1.5))
    return upper_csc(2 * blocks, e)


def _chain(n):
    e = {(j, j): 0.5 for j in range(n)}
    e.update({(j - 1, j): -1.0 for j in range(1, n)})
    return upper_csc(n, e)


def _chains(count, length=3):
    """block diagonal: `count` disjoint tridiagonal chains of `length` columns, so every height level has `count` columns"""
    e = {}
    for c in range(count):
        for t in range(length):
            j = c * length + t
            e[(j, j)] = 0.5 + 0.1 * c            # (no pivot of any chain comes out zero)
            if t:
                e[(j - 1, j)] = -1.0
    return upper_csc(count * length, e)


def _arrow(n):
    e = {(j, j): float(n) for j in range(n)}
    e[(0, 0)] = -1.0
    e.update({(0, j): 1.0 for j in range(1, n)})
    return upper_csc(n, e)


STAR_LEAVES = (0, 1, 7, 8, 9, 16, 17)    # updates of a hub's row: none, one, either side of one fetch of eight, and of two
STAR_SEED = 20250917


def _stars(leaves=STAR_LEAVES, seed=STAR_SEED):
    """a forest of stars, every hub numbered after its leaves: the row of a hub with c leaves takes exactly c updates (a leaf's
    column holds its diagonal and the hub's row, there is no fill), a leaf's none.  The diagonal (1 + j / 8) (-1)^j is distinct
    and of both signs, the off-diagonals are uniform in [-1, 1]: 65 columns"""
    rng = np.random.default_rng(seed)
    e, j = {}, 0
    for c in leaves:
        hub = j + c
        for k in range(j, hub + 1):
            e[(k, k)] = (1.0 + k / 8.0) * (-1.0 if k % 2 else 1.0)
            if k < hub:
                e[(k, hub)] = float(rng.uniform(-1.0, 1.0))
        j = hub + 1
    return upper_csc(j, e)


def star_hubs(leaves=STAR_LEAVES):
    """{hub column: its leaves} of _stars"""
    out, j = {}, 0
    for c in leaves:
        out[j + c] = c
        j += c + 1
    return out


def _signed_blocks(nblocks, bs):
    n, p, i, x = arrow_blocks(nblocks, bs)
    x = np.asarray(x, np.float64)
    cols = np.repeat(np.arange(n), np.diff(p))
    x[(cols // bs) % 2 == 1] *= -1.0
    return n, p, i, x


def _build():
    cases = []
    add = cases.append
    add(Case("one", 1, [0, 1], [0], [-3.0], seed=1))
    add(Case("diagonal", 70, np.arange(71), np.arange(70), (1.0 + np.arange(70) / 7.0) * np.where(np.arange(70) % 2, -1.0, 1.0),
             seed=2))
    add(Case("leaves", *_leaves(300, 20240703), seed=3))
    add(Case("chain", *_chain(257), seed=4))
    add(Case("grid24-shift-natural", *shifted(*grid_upper(24)), order=0, seed=5))
    add(Case("grid24-shift", *shifted(*grid_upper(24)), order=1, seed=6))
    add(Case("dups", *shifted(*with_dups_and_lower(24, 14)), order=1, seed=7))
    add(Case("kkt-sqd-natural", *kkt(KKT_NH, KKT_NC, KKT_SEED, 1.0), seed=8))
    add(Case("kkt-sqd", *kkt(KKT_NH, KKT_NC, KKT_SEED, 1.0, KKT_PERM), seed=9))
    add(Case("kkt-zero", *kkt(KKT_NH, KKT_NC, KKT_SEED, 0.0, KKT_PERM), perturb=1e-10, seed=10, breaks=True))
    add(Case("long-column", *_arrow(WINDOW + 1), seed=11))
    add(Case("long-column-updated", *_arrow(WINDOW + 2), seed=12))     # its column 1 is long AND takes an update, in place
    add(Case("sparse-trees", *_signed_blocks(40, 24), seed=13))
    add(Case("chains4", *_chains(4), seed=14))       # three levels of 4 columns: the widest the walker takes
    add(Case("chains5", *_chains(5), seed=15))       # ... of 5: a wave per column
    add(Case("update-batches", *_stars(), seed=16))  # rows of 0, 1, 7, 8, 9, 16, 17 updates: the edges of the fetch of eight
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
SMALL = [c.name for c in CASES if c.n <= 600]
VALUE_SETS = ("A", 0, 1)


# Right-hand sides: BASE columns uniform in [-1, 1] from a committed seed, as rows of the returned array.  The componentwise
# backward error of an unrefined L D L' solve of the quasi-definite KKT case is 3 - 6 eps over such columns (measured with the
# plain-C triangular solves over 300 seeds: the worst of three columns has median 4.8 eps), so "omega <= 4 eps without
# refinement" holds for most columns, not all: the seed is one whose three columns meet it under the reference on both orders
# of the case (tests/test_ldl_cpu.py asserts it; 3.1 - 3.6 eps).  Wider blocks repeat the three columns scaled by powers of two
# (exact: every operation of a solve scales with it, omega does not change), so every column of every block is one the CPU test
# has held to the condition, and a column that lands in the wrong place is still seen.
RHS_SEED, BASE = 20240988, 3


def rhs(case, k=BASE):
    base = np.random.default_rng(RHS_SEED).uniform(-1.0, 1.0, (BASE, case.n))
    return np.stack([base[c % BASE] * 2.0 ** (c // BASE) for c in range(k)])


def random_block(case, k, seed=20240705):
    """n x k independent columns uniform in [-1, 1]: varied data for the wide block paths; held to no bound on omega"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (case.n, k))
