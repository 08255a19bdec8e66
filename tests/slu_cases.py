"""Inputs shared by the static-pivot LU tests: for every case the unsymmetric matrix A as raw CSC arrays, the
order, the perturbation, how the diagonal is matched, two new value sets on A's pattern and one that breaks down.

New values are A2 = D1 A D2 with D = diag(1 + 1e-3 u), u uniform in [-1, 1] from a committed seed, applied entry by entry, so of
duplicate entries the last still wins.  The breaking value set has every stored copy of ONE entry set to 0.0: the entry that is
the pivot of the column eliminated first (Case.breaking(i0, j0); tests/slu_oracle.py says which), the matrix otherwise kept.
Where the case runs with a perturbation a zero pivot is perturbed, not a breakdown: the entry is +inf there (so is |A|_1 and with
it the threshold), which no perturbation mends.

The matching of `west` is the product's own (maxtrans_array(A, WEST_SEED), recorded from an MI355X): it runs on the device only,
so the CPU tests take the committed rows and the GPU test asserts that the device still returns them."""
import os

import numpy as np

import _csx
import ldl_cases as LC

SIGMA = 3.7
CONVECTION = 0.3
WINDOW, RUN_LEVELS = _csx.slu_window()   # LDS window in entries and levels per walker launch, asked of the library (no GPU needed)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

WEST_SEED = 3
WEST_PROW = [5, 20, 60, 26, 27, 28, 7, 0, 1, 2, 56, 8, 4, 11, 6, 57, 9, 3, 55, 13, 10, 58, 12, 18, 14, 35, 16, 37, 38, 63,
             15, 24, 25, 17, 59, 19, 32, 29, 21, 22, 61, 34, 23, 45, 46, 65, 33, 53, 41, 30, 31, 62, 42, 43, 40, 39, 50, 51,
             44, 64, 36, 49, 66, 47, 52, 54, 48]


class Case(object):
    def __init__(self, name, n, p, i, x, order=0, perturb=0.0, seed=1, match=None, prow=None, match_seed=0, breaks=False):
        self.name, self.n, self.order, self.perturb = name, int(n), order, perturb
        self.match, self.match_seed = match, match_seed
        self.prow = None if prow is None else np.asarray(prow, np.int32)   # the rows a matching puts on the diagonal, or none
        self.breaks = breaks                   # A itself breaks down at perturb = 0
        self.p = np.asarray(p, np.int32)
        self.i = np.asarray(i, np.int32)
        self.x = np.asarray(x, np.float64)
        self.cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.p))
        self.A2 = [self.scaled(seed * 100 + k) for k in (1, 2)]

    def scaled(self, seed):
        rng = np.random.default_rng(seed)
        d1 = 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, self.n)
        d2 = 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, self.n)
        return d1[self.i] * self.x * d2[self.cols]

    def values(self, which):
        return self.x if which == "A" else self.A2[which]

    def breaking(self, i0, j0):
        bad = self.x.copy()
        on = (self.cols == j0) & (self.i == i0)
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
        """the matrix the factorisation sees: of duplicates the last"""
        x = self.x if x is None else x
        D = np.zeros((self.n, self.n))
        for k in range(len(self.i)):
            D[self.i[k], self.cols[k]] = x[k]
        return D


def csc(n, entries):
    """CSC arrays (rows ascending) of {(i, j): v}"""
    cols = [[] for _ in range(n)]
    for (i, j), v in entries.items():
        cols[j].append((i, v))
    p, ii, x = [0], [], []
    for j in range(n):
        for i, v in sorted(cols[j]):
            ii.append(i)
            x.append(v)
        p.append(len(ii))
    return n, p, ii, x


def grid(g, c=CONVECTION, sigma=0.0, one_sided=False):
    """convection-diffusion on a g x g grid, row by row: 4 - sigma on the diagonal, -1 -+ c to the west / east, -1 north and
    south; one_sided: A(k, k + g) dropped for every fifth k while A(k + g, k) stays"""
    e = {}
    for k in range(g * g):
        e[(k, k)] = 4.0 - sigma
        if k % g:
            e[(k, k - 1)] = -1.0 - c
            e[(k - 1, k)] = -1.0 + c
        if k >= g:
            e[(k, k - g)] = -1.0
            if not (one_sided and (k - g) % 5 == 0):
                e[(k - g, k)] = -1.0
    return csc(g * g, e)


def with_dups(n, p, i, x, seed):
    """every fifth entry split into two (a stray value first, the true one last)"""
    rng = np.random.default_rng(seed)
    p2, i2, x2 = [0], [], []
    for j in range(n):
        for t in range(p[j], p[j + 1]):
            if t % 5 == 0:
                i2.append(i[t])
                x2.append(float(rng.uniform(5.0, 9.0)))
            i2.append(i[t])
            x2.append(x[t])
        p2.append(len(i2))
    return n, p2, i2, x2


def saddle(nh, nc, seed, perm=None):
    """[[H, B1'], [B2, 0]]: H unsymmetric tridiagonal and diagonally dominant (diagonal in [4, 5], off-diagonals in [-1, 1]), B1
    and B2 on one pattern of three entries a constraint with different values of size <= 0.25, the zero block's diagonal stored
    as 0.0; under the symmetric permutation perm (new index of old i = perm[i]) or none"""
    rng = np.random.default_rng(seed)
    e = {}
    for j in range(nh):
        e[(j, j)] = float(rng.uniform(4.0, 5.0))
        if j:
            e[(j - 1, j)] = float(rng.uniform(-1.0, 1.0))
            e[(j, j - 1)] = float(rng.uniform(-1.0, 1.0))
    for c in range(nc):
        for r in sorted(rng.choice(nh, 3, replace=False).tolist()):
            e[(r, nh + c)] = float(rng.uniform(-0.25, 0.25))
            e[(nh + c, r)] = float(rng.uniform(-0.25, 0.25))
        e[(nh + c, nh + c)] = 0.0
    if perm is not None:
        e = {(perm[i], perm[j]): v for (i, j), v in e.items()}
    return csc(nh + nc, e)


SADDLE_NH, SADDLE_NC, SADDLE_SEED, SADDLE_PERM_SEED = 200, 80, 20240801, 20240814
SADDLE_PERM = np.random.default_rng(SADDLE_PERM_SEED).permutation(SADDLE_NH + SADDLE_NC).tolist()


def _blocks(count, seed):
    rng = np.random.default_rng(seed)
    e = {}
    for b in range(count):
        e[(2 * b, 2 * b)] = float(rng.uniform(0.5, 1.5))
        e[(2 * b, 2 * b + 1)] = 2.0
        e[(2 * b + 1, 2 * b)] = float(rng.uniform(-1.5, -0.5))
        e[(2 * b + 1, 2 * b + 1)] = float(rng.uniform(0.5, 1.5))
    return csc(2 * count, e)


def _chain(n):
    e = {(j, j): 0.5 for j in range(n)}
    e.update({(j - 1, j): -1.0 for j in range(1, n)})
    e.update({(j, j - 1): 0.75 for j in range(1, n)})
    return csc(n, e)


def _chains(count, length=3):
    """block diagonal: `count` disjoint unsymmetric tridiagonal chains of `length` columns, so every height level has `count`
    columns"""
    e = {}
    for c in range(count):
        for t in range(length):
            j = c * length + t
            e[(j, j)] = 0.5 + 0.125 * c
            if t:
                e[(j - 1, j)] = -1.0
                e[(j, j - 1)] = 0.75
    return csc(count * length, e)


def _arrow(n):
    e = {(j, j): float(n) for j in range(n)}
    e[(0, 0)] = -1.0
    e.update({(0, j): 1.0 for j in range(1, n)})
    e.update({(j, 0): -0.5 for j in range(1, n)})
    return csc(n, e)


def _stars(seed=20250918):
    """ldl_cases._stars' forest (hub rows of 0, 1, 7, 8, 9, 16 and 17 updates, the same diagonal) with unsymmetric off-diagonals:
    A(leaf, hub) and A(hub, leaf) are independent, uniform in [-1, 1]"""
    rng = np.random.default_rng(seed)
    n, p, i, x = LC._stars()
    e = {}
    for j in range(n):
        for t in range(p[j], p[j + 1]):
            e[(i[t], j)] = x[t]
            if i[t] != j:
                e[(i[t], j)], e[(j, i[t])] = float(rng.uniform(-1.0, 1.0)), float(rng.uniform(-1.0, 1.0))
    return csc(n, e)


def _golden(name, key="A"):
    """the matrix `key` of a fixture: "A" as loaded, "C" with the duplicates of the triplet file summed"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return int(g[key + "_mn"][1]), g[key + "_p"], g[key + "_i"], g[key + "_x"]


def _build():
    cases = []
    add = cases.append
    add(Case("one", 1, [0, 1], [0], [-3.0], seed=1))
    add(Case("diagonal", 70, np.arange(71), np.arange(70), (1.0 + np.arange(70) / 7.0) * np.where(np.arange(70) % 2, -1.0, 1.0),
             seed=2))
    add(Case("blocks", *_blocks(300, 20240803), seed=3))
    add(Case("chain256", *_chain(RUN_LEVELS), seed=4))
    add(Case("chain257", *_chain(RUN_LEVELS + 1), seed=5))
    add(Case("grid24-natural", *grid(24), order=0, seed=6))
    add(Case("grid24", *grid(24), order=1, seed=7))
    add(Case("grid24-shift-natural", *grid(24, sigma=SIGMA), order=0, seed=8))
    add(Case("grid24-shift", *grid(24, sigma=SIGMA), order=1, seed=9))
    add(Case("one-sided", *grid(24, sigma=SIGMA, one_sided=True), order=1, seed=10))
    add(Case("dups", *with_dups(*grid(24, sigma=SIGMA), 14), order=1, seed=11))
    add(Case("west", *_golden("west0067", "C"), order=0, seed=12, match=True, prow=WEST_PROW, match_seed=WEST_SEED))
    add(Case("west-nd", *_golden("west0067", "C"), order=1, seed=18, match=True, prow=WEST_PROW, match_seed=WEST_SEED))
    add(Case("fs183", *_golden("fs_183_1"), order=0, seed=13, match=False))
    add(Case("saddle-natural", *saddle(SADDLE_NH, SADDLE_NC, SADDLE_SEED), seed=14, match=False))
    add(Case("saddle", *saddle(SADDLE_NH, SADDLE_NC, SADDLE_SEED, SADDLE_PERM), perturb=1e-10, seed=15, match=False, breaks=True))
    add(Case("long-column", *_arrow(WINDOW + 1), seed=16))
    add(Case("long-column-updated", *_arrow(WINDOW + 2), seed=17))     # its column 1 is long AND takes an update, in place
    add(Case("chains4", *_chains(4), seed=19))       # three levels of 4 columns: the widest the walker takes
    add(Case("chains5", *_chains(5), seed=20))       # ... of 5: a wave per column
    add(Case("update-batches", *_stars(), seed=21))  # rows of 0, 1, 7, 8, 9, 16, 17 updates: the edges of the fetch of eight
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
VALUE_SETS = ("A", 0, 1)

# Right-hand sides: BASE columns uniform in [-1, 1] from a committed seed, as rows of the returned array; wider blocks repeat them
# scaled by powers of two (exact: every operation of a solve scales with it, omega does not change), so every column of every
# block is one the CPU test has held to its condition, and a column that lands in the wrong place is still seen.
RHS_SEED, BASE = 20240989, 3


def rhs(case, k=BASE):
    base = np.random.default_rng(RHS_SEED).uniform(-1.0, 1.0, (BASE, case.n))
    return np.stack([base[c % BASE] * 2.0 ** (c // BASE) for c in range(k)])


def random_block(case, k, seed=20240805):
    """n x k independent columns uniform in [-1, 1]: varied data for the wide block paths; held to no bound on omega"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (case.n, k))
