"""Inputs shared by the schur_factor tests: the matrices are those of tests/ldl_cases.py (its builders and its Case:
raw CSC arrays, two congruent value sets A2 = D A D from a committed seed), each with the index set `keep` whose Schur complement
is wanted, the order of the interior (0 ascending, 1 nested dissection) and no perturbation anywhere: kkt-zero, which
ldlsol_factor cannot factor without perturbing pivots, is eliminated here down to its constraints and meets no small pivot.

Two more value sets per case: breaking(j0) zeroes the diagonal of the interior column that is eliminated first (its pivot is that
entry itself: an interior breakdown), kept_zero() zeroes the diagonal entry of keep[0] (data of S: it must factor).

schur_chunks: the (column, chunk) pairs of the trailing-column kernel, from the geometry alone: column t of S (t = 0 .. ns - 1)
spans the ns - t rows t .. ns - 1 and is cut into chunks of WINDOW consecutive rows, so
    chunks(ns) = sum over t of ceil((ns - t) / WINDOW).
ns <= WINDOW: every column is one chunk, ns in all.  ns = WINDOW + 1: column 0 alone spans WINDOW + 1 rows and takes two, ns + 1
in all.  ns = 2 WINDOW + 1: column 0 takes three, columns 1 .. WINDOW two, the WINDOW shorter ones one: 3 WINDOW + 3."""
import numpy as np

import ldl_cases as LC
from chol_refactor_cases import grid_upper, with_dups_and_lower

WINDOW = LC.WINDOW
G = 24
LINE = list(range(12 * G, 13 * G))                                             # grid row 12: two subdomains
CROSS = LINE + [r * G + 12 for r in range(G) if r != 12]                       # ... and grid column 12: four


class SchurCase(object):
    def __init__(self, name, case, keep, order=0):
        self.name, self.case, self.keep, self.order = name, case, [int(v) for v in keep], order
        self.n, self.ns = case.n, len(keep)
        self.n1 = self.n - self.ns

    def values(self, which):
        return self.case.values(which)

    def matrix(self, mod, x=None):
        return self.case.matrix(mod, x)

    def dense(self, x=None):
        return self.case.dense(x)

    def kept_zero(self):
        """A's values with the diagonal entry of keep[0] (every stored copy) set to 0.0"""
        c = self.case
        x = c.x.copy()
        on = (c.cols == self.keep[0]) & (c.i == self.keep[0])
        assert on.any()
        x[on] = 0.0
        return x

    def chunks(self):
        """see the module's docstring"""
        return sum(-(-(self.ns - t) // WINDOW) for t in range(self.ns))


def _border(ns, seed):
    """three interior chain nodes (indices 0, 1, 2), each coupled to every one of ns kept nodes (3 .. ns + 2), which are coupled
    to each other by nothing but a diagonal of both signs: S is a full ns x ns matrix"""
    rng = np.random.default_rng(seed)
    e = {(0, 0): 4.0, (1, 1): -5.0, (2, 2): 6.0, (0, 1): -1.0, (1, 2): -1.0}
    for t in range(ns):
        for k in range(3):
            e[(k, 3 + t)] = float(rng.uniform(-1.0, 1.0))
        e[(3 + t, 3 + t)] = float(rng.uniform(1.0, 2.0)) * (-1.0 if t % 3 == 0 else 1.0)
    return LC.upper_csc(3 + ns, e)


BATCH_ROWS = ((), (9, False), (7, True), (8, True))     # per kept node: (its interior neighbours, coupled to the first kept node)


def _border_batches(seed=20250919):
    """Kept node t has BATCH_ROWS[t][0] interior leaves of its own (a diagonal and the one coupling each: no fill among them)
    and, where the flag says so, an entry with kept node 0.  With the interior ascending and the kept nodes last, the row view
    of a trailing column lists its interior columns and then the kept one, so the update loop's fetches of eight see: no
    descriptor at all; 9 interior ones (a full fetch and one more); 7 interior and the kept one refused INSIDE the fetch; 8
    interior and the kept one refused as the FIRST descriptor of the next fetch, which ends the loop"""
    rng = np.random.default_rng(seed)
    n1 = sum(r[0] for r in BATCH_ROWS if r)
    e, k = {}, 0
    for t, row in enumerate(BATCH_ROWS):
        kept = n1 + t
        e[(kept, kept)] = float(rng.uniform(1.0, 2.0)) * (-1.0 if t % 2 else 1.0)
        if row:
            for _ in range(row[0]):
                e[(k, k)] = float(rng.uniform(1.0, 2.0)) * (-1.0 if k % 3 == 0 else 1.0)
                e[(k, kept)] = float(rng.uniform(-1.0, 1.0))
                k += 1
            if row[1]:
                e[(n1, kept)] = float(rng.uniform(-1.0, 1.0))
    return LC.upper_csc(n1 + len(BATCH_ROWS), e), list(range(n1, n1 + len(BATCH_ROWS)))


def _two():
    return LC.upper_csc(2, {(0, 0): 2.0, (0, 1): 1.0, (1, 1): -3.0})


def _build():
    C = LC.Case
    out = []
    add = out.append
    one = C("one", 1, [0, 1], [0], [-3.0], seed=31)
    add(SchurCase("one-keep-all", one, [0]))                                   # n1 = 0: S = A
    add(SchurCase("one-keep-none", one, []))                                   # ns = 0: the LDL' of A
    add(SchurCase("two", C("two", *_two(), seed=32), [1]))
    grid = C("grid24-shift", *LC.shifted(*grid_upper(G)), seed=33)
    for order in (0, 1):
        add(SchurCase("grid-line-%d" % order, grid, LINE, order))
        add(SchurCase("grid-line-reversed-%d" % order, grid, LINE[::-1], order))
        add(SchurCase("grid-cross-%d" % order, grid, CROSS, order))
    add(SchurCase("dups", C("dups", *LC.shifted(*with_dups_and_lower(G, 14)), seed=34), LINE, 1))
    nh, nc = LC.KKT_NH, LC.KKT_NC
    add(SchurCase("kkt-sqd-natural", C("kkt-sqd-natural", *LC.kkt(nh, nc, LC.KKT_SEED, 1.0), seed=35), range(nh, nh + nc)))
    under = [LC.KKT_PERM[nh + c] for c in range(nc)]                           # the constraint rows under KKT_PERM: unsorted
    add(SchurCase("kkt-sqd", C("kkt-sqd", *LC.kkt(nh, nc, LC.KKT_SEED, 1.0, LC.KKT_PERM), seed=36), under, 1))
    add(SchurCase("kkt-zero", C("kkt-zero", *LC.kkt(nh, nc, LC.KKT_SEED, 0.0, LC.KKT_PERM), seed=37), under, 1))
    add(SchurCase("chain600", C("chain600", *LC._chain(600), seed=38), [598, 599]))         # 598 narrow levels: the walker is cut at 256
    for tag, ns in (("border-window", WINDOW), ("border-window+1", WINDOW + 1), ("border-2window+1", 2 * WINDOW + 1)):
        add(SchurCase(tag, C(tag, *_border(ns, 40 + ns % 7), seed=39), range(3, 3 + ns)))
    batches, kept = _border_batches()
    add(SchurCase("border-batches", C("border-batches", *batches, seed=42), kept))            # refusals at the edges of the fetch of eight
    trees = C("sparse-trees", *LC._signed_blocks(40, 24), seed=41)
    add(SchurCase("sparse-trees", trees, [b * 24 + 23 for b in range(40)], 1))                # the root of every tree: a block-diagonal (here diagonal) S
    return out


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
SMALL = [c.name for c in CASES if c.n <= 600]
BORDERS = ("border-window", "border-window+1", "border-2window+1")
# stated, not computed by the library: see the module's docstring
BORDER_CHUNKS = {"border-window": WINDOW, "border-window+1": WINDOW + 2, "border-2window+1": 3 * WINDOW + 3}
VALUE_SETS = ("A", 0, 1)

X2_SEED = 20250311


def x2(sc, k=1):
    """ns x k interface values uniform in [-1, 1] from a committed seed: an x2 that is not a solve"""
    return np.random.default_rng(X2_SEED).uniform(-1.0, 1.0, (sc.ns, k))


def rhs(sc, k):
    """k right-hand sides as rows (ldl_cases.rhs)"""
    return LC.rhs(sc.case, k)
