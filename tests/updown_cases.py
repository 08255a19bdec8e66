"""Cases for updown_block, each aimed at one stated edge of its schedule: a launch class, the 60 KB LDS
limit of W, the 64 / 65-entry column, the refills of 16 terms, masks of one bit, the chunk cuts, the second trip of the
lanes, and the ways a downdate can fail (tests/test_updown_cases_cpu.py, tests/test_gpu_updown_edges.py).

The factors are built directly, not factored from a matrix: Cholesky-shaped by construction (diagonal first, rows
ascending, the struct of a column inside its path), a seeded diagonal in [2, 3] and small entries below it.  band(n, bw):
column j holds rows j .. min(j + bw, n - 1), so the tree is a chain and a column has bw + 1 entries.  arrow(leaves, sep):
every leaf column holds itself and all sep separator rows, the separators are dense among themselves.  A forest is the
block diagonal of these.

get(name) builds a case once: L (numpy p, i, x), the columns of C, sigma, and `applied` / `ref_x`, the count and the bytes
of L.x the reference loop (updown_block_oracle.loop on csparse_oracle.cs_updown) leaves.  `want` is the count the case is
built for: k for a case that succeeds, the intended term for one that fails.  The columns that are not meant to fail are
scaled down until the loop gives it, and the builder asserts it, so a success case cannot quietly turn into a failure case.
`expect` holds the facts of the schedule the case is named for, stated by hand; the CPU test holds the model
(updown_block_oracle.schedule) to them and the GPU test holds the device's report to the model."""
import functools

import numpy as np

import csparse_oracle as O
import updown_block_oracle as UB


# ---- factors

def band(n, bw, rng):
    cols = []
    for j in range(n):
        rows = list(range(j, min(j + bw, n - 1) + 1))
        vals = [float(rng.uniform(2.0, 3.0))] + [float(v) for v in rng.uniform(-0.05, 0.05, len(rows) - 1)]
        cols.append((rows, vals))
    return cols


def arrow(leaves, sep, rng):
    n = leaves + sep
    cols = []
    for j in range(n):
        rows = [j] + list(range(leaves, n)) if j < leaves else list(range(j, n))
        vals = [float(rng.uniform(2.0, 3.0))] + [float(v) for v in rng.uniform(-0.05, 0.05, len(rows) - 1)]
        cols.append((rows, vals))
    return cols


def forest(blocks):
    """the block diagonal of the blocks -> (p, i, x) as numpy arrays and every block's first column"""
    p, i, x, first = [0], [], [], []
    off = 0
    for cols in blocks:
        first.append(off)
        for rows, vals in cols:
            i += [r + off for r in rows]
            x += vals
            p.append(len(i))
        off += len(cols)
    return (np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64)), first


# ---- terms: (rows, values, sigma, fixed); the values of a term that is not `fixed` are scaled by the builder

def _term(L, f, rng, sigma=None, extra=3):
    """f and up to `extra` rows of L(:, f)'s pattern (rows on f's path), values of magnitude 0.4 .. 1.2 (before scaling)"""
    p, i, _ = L
    pat = i[p[f] + 1:p[f + 1]]
    rows = [int(f)] + sorted(int(r) for r in rng.choice(pat, size=min(len(pat), extra), replace=False))
    vals = [float(v) for v in rng.uniform(0.4, 1.2, len(rows)) * rng.choice([-1.0, 1.0], len(rows))]
    if sigma is None:
        sigma = 1 if rng.uniform() < 0.5 else -1
    return rows, vals, sigma, False


def _bad(L, f, depth):
    """a downdate that passes `depth` columns of f's path and is not positive definite at the next: three times that column's
    diagonal there (alpha is about 3, beta2 about 1 - 9)"""
    p, i, x = L
    j = int(f)
    for _ in range(depth):
        j = int(i[p[j] + 1])
    if depth == 0:
        return [j], [3.0 * float(x[p[j]])], -1, True
    return [int(f), j], [0.05, 3.0 * float(x[p[j]])], -1, True


class Case:
    def __init__(self, name, L, terms, want, expect):
        self.name = name
        self.p, self.i, self.x = L
        self.n = len(self.p) - 1
        self.want = want
        self.expect = expect
        self.k = len(terms)
        self.sigma = [t[2] for t in terms]
        self.fails = want < self.k
        scale = 0.05
        for _ in range(8):
            self.cols = [(list(r), [v if fixed else scale * v for v in vals]) for r, vals, _, fixed in terms]
            Lo = self.oracle_L()
            self.applied = UB.loop(Lo, self.sigma, self.oracle_C(), UB.tree_of(Lo), O)
            if self.applied == want:
                break
            scale *= 0.25
        assert self.applied == want, (name, self.applied, want)
        self.ref_x = np.asarray(Lo.x[:len(self.x)], np.float64).tobytes()      # (bytes: nobody can change them)
        assert not np.isnan(np.frombuffer(self.ref_x)).any()

    def oracle_L(self):
        return csc(O, self.n, self.n, self.p, self.i, self.x)

    def oracle_C(self):
        return columns(O, self.n, self.cols)


def csc(mod, m, n, p, i, x):
    A = mod.cs_spalloc(m, n, max(1, len(i)), True, False)
    A.p, A.i, A.x = [int(v) for v in p], [int(v) for v in i] or [0], [float(v) for v in x] or [0.0]
    return A


def columns(mod, n, cols):
    """the n x len(cols) CSC matrix of module `mod` with the given (rows, values) columns, in the given storage order"""
    p, i, x = [0], [], []
    for r, v in cols:
        i += r
        x += v
        p.append(len(i))
    return csc(mod, n, len(cols), p, i, x)


# ---- the cases

_BUILDERS = {}


def _case(fn):
    _BUILDERS[fn.__name__] = fn
    return fn


def _four(extra=None):
    """four_classes: one tree per launch class, 64 terms each from the block's first column, the term indices interleaved.
    ucnt * nterm = 120 * 64 = 7680 doubles is exactly 60 KB (LDS), 121 * 64 = 7744 is over (global); columns of 64 entries
    take one wave, of 65 take 256 lanes.  extra = c: one failing term more, the 65th of block c (chunk 1 of that tree)."""
    rng = np.random.default_rng(41)
    L, first = forest([band(120, 63, rng), band(120, 64, rng), band(121, 63, rng), band(121, 64, rng)])
    terms = [_term(L, first[t % 4], rng) for t in range(256)]
    if extra is not None:
        terms.append(_bad(L, first[extra], 2))
    return L, terms


@_case
def four_classes():
    L, terms = _four()
    return Case("four_classes", L, terms, 256,
                {"chunks": 1, "groups": [4], "classes": [1, 1, 1, 1], "union_columns": 482,
                 "tree_groups": [[(64, 120, 64, 2), (64, 120, 65, 3), (64, 121, 64, 0), (64, 121, 65, 1)]],
                 "w_doubles": [7680, 7680, 7744, 7744]})


def _fail_in_class(c):
    def build():
        L, terms = _four(c)
        classes = [1, 1, 1, 1]
        classes[(2, 3, 2, 3)[c]] += 1                 # chunk 1: the one term of block c, W in LDS, lanes by the column length
        return Case("fail_in_class%d" % c, L, terms, 256,
                    {"chunks": 2, "groups": [4, 1], "classes": classes, "union_columns": 482 + (120, 120, 121, 121)[c]})
    build.__name__ = "fail_in_class%d" % c
    return _case(build)


def _fail_inside_class(c):
    """four_classes with the last term of block c (rank 63, global term 252 + c) failing: the failure, not only the replay,
    happens in that block's launch (blocks 0 .. 3 run in classes 2, 3, 0, 1)"""
    def build():
        L, terms = _four()
        terms[252 + c] = _bad(L, (0, 120, 240, 361)[c], 2)
        return Case("fail_inside_class%d" % c, L, terms, 252 + c,
                    {"chunks": 1, "groups": [4], "classes": [1, 1, 1, 1], "union_columns": 482})
    build.__name__ = "fail_inside_class%d" % c
    return _case(build)


for _c in range(4):
    _fail_in_class(_c)
    _fail_inside_class(_c)


@_case
def lds_edge_by_terms():
    """the LDS edge again with nterm != 64 (W's row stride is then not 64): 128 columns x 60 terms = 7680, x 61 = 7808"""
    rng = np.random.default_rng(42)
    L, first = forest([band(128, 2, rng), band(128, 2, rng)])
    owner = [t % 2 for t in range(120)] + [1]
    terms = [_term(L, first[b], rng) for b in owner]
    return Case("lds_edge_by_terms", L, terms, 121,
                {"chunks": 1, "groups": [2], "classes": [1, 0, 1, 0], "union_columns": 256,
                 "tree_groups": [[(60, 128, 3, 2), (61, 128, 3, 0)]], "w_doubles": [7680, 7808]})


@_case
def staggered():
    """term t starts at column t of one chain: in chunk 0 column j carries min(j + 1, 64) terms, so every count 1 .. 64
    occurs (the refills at 16 / 17, 32 / 33, 48 / 49); three chunks, 64 + 64 + 2, the first with W in global memory"""
    rng = np.random.default_rng(43)
    L, _ = forest([band(140, 3, rng)])
    terms = [_term(L, t, rng) for t in range(130)]
    return Case("staggered", L, terms, 130,
                {"chunks": 3, "groups": [1, 1, 1], "classes": [1, 0, 2, 0], "union_columns": 140 + 76 + 12,
                 "tree_groups": [[(64, 140, 4, 0)], [(64, 76, 4, 2)], [(2, 12, 4, 2)]]})


@_case
def fail_staggered():
    """staggered with term 100 (chunk 1) failing: the three chunks' unions are different columns of one tree, a column's
    place in the union differs from chunk to chunk, and the replay of chunk 0 needs chunk 0's places again"""
    rng = np.random.default_rng(43)
    L, _ = forest([band(140, 3, rng)])
    terms = [_term(L, t, rng) for t in range(130)]
    terms[100] = _bad(L, 100, 1)
    return Case("fail_staggered", L, terms, 100,
                {"chunks": 3, "groups": [1, 1, 1], "classes": [1, 0, 2, 0], "union_columns": 140 + 76 + 12})


@_case
def sparse_masks():
    """term b starts at leaf b of an arrow: the leaves' masks are single bits (bit 0 and bit 63 among them), the separators'
    are all ones; a second chunk of 7 terms on leaves 0, 9 and 63"""
    rng = np.random.default_rng(44)
    L, _ = forest([arrow(64, 5, rng)])
    terms = [_term(L, b, rng) for b in range(64)] + [_term(L, f, rng) for f in (0, 9, 63, 0, 9, 63, 0)]
    return Case("sparse_masks", L, terms, 71,
                {"chunks": 2, "groups": [1, 1], "classes": [0, 0, 2, 0], "union_columns": 69 + 8,
                 "tree_groups": [[(64, 69, 6, 2)], [(7, 8, 6, 2)]]})


@_case
def block_trips():
    """256 and 257 entries below a diagonal: one and two trips of the 256 lanes; and the 65- and 64-entry columns"""
    rng = np.random.default_rng(45)
    L, first = forest([band(300, 256, rng), band(300, 257, rng), band(70, 64, rng), band(70, 63, rng)])
    terms = [_term(L, first[t % 4], rng) for t in range(12)]
    return Case("block_trips", L, terms, 12,
                {"chunks": 1, "groups": [4], "classes": [0, 0, 1, 3], "union_columns": 740,
                 "tree_groups": [[(3, 300, 257, 3), (3, 300, 258, 3), (3, 70, 65, 3), (3, 70, 64, 2)]]})


def _interleave(counts):
    """tree labels, round robin while a tree has terms left: the terms of every tree spread over the whole index range"""
    left, out = list(counts), []
    while any(left):
        for g in range(len(left)):
            if left[g]:
                left[g] -= 1
                out.append(g)
    return out


@_case
def chunks_uneven():
    """trees with 129, 64 and 1 terms: 3, 1 and 1 groups in the three chunks"""
    rng = np.random.default_rng(46)
    L, first = forest([band(20, 2, rng), band(20, 2, rng), band(20, 2, rng)])
    terms = [_term(L, first[g] + int(rng.integers(0, 4)), rng) for g in _interleave([129, 64, 1])]
    return Case("chunks_uneven", L, terms, 194, {"chunks": 3, "groups": [3, 1, 1]})


@_case
def dense_1030():
    """a dense lower triangle of order 1030, an update and a downdate from column 0: the rank-1 kernel's second trip of
    1024 lanes, the block kernel's fifth of 256"""
    rng = np.random.default_rng(47)
    L, _ = forest([band(1030, 1029, rng)])
    terms = [_term(L, 0, rng, sigma=1, extra=40), _term(L, 0, rng, sigma=-1, extra=40)]
    return Case("dense_1030", L, terms, 2,
                {"chunks": 1, "groups": [1], "classes": [0, 0, 0, 1], "union_columns": 1030,
                 "tree_groups": [[(2, 1030, 1030, 3)]]})


def _zero_beta2(L, f):
    """sigma = -1 and C(:,t) = L(f,f) e_f on an L(f,f) no earlier term touches: alpha = 1 and beta2 = 1 - 1 = 0.0 exactly"""
    p, _, x = L
    return [int(f)], [float(x[p[f]])], -1, True


@_case
def zero_beta2_only():
    rng = np.random.default_rng(48)
    L, _ = forest([band(6, 2, rng)])
    return Case("zero_beta2_only", L, [_zero_beta2(L, 0)], 0, {"chunks": 1, "groups": [1], "classes": [0, 0, 1, 0]})


@_case
def zero_beta2_mid():
    """term 5 of 9 on one chain; the others start above column 0 and leave L(0,0) as it was"""
    rng = np.random.default_rng(49)
    L, _ = forest([band(12, 2, rng)])
    terms = [_term(L, 1 + t % 4, rng) for t in range(9)]
    terms[5] = _zero_beta2(L, 0)
    return Case("zero_beta2_mid", L, terms, 5, {"chunks": 1, "groups": [1], "classes": [0, 0, 1, 0]})


@_case
def fail_upstream():
    """term 3 passes two columns and fails at its third: its writes to the first two are part of the loop's state"""
    rng = np.random.default_rng(50)
    L, _ = forest([band(10, 3, rng)])
    terms = [_term(L, t % 3, rng) for t in range(6)]
    terms[3] = _bad(L, 1, 2)
    return Case("fail_upstream", L, terms, 3, {"chunks": 1, "groups": [1]})


@_case
def fail_first_upstream():
    """term 0 itself fails, two columns up: nothing is applied in full and yet L is not as it was"""
    rng = np.random.default_rng(61)
    L, _ = forest([band(10, 3, rng)])
    terms = [_bad(L, 0, 2)] + [_term(L, t % 3, rng) for t in range(3)]
    return Case("fail_first_upstream", L, terms, 0, {"chunks": 1, "groups": [1]})


@_case
def fail_in_chunk1_shared():
    """one chain, 100 terms through the same columns, term 80 fails: chunks 0 and 1 snapshot the same columns, chunk 1's
    after chunk 0 ran, so only last-chunk-first puts the first values back"""
    rng = np.random.default_rng(51)
    L, _ = forest([band(30, 3, rng)])
    terms = [_term(L, t % 3, rng) for t in range(100)]
    terms[80] = _bad(L, 0, 1)
    return Case("fail_in_chunk1_shared", L, terms, 80, {"chunks": 2, "groups": [1, 1]})


@_case
def fail_chunk0_skips_chunk1():
    """tree A (100 terms) fails at its rank-10 term, global term 20; tree B (70 terms, none failing) has terms on both sides
    of it.  A's chunk 1 comes after the failure; B's terms above 20 run in the first pass and not in the replay."""
    rng = np.random.default_rng(52)
    L, first = forest([band(16, 2, rng), band(16, 2, rng)])
    owner = _interleave([100, 70])
    assert owner[20] == 0 and owner[:20].count(0) == 10
    terms = [_term(L, first[g] + int(rng.integers(0, 3)), rng) for g in owner]
    terms[20] = _bad(L, first[0], 1)
    return Case("fail_chunk0_skips_chunk1", L, terms, 20, {"chunks": 2, "groups": [2, 2]})


@_case
def two_trees_fail():
    """tree A fails at global term 40, tree B at 25: 25 applied, A's terms below 25 in full, A's term 40 not at all"""
    rng = np.random.default_rng(53)
    L, first = forest([band(16, 2, rng), band(16, 2, rng)])
    owner = _interleave([30, 30])
    assert owner[40] == 0 and owner[25] == 1
    terms = [_term(L, first[g] + int(rng.integers(0, 3)), rng) for g in owner]
    terms[40] = _bad(L, first[0], 1)
    terms[25] = _bad(L, first[1] + 1, 2)
    return Case("two_trees_fail", L, terms, 25, {"chunks": 1, "groups": [2]})


def _fail_at_rank(name, bad):
    def build():
        rng = np.random.default_rng(54)
        L, _ = forest([band(20, 3, rng)])
        terms = [_term(L, t % 4, rng) for t in range(70)]
        terms[bad] = _bad(L, 1, 1)
        return Case(name, L, terms, bad, {"chunks": 2, "groups": [1, 1]})
    build.__name__ = name
    return _case(build)


_fail_at_rank("fail_bit63", 63)       # the last term of a full chunk: the terms below it are (1ull << 63) - 1
_fail_at_rank("fail_bit0_chunk1", 64)  # the first term of chunk 1: no term of that chunk goes on


@_case
def dup_rows():
    """a row given twice: the later value wins, also at f itself"""
    rng = np.random.default_rng(55)
    L, _ = forest([band(10, 3, rng)])
    terms = []
    for t in range(4):
        rows, vals, sigma, _ = _term(L, t % 2, rng)
        rows = rows + [rows[1], rows[0], rows[1]]
        vals = vals + [0.9, -0.7, 0.3]
        terms.append((rows, vals, sigma, False))
    return Case("dup_rows", L, terms, 4, {"chunks": 1, "groups": [1]})


@_case
def off_path():
    """rows off the path of f: another leaf of the same arrow (a union column of the tree through term 1, but not on term
    0's path), and a row of another tree; assigned and never read"""
    rng = np.random.default_rng(56)
    L, first = forest([arrow(4, 2, rng), band(5, 1, rng)])
    r0, v0, s0, _ = _term(L, 0, rng)
    terms = [(r0 + [2, first[1] + 3], v0 + [7.0, -5.0], s0, False), _term(L, 2, rng), _term(L, first[1], rng)]
    return Case("off_path", L, terms, 3, {"chunks": 1, "groups": [2]})


@_case
def empty_between():
    rng = np.random.default_rng(57)
    L, first = forest([band(8, 2, rng), band(8, 2, rng)])
    terms = []
    for t in range(9):
        terms.append(([], [], 1 if t % 2 else -1, False) if t % 3 == 1 else _term(L, first[t % 2] + t % 3, rng))
    return Case("empty_between", L, terms, 9, {"chunks": 1, "groups": [2]})


@_case
def all_empty():
    rng = np.random.default_rng(58)
    L, _ = forest([band(8, 2, rng)])
    return Case("all_empty", L, [([], [], 1, False), ([], [], -1, False), ([], [], 1, False)], 3,
                {"chunks": 0, "groups": [], "classes": [0, 0, 0, 0], "union_columns": 0})


@_case
def isolated_root():
    """f at a root whose column is its diagonal only, between two other trees"""
    rng = np.random.default_rng(59)
    L, first = forest([band(5, 2, rng), band(1, 0, rng), band(4, 1, rng)])
    terms = [_term(L, first[0], rng), ([first[1]], [1.0], 1, False), _term(L, first[2], rng), ([first[1]], [0.8], -1, False)]
    return Case("isolated_root", L, terms, 4, {"chunks": 1, "groups": [3], "union_columns": 5 + 1 + 4})


@_case
def n1():
    rng = np.random.default_rng(60)
    L, _ = forest([band(1, 0, rng)])
    return Case("n1", L, [([0], [1.0], 1, False), ([0], [0.7], -1, False)], 2,
                {"chunks": 1, "groups": [1], "classes": [0, 0, 1, 0], "union_columns": 1})


NAMES = sorted(_BUILDERS)


@functools.lru_cache(maxsize=None)
def get(name):
    return _BUILDERS[name]()


FAILING = [n for n in NAMES if n.startswith(("fail_", "zero_beta2", "two_trees"))]
