"""Inputs of the sparseinv_ldl / sparseinv_lu tests: factors built straight from patterns with seeded values, one
case on each side of every cut of the launch selection of csx_sparseinv.hip, and a model of that selection written from its
rules.  No ordering and no factorisation stands between a case and the kernels.

A case is a Cholesky pattern (p, i: diagonal first, rows ascending) with
    lx  L's values: 1.0 on the diagonal, |l| <= 1 below it
    ux  Ut's values on the same pattern: the pivot on the diagonal, |u| <= 1 below it
    d   the LDL' pivots (= Ut's diagonal): of both signs, 0.5 <= |d| <= 2
Entries below the diagonal of a column with m rows are uniform in [-1, 1] times min(1, 4 / m): a dense unit triangle with entries
of size 1 has an inverse that grows like 2^m, which at 513 rows overflows; with this scale the growth stays below e^4.

Model: depth[j] = steps to the root over parent[j] = the first row below the diagonal; one launch per depth, roots first; the
longest column of a depth picks the kernel; with the walk on, a run of depths of one column each with at most WIDE_ROWS rows is
one launch of k_si_block."""
import numpy as np

WIDE_ROWS = 128       # SI_WIDE_ROWS
CHUNK = 512           # SI_WIDE_CHUNK


class Case(object):
    def __init__(self, name, cols, seed, expect):
        """cols: for every column its rows (diagonal first, ascending); expect: kernels the model must name for the case"""
        self.name, self.n, self.expect = name, len(cols), set(expect)
        self.p = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)
        self.i = np.concatenate([np.asarray(c, np.int32) for c in cols]).astype(np.int32)
        rng = np.random.default_rng(seed)
        nnz = int(self.p[-1])
        m = np.repeat(np.diff(self.p) - 1, np.diff(self.p))
        scale = np.minimum(1.0, 4.0 / np.maximum(m, 1))
        self.lx = rng.uniform(-1.0, 1.0, nnz) * scale
        self.ux = rng.uniform(-1.0, 1.0, nnz) * scale
        self.d = rng.uniform(0.5, 2.0, self.n) * rng.choice([-1.0, 1.0], self.n)
        self.lx[self.p[:-1]] = 1.0
        self.ux[self.p[:-1]] = self.d

    def dense_l(self):
        return _dense(self.n, self.p, self.i, self.lx)

    def dense_ldl(self):
        L = self.dense_l()
        return L @ np.diag(self.d) @ L.T

    def dense_lu(self):
        return self.dense_l() @ _dense(self.n, self.p, self.i, self.ux).T

    def terms(self):
        m = np.diff(self.p).astype(np.int64) - 1
        return int(np.sum(m * m))


def _dense(n, p, i, x):
    D = np.zeros((n, n))
    D[i, np.repeat(np.arange(n), np.diff(p))] = x
    return D


def clique(first, c):
    return [list(range(first + k, first + c)) for k in range(c)]


def cliques(sizes):
    cols, first = [], 0
    for c in sizes:
        cols += clique(first, c)
        first += c
    return cols


def arrow_tree(first, bs):
    """tridiagonal plus a full last row: column k holds k, k + 1 and the last row -- no clique tail, so the pair
    (k + 1, last) of column k is found in column k + 1 by bisection"""
    return [sorted({first + k, first + min(k + 1, bs - 1), first + bs - 1}) for k in range(bs)]


def chain(n):
    return [[k, k + 1] if k + 1 < n else [k] for k in range(n)]


def model(case, walk=True):
    """(depths, widest, launches): launches = [(kernel, first depth, depths taken)] by the rules of csx_sparseinv.hip"""
    n, p, i = case.n, case.p, case.i
    depth = np.zeros(n, np.int64)
    for j in range(n - 1, -1, -1):
        if p[j + 1] - p[j] > 1:
            depth[j] = depth[i[p[j] + 1]] + 1
    nd = int(depth.max()) + 1 if n else 0
    count = np.bincount(depth, minlength=nd)
    rows = np.zeros(nd, np.int64)
    np.maximum.at(rows, depth, np.diff(p) - 1)
    launches, t = [], 0
    while t < nd:
        u, r = t + 1, int(rows[t])
        if walk and count[t] == 1 and r <= WIDE_ROWS:
            while u < nd and count[u] == 1 and rows[u] <= WIDE_ROWS:
                r = max(r, int(rows[u]))
                u += 1
        if u - t > 1:
            launches.append(("walk<%d>" % (64 if r <= 64 else 256), t, u - t))
        elif r <= 64:
            launches.append(("group<%d>" % (8 if r <= 8 else 16 if r <= 16 else 32 if r <= 32 else 64), t, 1))
        elif r <= WIDE_ROWS:
            launches.append(("block<256>", t, 1))
        else:
            launches.append(("wide/%d" % ((r + CHUNK - 1) // CHUNK), t, 1))
        t = u
    return nd, (int(count.max()) if n else 0), launches


def kernels(case, walk=True):
    return {k for k, _, _ in model(case, walk)[2]}


def _build():
    cases = []
    add = cases.append
    seed = 20241000
    # forests of TWO equal cliques (a depth holds two columns: no walk): c columns = c - 1 rows in the longest column
    for c, expect in ((9, ["group<8>"]), (10, ["group<16>"]), (17, ["group<16>"]), (18, ["group<32>"]), (33, ["group<32>"]),
                      (34, ["group<64>"]), (65, ["group<64>"]), (66, ["block<256>"]), (129, ["block<256>"]),
                      (130, ["wide/1"]), (514, ["wide/2"])):
        seed += 1
        add(Case("cliques2x%d" % c, cliques([c, c]), seed, expect))
    ragged = cliques([c for _ in range(3) for c in range(2, 10)])
    for _ in range(2):                                  # two arrow trees beside them: columns of 1 and 2 rows in the depths of
        ragged += arrow_tree(len(ragged), 9)            # columns of up to 8
    add(Case("ragged", ragged, seed + 1, ["group<8>"]))
    add(Case("clique130", cliques([130]), seed + 2, ["wide/1", "walk<256>"]))
    trees = []
    for _ in range(5):
        trees += arrow_tree(len(trees), 24)
    add(Case("arrow24x5", trees, seed + 3, ["group<8>"]))
    add(Case("chain300", chain(300), seed + 4, ["walk<64>"]))
    add(Case("one", [[0]], seed + 5, ["group<8>"]))
    add(Case("diagonal", [[k] for k in range(70)], seed + 6, ["group<8>"]))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
SMALL = [c.name for c in CASES if c.terms() <= 250000]     # the scalar loops take these in about a second each
WALK_OFF = ["clique130", "chain300"]                      # run with "sparseinv.walk" = 0 as well
