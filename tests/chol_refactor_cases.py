"""Inputs shared by the Cholesky-refactor tests: for every case the matrix A (raw CSC arrays: the upper triangle,
in some cases lower entries and duplicate entries too), a list of new value sets A2 on A's pattern, a value set that is not
positive definite, the order, the kernel-selection options the case runs under and the route it is built for.

New values are A2 = D A D + s diag(A) with D = diag(1 + 1e-3 u), u uniform in [-1, 1], s = 1e-3: the congruence of an SPD
matrix plus a non-negative diagonal is SPD whatever A's condition number (an entrywise perturbation is not safe on
bcsstk01).  The formula is applied entry by entry, so of duplicate entries the last still wins with the transformed value and
lower entries stay what they are: ignored.  The value set that is not SPD is A with the diagonal of column n // 2 negated."""
import numpy as np

import synth
from conftest import golden

S_SHIFT = 1e-3


class Case(object):
    def __init__(self, name, n, p, i, x, order=0, options=(), exact=None, expect=None, seed=1, same_bytes=True):
        self.name, self.n, self.order, self.exact = name, int(n), order, exact
        self.same_bytes = same_bytes           # False: the refactor's L.x equals a fresh factor's to rounding only (see below)
        self.p = np.asarray(p, np.int32)
        self.i = np.asarray(i, np.int32)
        self.x = np.asarray(x, np.float64)
        self.options = tuple(options)          # ((name, value), ...) in force for the factor and every refactor
        self.expect = dict(expect or {})       # refactor_info() fields: a value, or ">=1"
        self.cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.p))
        self.A2 = [self.congruent(seed * 100 + k) for k in (1, 2)]
        bad = self.x.copy()
        on_diag = (self.cols == self.n // 2) & (self.i == self.n // 2)
        assert on_diag.any()
        bad[on_diag] = -bad[on_diag]
        self.bad = bad

    def congruent(self, seed):
        d = 1.0 + 1e-3 * np.random.default_rng(seed).uniform(-1.0, 1.0, self.n)
        x2 = d[self.i] * self.x * d[self.cols]
        diag = self.i == self.cols
        x2[diag] += S_SHIFT * self.x[diag]
        return x2

    def matrix(self, mod, x=None):
        """a `cs` of module mod (the product or the oracle) with A's pattern and the values x (default A's own)"""
        x = self.x if x is None else x
        A = mod.cs_spalloc(self.n, self.n, max(len(self.i), 1), True, False)
        A.p, A.i, A.x = self.p.tolist(), (self.i.tolist() or [0]), (np.asarray(x, np.float64).tolist() or [0.0])
        return A

    def effective_upper(self, x=None):
        """dense upper triangle as cs_chol reads it: entries with row <= column, of duplicates the last"""
        x = self.x if x is None else x
        U = np.zeros((self.n, self.n))
        for k in range(len(self.i)):
            if self.i[k] <= self.cols[k]:
                U[self.i[k], self.cols[k]] = x[k]
        return U


def grid_upper(g):
    """upper triangle of the five-point Laplacian on a g x g grid, natural (row by row) numbering, rows ascending"""
    n = g * g
    p, i, x = [0], [], []
    for j in range(n):
        if j >= g:
            i.append(j - g)
            x.append(-1.0)
        if j % g:
            i.append(j - 1)
            x.append(-1.0)
        i.append(j)
        x.append(4.0)
        p.append(len(i))
    return n, p, i, x


def with_dups_and_lower(g, seed):
    """grid_upper(g) with every fifth upper entry split into two entries (a stray value first, the true one last) and the strict
    lower triangle present with other values"""
    n, p, i, x = grid_upper(g)
    rng = np.random.default_rng(seed)
    p2, i2, x2 = [0], [], []
    k = 0
    for j in range(n):
        for t in range(p[j], p[j + 1]):
            if k % 5 == 0:
                i2.append(i[t])
                x2.append(float(rng.uniform(5.0, 9.0)))
            i2.append(i[t])
            x2.append(x[t])
            k += 1
        for r in (j + 1, j + g):            # the mirror entries, with values that would break the factor if they were read
            if r < n and (r != j + 1 or r % g):
                i2.append(r)
                x2.append(float(rng.uniform(20.0, 30.0)))
        p2.append(len(i2))
    return n, p2, i2, x2


def arrow_blocks(nblocks, bs):
    """block diagonal, every block tridiagonal plus a full last column: a forest of small SPARSE trees on consecutive columns"""
    p, i, x = [0], [], []
    for b in range(nblocks):
        c0 = b * bs
        for a in range(bs):
            j = c0 + a
            if a == bs - 1:
                for r in range(bs - 2):
                    i.append(c0 + r)
                    x.append(0.5)
            if a > 0:
                i.append(j - 1)
                x.append(-1.0)
            i.append(j)
            x.append(4.0 if a < bs - 1 else float(bs + 6))
            p.append(len(i))
    return nblocks * bs, p, i, x


def _golden_C(name):
    g = golden(name)
    n = int(g["C_mn"][1])
    p = g["C_p"].astype(np.int64)
    return n, p, g["C_i"][:p[n]], g["C_x"][:p[n]]


def _build():
    cases = []
    add = cases.append
    add(Case("bcsstk01-natural", *_golden_C("bcsstk01"), order=0, seed=1))
    add(Case("bcsstk01-ordered", *_golden_C("bcsstk01"), order=1, expect={"route": "general"}, seed=2))
    g22, g24 = grid_upper(22), grid_upper(24)
    add(Case("grid22", *g22, order=1, expect={"route": "general", "trees": ">=1", "band": 0}, seed=3))
    add(Case("grid22-no-dense-trees", *g22, order=1, options=(("chol.dense_trees", 0),),
             expect={"route": "general", "trees": ">=1", "dense_trees": 0}, seed=4))
    add(Case("grid24", *g24, order=1, expect={"route": "general", "levels": ">=1", "supernodes": ">=1", "band": 0}, seed=5))
    add(Case("grid24-no-supernodes", *g24, order=1, options=(("chol.supernodes", 0),),
             expect={"route": "general", "levels": ">=1", "supernodes": 0, "band": 0}, seed=6))
    add(Case("grid24nat", *g24, order=0, expect={"route": "general", "band": 1, "levels": 0}, seed=7))
    add(Case("grid24nat-wide-band", *g24, order=0, options=(("chol.wband", 2),), expect={"route": "general", "band": 2}, seed=8))
    add(Case("grid24nat-coop", *g24, order=0, options=(("chol.band", 0),),
             expect={"route": "general", "band": 0, "levels": ">=1"}, seed=9))
    c16 = synth.gspd(8, 16, 20240611)
    for exact in (True, False):
        add(Case("cliques16-exact" if exact else "cliques16-rounding", 128, *c16, order=0, exact=exact,
                 expect={"route": "forest"}, seed=10))
    add(Case("cliques16-general", 128, *c16, order=0, options=(("chol.clique", 0),), expect={"route": "general"}, seed=11))
    rn, rp, ri, rx, _ = synth.ragged_cliques(300, 8, 64, 20240612)
    add(Case("ragged", rn, rp, ri, rx, order=0, expect={"route": "forest"}, seed=12))
    # "chol.exact" = 0 (the opt-in rounding-equal block arithmetic).  A solver made with exact=True factors without an emission:
    # fresh factor and refactor run the same kernel, the bytes agree.  With exact=None / False the fresh factor's block kernel also
    # emits the matrix-core solve's operands -- for unequal cliques that is another kernel (the blocked factorisation per size
    # class) than the refactor's, so L.x agrees to rounding, which is all "chol.exact" = 0 promises of L.x anyway.
    relaxed = (("chol.exact", 0),)
    add(Case("cliques16-relaxed", 128, *c16, order=0, exact=True, options=relaxed, expect={"route": "forest"}, seed=17))
    add(Case("ragged-relaxed", rn, rp, ri, rx, order=0, exact=True, options=relaxed, expect={"route": "forest"}, seed=18))
    add(Case("cliques16-relaxed-emitted", 128, *c16, order=0, exact=False, options=relaxed, expect={"route": "forest"}, seed=19,
             same_bytes=False))
    add(Case("ragged-relaxed-emitted", rn, rp, ri, rx, order=0, exact=None, options=relaxed, expect={"route": "forest"}, seed=20,
             same_bytes=False))
    add(Case("sparse_trees", *arrow_blocks(40, 24), order=0, expect={"route": "forest"}, seed=13))
    add(Case("dups", *with_dups_and_lower(24, 14), order=1, expect={"route": "general", "levels": ">=1"}, seed=14))
    add(Case("one", 1, [0, 1], [0], [3.0], order=0, seed=15))
    add(Case("diagonal", 70, np.arange(71), np.arange(70), 1.0 + np.arange(70) / 7.0, order=0, seed=16))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]


def oracle_symbolic(O, case, pinv):
    """the oracle's S for P A P' (pinv a list, or None: natural order)"""
    A = case.matrix(O)
    S = O.cs_schol(0, A if pinv is None else O.cs_symperm(A, pinv, False))
    S.pinv = pinv
    return S


_ORACLE = {}


def oracle_factor(O, case, which, S):
    """O.cs_chol of the case's value set `which` (0, 1: A2s; "A": A's own; "bad") under S, computed once: (p, i, x) or None"""
    key = (case.name, which, None if S.pinv is None else tuple(S.pinv))
    if key not in _ORACLE:
        x = case.x if which == "A" else case.bad if which == "bad" else case.A2[which]
        N = O.cs_chol(case.matrix(O, x), S)
        if N is None:
            _ORACLE[key] = None
        else:
            nnz = N.L.p[case.n]
            _ORACLE[key] = (np.asarray(N.L.p, np.int64), np.asarray(N.L.i[:nnz], np.int64), np.asarray(N.L.x[:nnz], np.float64))
    return _ORACLE[key]
