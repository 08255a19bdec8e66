"""The cases of csx_pattern_outer and csx_assemble_pullback, one per edge, cut by the library's own constants
(_csx.pattern_outer_limits()): shared by tests/test_outer_cases_cpu.py (host rule against the restatement of
tests/outer_oracle.py) and tests/test_gpu_pattern_outer.py (device against the host rule).

W is the most partial sums of an entry (PO_LANES), E the entries a workgroup takes (PO_CHUNK), EW the entries one of its waves
takes (PO_WAVE_CHUNK), F the consecutive entries a lane group keeps in flight (PO_FLIGHT), KEPT the passes of W columns of a
column's own rows that stay in registers while a step's entries share the column (PO_KEPT).  Data: full-mantissa doubles of mixed sign with
exponents spread over 2^-20 .. 2^20, so that the order of a sum shows in its bits."""
import numpy as np

import _csx

LIMITS = _csx.pattern_outer_limits()
W, E, EW, F = LIMITS["PO_LANES"], LIMITS["PO_CHUNK"], LIMITS["PO_WAVE_CHUNK"], LIMITS["PO_FLIGHT"]
KEPT = LIMITS["PO_KEPT"]

NRHS = (1, 2, 3, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 130)
COLUMN_LENGTHS = (E - 1, E, E + 1, 4 * E + 1, EW - 1, EW, EW + 1)
# the register passes of a column's own rows: 1, 2, 4, ... KEPT passes of W columns, and one column past the last
KEPT_NRHS = tuple(sorted({W + 1, 2 * W, 2 * W + 1, 4 * W, 4 * W + 1, KEPT * W - 1, KEPT * W, KEPT * W + 1}))


def block(rows, k, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((rows, k)) * 2.0 ** rng.integers(-20, 21, (rows, k))


class Case(object):
    def __init__(self, name, m, n, p, i, nrhs, kind, special=None, values=None):
        self.name, self.m, self.n, self.nrhs, self.kind = name, int(m), int(n), int(nrhs), kind
        self.p, self.i = np.asarray(p, np.int32), np.asarray(i, np.int32)
        self.nnz = int(self.p[-1])
        self.special = special          # None, or (which block, row, value): one row of U or V holds a NaN / an inf
        self.values = values            # None (pattern only) or nnz values that no result may depend on
        assert len(self.p) == self.n + 1 and len(self.i) == self.nnz

    @property
    def square(self):
        return self.m == self.n

    def column_lengths(self):
        return np.diff(self.p)

    def data(self, clean=False):
        """(U, V): m x nrhs and n x nrhs; clean: without the special value"""
        seed = sum(ord(c) for c in self.name)
        U, V = block(self.m, self.nrhs, 2 * seed + 1), block(self.n, self.nrhs, 2 * seed + 2)
        if self.special is not None and not clean:
            which, row, value = self.special
            (U if which == "U" else V)[row, self.nrhs // 2] = value
        return U, V

    def touched(self, sym):
        """the entries whose rows hold the special value"""
        which, row, _ = self.special
        col = np.repeat(np.arange(self.n), self.column_lengths())
        if sym:
            return ((self.i == row) | (col == row)) & (self.i <= col)
        return self.i == row if which == "U" else col == row


def _random(m, n, seed, per_col=5):
    """unsorted columns with duplicates inside a column, empty columns and empty rows"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 2 * per_col, n)
    counts[rng.choice(n, max(n // 8, 1), replace=False)] = 0
    live = rng.choice(m, max(1, (4 * m) // 5), replace=False)
    return np.concatenate([[0], np.cumsum(counts)]), rng.choice(live, int(counts.sum()))


def _from_coo(n, r, c):
    """CSC pattern of the pairs (r, c), ascending rows inside a column"""
    order = np.lexsort((r, c))
    return np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]), np.asarray(r)[order]


def _one_column(cnt, seed):
    """one column of cnt entries over cnt + 3 rows, in random order, rows 0 and m - 1 among them"""
    rng = np.random.default_rng(seed)
    m = cnt + 3
    rows = rng.permutation(np.concatenate([[0, m - 1], 1 + rng.choice(m - 2, cnt - 2, replace=False)])) if cnt >= 2 else [0]
    return m, [0, cnt], rows


def _sym_upper(n, seed):
    """(r, c) of a strict upper triangle with about four entries per column, and the diagonal"""
    rng = np.random.default_rng(seed)
    r, c = [], []
    for j in range(1, n):
        for i in rng.choice(j, min(j, 4), replace=False):
            r.append(int(i))
            c.append(j)
    return np.array(r), np.array(c), np.arange(n)


def _build():
    cases = []

    def add(*a, **k):
        cases.append(Case(*a, **k))

    p, i = _random(31, 31, 11)
    for k in NRHS:
        add("nrhs%d" % k, 31, 31, p, i, k, "nrhs")
    add("0x0", 0, 0, [0], [], 3, "shape")
    add("m0", 0, 4, [0] * 5, [], 3, "shape")
    add("n0", 4, 0, [0], [], 3, "shape")
    add("nnz0_n5", 5, 5, [0] * 6, [], 3, "shape")
    add("1x1", 1, 1, [0, 1], [0], 3, "shape")
    for cnt in COLUMN_LENGTHS:
        m, p, i = _one_column(cnt, cnt)
        add("column%d" % cnt, m, 1, p, i, 3, "column")
    rng = np.random.default_rng(5)
    add("columns_of_one", 50, 3 * E, np.arange(3 * E + 1), rng.integers(0, 50, 3 * E), 2, "columns_of_one")
    p, i = _random(30, 40, 12)
    counts = np.diff(p)
    counts[1::2] = 0
    add("every_other_empty", 30, 40, np.concatenate([[0], np.cumsum(counts)]), rng.integers(0, 30, int(counts.sum())), 5, "empty")
    counts = rng.integers(1, 9, 20)
    counts[0] = counts[-1] = 0
    add("first_last_empty", 20, 20, np.concatenate([[0], np.cumsum(counts)]), rng.integers(0, 20, int(counts.sum())), 5, "empty")
    p, i = _random(5, 300, 13, per_col=3)
    add("5x300", 5, 300, p, i, 7, "heights")
    p, i = _random(300, 5, 14, per_col=60)
    add("300x5", 300, 5, p, i, 7, "heights")
    add("rows_0_and_last", 70, 6, [0, 2, 4, 6, 8, 10, 12], [0, 69] * 6, 4, "rows")
    add("duplicates_unsorted", 9, 3, [0, 2, 10, 11], [4, 4, 8, 2, 8, 0, 2, 2, 8, 5, 1], 6, "duplicates")
    # columns longer than a step (the column's rows stay in registers) and shorter, of lengths that are no multiple of the step,
    # at every number of kept passes and one column past the last; square, so that the mirrored rows are kept too
    lens = [0, 70, 1, F, F + 1, 2, 4 * W * F + 3, 0, 3, F - 1, 37]
    n = 4 * W * F + 10
    rng = np.random.default_rng(6)
    p = np.concatenate([[0], np.cumsum(lens + [0] * (n - len(lens)))])
    i = np.concatenate([rng.choice(n, ln, replace=False) for ln in lens])
    for k in KEPT_NRHS:
        add("kept%d" % k, n, n, p, i, k, "kept")
    # symmetric storages: three of them share one upper triangle
    n = 40
    r, c, d = _sym_upper(n, 15)
    p, i = _from_coo(n, np.concatenate([r, d]), np.concatenate([c, d]))
    add("sym_upper", n, n, p, i, 5, "sym")
    p, i = _from_coo(n, np.concatenate([r, d, c]), np.concatenate([c, d, r]))
    add("sym_full", n, n, p, i, 5, "sym")
    add("sym_full_other_below", n, n, p, i, 5, "sym", values=block(len(i), 1, 16).ravel())
    add("sym_diagonal", n, n, np.arange(n + 1), d, 5, "sym")
    p, i = _from_coo(n, c, r)
    add("sym_strictly_lower", n, n, p, i, 5, "sym")
    p, i = _random(33, 33, 17)
    add("nan_in_U", 33, 33, p, i, W + 3, "special", special=("U", int(i[len(i) // 2]), np.nan))
    add("inf_in_V", 33, 33, p, i, W + 3, "special", special=("V", int(np.argmax(np.diff(p))), np.inf))
    return cases


CASES = _build()
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
SYM_SHARED = ("sym_upper", "sym_full", "sym_full_other_below")


def modes(case):
    """the modes a case runs in: general always, sym when the matrix is square"""
    return (False, True) if case.square else (False,)


def upper_slots(case):
    """{(i, j): slot} of the entries on or above the diagonal (the storages of SYM_SHARED hold each once)"""
    col = np.repeat(np.arange(case.n), case.column_lengths())
    return {(int(i), int(j)): q for q, (i, j) in enumerate(zip(case.i, col)) if i <= j}


class Plan(object):
    """an assembly plan's host arrays for the pull-back: the triplets (Ti, Tj) of an m x n matrix through
    csx_assemble_plan_host"""

    def __init__(self, name, m, n, Ti, Tj):
        self.name, self.m, self.n = name, m, n
        self.Ti, self.Tj = np.asarray(Ti, np.int32), np.asarray(Tj, np.int32)
        nz = self.nz = len(self.Ti)
        Cp, Ci = np.zeros(n + 1, np.int32), np.zeros(max(nz, 1), np.int32)
        sp, src = np.zeros(nz + 1, np.int32), np.zeros(max(nz, 1), np.int32)
        nnz = _csx.C.c_int32(0)
        _csx.check(_csx.load().csx_assemble_plan_host(m, n, nz, _csx.pi(self.Ti), _csx.pi(self.Tj), _csx.pi(Cp), _csx.pi(Ci),
                                                      _csx.pi(sp), _csx.pi(src), _csx.C.byref(nnz)), "csx_assemble_plan_host")
        self.nnz = nnz.value
        self.sp, self.src = sp[:self.nnz + 1], src[:nz]
        self.g = block(max(self.nnz, 1), 1, 18).ravel()[:self.nnz]


def _plans():
    rng = np.random.default_rng(19)
    perm = rng.permutation(12 * 9)[:60]
    dup_i = np.concatenate([rng.integers(0, 12, 40), np.full(70, 7), rng.integers(0, 12, 40)])
    dup_j = np.concatenate([rng.integers(0, 9, 40), np.full(70, 3), rng.integers(0, 9, 40)])
    shuffle = rng.permutation(len(dup_i))
    return [Plan("no_duplicates", 12, 9, perm // 9, perm % 9), Plan("dup70", 12, 9, dup_i[shuffle], dup_j[shuffle]),
            Plan("nz0", 4, 3, [], [])]


PLANS = _plans()


# ---- the exact fixtures of solve_grad: dyadic rationals, so that every operation of a factorisation in natural order, of its
# solves and of the outer product is exact, and the float64 gradient must EQUAL the rational one (tests/test_outer_cases_cpu.py
# proves it on the host rules, tests/test_gpu_solve_grad.py asserts it of the six solvers) -------------------------------------

from fractions import Fraction  # noqa: E402

EXACT_N, EXACT_K = 12, 3


def _band(seed, diagonal):
    """a dense EXACT_N x EXACT_N lower triangular band of integers: the diagonal drawn from `diagonal`, three subdiagonals from
    {-1, 0, 1}, the first of them without zeros (one connected piece)"""
    rng = np.random.default_rng(seed)
    n = EXACT_N
    L = np.zeros((n, n))
    L[np.arange(n), np.arange(n)] = rng.choice(diagonal, n)
    for d in (1, 2, 3):
        L[np.arange(d, n), np.arange(n - d)] = rng.choice([-1, 1] if d == 1 else [-1, 0, 1], n - d)
    return L


class Exact(object):
    """name; dense (the matrix as floats that hold integers); sym; (p, i, x): its stored entries, zeros left out, the whole
    matrix also when it is symmetric (the solvers read the upper triangle); B, GX: EXACT_N x EXACT_K integers in -3 .. 3"""

    def __init__(self, name, dense, sym, seed):
        self.name, self.dense, self.sym, self.n = name, dense, sym, EXACT_N
        r, c = np.nonzero(dense.T)            # by column, ascending rows
        self.i, cols = c.astype(np.int32), r
        self.p = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=self.n))]).astype(np.int32)
        self.x = dense[self.i, cols].astype(np.float64)
        self.cols = cols
        rng = np.random.default_rng(seed)
        self.B = rng.integers(-3, 4, (self.n, EXACT_K)).astype(np.float64)
        self.GX = rng.integers(-3, 4, (self.n, EXACT_K)).astype(np.float64)

    def matrix(self, mod):
        A = mod.cs_spalloc(self.n, self.n, len(self.i), True, False)
        A.p, A.i, A.x = self.p.tolist(), self.i.tolist(), self.x.tolist()
        return A

    def rational(self, trans=False):
        """(X, gb, gA) in Fractions: X = op(A)^-1 B, gb = op(A)^-T GX, gA on the stored entries by the issue's formulas"""
        n, k = self.n, EXACT_K
        A = [[Fraction(int(self.dense[r, c])) for c in range(n)] for r in range(n)]
        At = [list(row) for row in zip(*A)]
        X = _rational_solve(At if trans else A, self.B)
        lam = _rational_solve(A if trans else At, self.GX)
        gA = []
        for q in range(len(self.i)):
            i, j = int(self.i[q]), int(self.cols[q])
            if self.sym:
                if i > j:
                    gA.append(Fraction(0))
                elif i == j:
                    gA.append(-sum(lam[i][c] * X[i][c] for c in range(k)))
                else:
                    gA.append(-sum(lam[i][c] * X[j][c] + lam[j][c] * X[i][c] for c in range(k)))
            elif trans:
                gA.append(-sum(X[i][c] * lam[j][c] for c in range(k)))
            else:
                gA.append(-sum(lam[i][c] * X[j][c] for c in range(k)))
        return X, lam, gA


def _rational_solve(A, B):
    """A^-1 B by Gauss-Jordan elimination in Fractions (A: rows of Fractions, nonsingular; B: an integer block)"""
    n, k = len(A), B.shape[1]
    M = [list(A[r]) + [Fraction(int(B[r, c])) for c in range(k)] for r in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c] != 0)
        M[c], M[piv] = M[piv], M[c]
        M[c] = [v / M[c][c] for v in M[c]]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c]
                M[r] = [a - f * b for a, b in zip(M[r], M[c])]
    return [row[n:] for row in M]


def as_floats(fr):
    """the Fractions as float64, asserting that each is one"""
    a = np.array([[float(v) for v in row] for row in fr] if fr and isinstance(fr[0], list) else [float(v) for v in fr])
    flat = [v for row in fr for v in row] if fr and isinstance(fr[0], list) else list(fr)
    assert all(Fraction(float(v)) == v for v in flat), "the fixture leaves the doubles"
    return a


def _exact():
    lower = _band(21, [-4, -2, 2, 4])
    lc = _band(22, [1, 2, 4])
    m = _band(23, [1])
    d = np.random.default_rng(24).choice([-4, -2, -1, 1, 2, 4], EXACT_N).astype(np.float64)
    return {"lower": Exact("lower", lower, False, 31), "chol": Exact("chol", lc @ lc.T, True, 32),
            "ldl": Exact("ldl", (m * d) @ m.T, True, 33)}


EXACT = _exact()
