"""The value rule of csx_residual_sym_block / csx_residual_sym_host and of csx_norm1_sym, CPU side -- TEST
INFRASTRUCTURE, NOT PRODUCT.

A is n x n CSC with values, columns possibly unsorted and with duplicates.  S is the symmetric matrix a Cholesky factorisation
sees in A: the stored entries with row <= column, mirrored; strictly lower entries are ignored.  For output row i the terms
(a, j) come in two phases, in plain Python floats (loops; every multiply, subtract, add and divide rounded on its own):

    phase 1: the entries q of stored column i, in storage order, with A.i[q] <= i:                    (A.x[q], A.i[q])
    phase 2: the entries of row i with column > i, in ascending (column, storage position) order -- the order of the
             stable row gather, built here by a sweep over the columns:                               (value, column)
    r = B[i,c];    t = a * X[j,c];      r = r - t
    d = |B[i,c]|;  u = |a| * |X[j,c]|;  d = d + u
    ratio = 0 when |r| == 0 and d == 0, else |r| / d;  omega[c], rnorm[c]: maxima over the rows of the bit patterns

An entry that fails its phase's test is skipped, not added as a zero.  norm1(): max_i sum |a| over row i's terms in that
order, the maximum over the bit patterns.

phase2_first=True and keep_lower=True are two MISTAKES a kernel could make -- the two phases in the other order, and the
test of phase 1 forgotten, so that the strictly lower entries of column i count as terms (a, A.i[q]) of row i -- kept here
so that the tests can show that neither gives the right bytes."""
from residual_oracle import bits, divide, from_bits


def rows_of(n, p, i, x, phase2_first=False, keep_lower=False):
    """the terms of every row of S, in the rule's order: lists of (a, j)"""
    first = [[(float(x[q]), int(i[q])) for q in range(int(p[r]), int(p[r + 1])) if keep_lower or int(i[q]) <= r]
             for r in range(n)]
    second = [[] for _ in range(n)]
    for j in range(n):
        for q in range(int(p[j]), int(p[j + 1])):
            if int(i[q]) < j:
                second[int(i[q])].append((float(x[q]), j))
    return [b + a if phase2_first else a + b for a, b in zip(first, second)]


def residual(n, p, i, x, k, X, B, phase2_first=False, keep_lower=False):
    """(R, omega, rnorm): X, B flat row-major sequences of n k floats; R a flat list"""
    R = [0.0] * (n * k)
    wmax, amax = [0] * k, [0] * k
    for r_i, terms in enumerate(rows_of(n, p, i, x, phase2_first, keep_lower)):
        for c in range(k):
            r = float(B[r_i * k + c])
            d = abs(r)
            for a, j in terms:
                xv = float(X[j * k + c])
                t = a * xv
                r = r - t
                u = abs(a) * abs(xv)
                d = d + u
            R[r_i * k + c] = r
            ar = abs(r)
            ratio = 0.0 if (ar == 0.0 and d == 0.0) else divide(ar, d)
            wmax[c] = max(wmax[c], bits(ratio))
            amax[c] = max(amax[c], bits(ar))
    return R, [from_bits(u) for u in wmax], [from_bits(u) for u in amax]


def norm1(n, p, i, x):
    """|S|_1 as csx_norm1_sym computes it (0.0 for n == 0)"""
    best = 0
    for terms in rows_of(n, p, i, x):
        s = 0.0
        for a, _ in terms:
            s = s + abs(a)
        best = max(best, bits(s))
    return from_bits(best)
