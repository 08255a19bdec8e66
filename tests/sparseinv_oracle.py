"""A pure-Python restatement of sparseinv: the Takahashi recurrence for Z = inv(L L') on the pattern of the
Cholesky factor L, in the one order of operations the device kernel reproduces bit for bit.

L is n-by-n CSC, every column non-empty, the diagonal entry first and positive, rows ascending.  With d = L(j,j), S_j = the rows
of column j below the diagonal in storage order and Zs(a, b) = the stored entry Z(max(a,b), min(a,b)):

    for j = n-1 down to 0:
        for every i in S_j:
            s = 0.0
            for k in S_j, in storage order:          # k == i: the diagonal of column i
                s = s + L(k,j) * Zs(i,k)             # product and sum rounded separately
            Z(i,j) = (-s) / d
        s = 0.0
        for k in S_j, in storage order:
            s = s + L(k,j) * Z(k,j)
        Z(j,j) = (1.0 / d - s) / d

Every Zs(i,k) read exists when the pattern is that of a Cholesky factor (S_j is a clique of the filled graph, so the pair lies
in column min(i,k), an ancestor of j in the elimination tree); a pattern where one does not raises ValueError.
tests/test_sparseinv_cpu.py holds this loop to numpy.linalg.inv."""


def sparseinv_x(n, p, i, x, columns=None):
    """Z.x as a list of len(x) floats for the factor (p, i, x: sequences of Python ints / floats).  columns: the columns to
    compute (any order; they are taken descending), which must be closed under "ancestor in the elimination tree" -- whole
    trees of the forest; entries of other columns stay None."""
    z = [None] * p[n]
    where = {}

    def pos(col, row):
        w = where.get(col)
        if w is None:
            w = where[col] = {i[q]: q for q in range(p[col], p[col + 1])}
        q = w.get(row)
        if q is None or z[q] is None:
            raise ValueError("Z(%d,%d) is not stored: not the pattern of a Cholesky factor" % (row, col))
        return q

    cols = range(n - 1, -1, -1) if columns is None else sorted(columns, reverse=True)
    for j in cols:
        b, e = p[j], p[j + 1]
        d = x[b]
        S = i[b + 1:e]
        lv = x[b + 1:e]
        for r, ii in enumerate(S):
            s = 0.0
            for t, k in enumerate(S):
                q = pos(k, ii) if k < ii else pos(ii, k)
                s = s + lv[t] * z[q]
            z[b + 1 + r] = (-s) / d
        s = 0.0
        for t in range(len(S)):
            s = s + lv[t] * z[b + 1 + t]
        z[b] = (1.0 / d - s) / d
    return z


def sparseinv(L):
    """Z for an oracle `cs` L: a new object of L's class with copies of L.p, L.i and the inverse's entries in x"""
    n = L.n
    nz = L.p[n]
    Z = type(L)()
    Z.m, Z.n, Z.nz, Z.nzmax = L.m, L.n, -1, L.nzmax
    Z.p = list(L.p)
    Z.i = list(L.i)
    Z.x = sparseinv_x(n, [int(v) for v in L.p], [int(v) for v in L.i[:nz]], [float(v) for v in L.x[:nz]]) + \
        [0.0] * (len(L.x) - nz)
    return Z


def dense_symmetric(n, p, i, zx):
    """the stored entries of Z scattered to a dense symmetric numpy matrix (zero elsewhere)"""
    import numpy as np
    D = np.zeros((n, n))
    for j in range(n):
        for q in range(p[j], p[j + 1]):
            D[i[q], j] = D[j, i[q]] = zx[q]
    return D
