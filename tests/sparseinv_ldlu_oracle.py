"""Pure-Python restatements of sparseinv_ldl and sparseinv_lu: the Takahashi recurrences for Z = inv(L D L') and
Z = inv(L U) on the pattern of L, in the one order of operations the device kernels reproduce bit for bit, the rule by which
csx_inverse_at reads an entry off the pattern, and a numpy form of both recurrences with the same bits.

L is n-by-n CSC on a Cholesky pattern: every column non-empty, the diagonal entry first (stored, never read: L is unit lower),
rows ascending.  S_j = the rows of column j below the diagonal in storage order.

LDL' (d: the n pivots; Zs(a, b) = the stored Z(max(a,b), min(a,b))):
    for j = n-1 .. 0:
        for i in S_j:  s = 0.0;  for k in S_j in storage order: s = s + L(k,j) * Zs(i,k);   Z(i,j) = -s
        s = 0.0;  for k in S_j in storage order: s = s + L(k,j) * Z(k,j);                   Z(j,j) = 1.0 / d[j] - s

LU (Ut on L's p and i, column j of Ut = row j of U, the pivot d = Ut(j,j) first; ZL(i,j) = Z(i,j), ZU(i,j) = Z(j,i), i >= j):
    for j = n-1 .. 0:
        for i in S_j:
            sL = 0.0; sU = 0.0
            for k in S_j in storage order:
                sL = sL + L(k,j)  * Z(i,k)      # ZL(i,k) if i > k, ZU(k,i) if i < k, the diagonal of column i if i == k
                sU = sU + Ut(k,j) * Z(k,i)      # the same slot in the other array
            ZL(i,j) = -sL;   ZU(i,j) = (-sU) / d
        s = 0.0;  for k in S_j in storage order: s = s + L(k,j) * ZU(k,j)
        ZL(j,j) = ZU(j,j) = 1.0 / d - s

Every product and every sum is rounded on its own.  tests/test_sparseinv_ldlu_cpu.py holds the loops to numpy.linalg.inv and
the numpy forms to the loops, byte for byte."""
import numpy as np


class _Where(object):
    """position of the stored pair (column, row), row >= column; ValueError for one that is not stored (or not computed yet)"""

    def __init__(self, p, i, z):
        self.p, self.i, self.z, self.cols = p, i, z, {}

    def __call__(self, col, row):
        w = self.cols.get(col)
        if w is None:
            w = self.cols[col] = {self.i[q]: q for q in range(self.p[col], self.p[col + 1])}
        q = w.get(row)
        if q is None or self.z[q] is None:
            raise ValueError("Z(%d,%d) is not stored: not the pattern of a Cholesky factor" % (row, col))
        return q


def ldl_x(n, p, i, x, d):
    """Z.x of inv(L D L') as a list of floats (p, i, x, d: sequences of Python ints / floats)"""
    z = [None] * p[n]
    pos = _Where(p, i, z)
    for j in range(n - 1, -1, -1):
        b, e = p[j], p[j + 1]
        S, lv = i[b + 1:e], x[b + 1:e]
        for r, ii in enumerate(S):
            s = 0.0
            for t, k in enumerate(S):
                s = s + lv[t] * z[pos(k, ii) if k < ii else pos(ii, k)]
            z[b + 1 + r] = -s
        s = 0.0
        for t in range(len(S)):
            s = s + lv[t] * z[b + 1 + t]
        z[b] = 1.0 / d[j] - s
    return z


def lu_x(n, p, i, lx, ux):
    """(ZL.x, ZU.x) of inv(L U) as two lists of floats"""
    zl, zu = [None] * p[n], [None] * p[n]
    pos = _Where(p, i, zl)
    for j in range(n - 1, -1, -1):
        b, e = p[j], p[j + 1]
        d = ux[b]
        S, lv, uv = i[b + 1:e], lx[b + 1:e], ux[b + 1:e]
        for r, ii in enumerate(S):
            sl = su = 0.0
            for t, k in enumerate(S):
                if k < ii:                     # Z(i,k) below the diagonal: ZL; Z(k,i) above it: ZU
                    q = pos(k, ii)
                    zik, zki = zl[q], zu[q]
                else:                          # (k == i: the diagonal of column i, the same in both)
                    q = pos(ii, k)
                    zik, zki = zu[q], zl[q]
                sl = sl + lv[t] * zik
                su = su + uv[t] * zki
            zl[b + 1 + r] = -sl
            zu[b + 1 + r] = (-su) / d
        s = 0.0
        for t in range(len(S)):
            s = s + lv[t] * zu[b + 1 + t]
        zl[b] = zu[b] = 1.0 / d - s
    return zl, zu


def gather(n, p, i, zl, zu, rmap, cmap, rows, cols):
    """csx_inverse_at's rule: for every t the entry Z(a, b), a = rmap[rows[t]], b = cmap[cols[t]] (None: the identity): a > b
    from column b of zl, a < b from column a of zu (None: of zl, a symmetric Z), a == b the first entry of column a; NaN for a
    pair that is not stored.  -> (numpy array, how many were missing)"""
    p, i = np.asarray(p), np.asarray(i)
    zl = np.asarray(zl, float)
    zu = zl if zu is None else np.asarray(zu, float)
    out, missing = np.empty(len(rows)), 0
    for t in range(len(rows)):
        a = int(rows[t]) if rmap is None else int(rmap[rows[t]])
        b = int(cols[t]) if cmap is None else int(cmap[cols[t]])
        col, row = min(a, b), max(a, b)
        q = p[col] + np.searchsorted(i[p[col] + 1:p[col + 1]], row) + 1 if a != b else p[col]
        if q < p[col + 1] and i[q] == row:
            out[t] = (zl if a >= b else zu)[q]
        else:
            out[t], missing = np.nan, missing + 1
    return out, missing


def _slots(n, p, i):
    """keys col * n + row of every stored entry (ascending: columns in order, rows ascending inside one)"""
    p, i = np.asarray(p, np.int64), np.asarray(i, np.int64)
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(p)) * n + i


def _positions(n, keys, S):
    """Q[r, t] = the position of the stored pair {S[r], S[t]} (column the smaller, row the larger)"""
    lo, hi = np.minimum(S[:, None], S[None, :]), np.maximum(S[:, None], S[None, :])
    want = lo * n + hi
    Q = np.searchsorted(keys, want)
    if Q.size and (Q.max() >= keys.size or not np.array_equal(keys[Q], want)):
        raise ValueError("a pair of one column is not stored: not the pattern of a Cholesky factor")
    return Q


def ldl_x_np(n, p, i, x, d):
    """ldl_x vectorised over the rows of a column: per term one elementwise multiply, then one add -- the same bits"""
    p, i = np.asarray(p, np.int64), np.asarray(i, np.int64)
    x, d = np.asarray(x, float), np.asarray(d, float)
    z = np.full(p[n], np.nan)
    keys = _slots(n, p, i)
    for j in range(n - 1, -1, -1):
        b, e = int(p[j]), int(p[j + 1])
        S, lv = i[b + 1:e], x[b + 1:e]
        m = e - b - 1
        Q = _positions(n, keys, S)
        s = np.zeros(m)
        for t in range(m):
            s = s + lv[t] * z[Q[:, t]]
        z[b + 1:e] = -s
        sd = 0.0
        for t in range(m):
            sd = sd + float(lv[t]) * float(z[b + 1 + t])
        z[b] = 1.0 / float(d[j]) - sd
    return z


def lu_x_np(n, p, i, lx, ux):
    """lu_x vectorised over the rows of a column -- the same bits"""
    p, i = np.asarray(p, np.int64), np.asarray(i, np.int64)
    lx, ux = np.asarray(lx, float), np.asarray(ux, float)
    zl, zu = np.full(p[n], np.nan), np.full(p[n], np.nan)
    keys = _slots(n, p, i)
    for j in range(n - 1, -1, -1):
        b, e = int(p[j]), int(p[j + 1])
        d = float(ux[b])
        S, lv, uv = i[b + 1:e], lx[b + 1:e], ux[b + 1:e]
        m = e - b - 1
        Q = _positions(n, keys, S)
        r = np.arange(m)
        sl, su = np.zeros(m), np.zeros(m)
        for t in range(m):
            below = t < r                      # S ascending: S[t] < S[r]
            a, c = zl[Q[:, t]], zu[Q[:, t]]
            sl = sl + lv[t] * np.where(below, a, c)
            su = su + uv[t] * np.where(below, c, a)
        zl[b + 1:e] = -sl
        zu[b + 1:e] = (-su) / d
        sd = 0.0
        for t in range(m):
            sd = sd + float(lv[t]) * float(zu[b + 1 + t])
        zl[b] = zu[b] = 1.0 / d - sd
    return zl, zu


def dense_lower_upper(n, p, i, zl, zu):
    """the stored entries scattered to a dense matrix: zl below and on the diagonal, zu (None: zl) above; zero elsewhere"""
    D = np.zeros((n, n))
    zu = zl if zu is None else zu
    for j in range(n):
        for q in range(p[j], p[j + 1]):
            D[i[q], j] = zl[q]
            D[j, i[q]] = zu[q]
    return D
