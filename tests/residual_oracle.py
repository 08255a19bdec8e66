"""The value rule of csx_residual_block / csx_residual_host, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

residual(): R = B - op(A) X for row-major blocks of k columns with, per column, omega = max_i |r| / (|op(A)| |X| + |B|)_i
and rnorm = max_i |r|, in plain Python floats (loops; every multiply, subtract, add and divide rounded on its own):

    row i of op(A): its terms (a_q, j_q) in ascending (column, storage position) order (op(A) = A; the order is built
                    here by a stable sweep over the columns) or in the storage order of column i of A (op(A) = A')
    r = B[i,c];    t = a_q * X[j_q,c];      r = r - t
    d = |B[i,c]|;  u = |a_q| * |X[j_q,c]|;  d = d + u
    ratio = 0 when |r| == 0 and d == 0, else |r| / d (IEEE: x / 0 = inf, 0 / 0 and NaN give NaN)
    omega[c], rnorm[c]: maxima over the rows of the bit patterns of the non-negative doubles (NaN ranks above inf)

fused=True and reverse=True are two MISTAKES a kernel could make -- the subtraction fused into one multiply-add, and the
row's terms from last to first -- kept here so that the tests can show that neither gives the right bytes."""
import math
import struct
from fractions import Fraction


def bits(v):
    """the bit pattern of |v| as an unsigned integer"""
    return struct.unpack("<Q", struct.pack("<d", abs(v)))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def divide(a, d):
    """a / d for a >= 0 or NaN and d >= 0 or NaN as IEEE 754 has it (Python raises for d == 0)"""
    if d == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.inf
    return a / d


def rows_of(m, n, p, i, x, trans):
    """the terms of every row of op(A), in the rule's order: lists of (a, j)"""
    if trans:
        return [[(float(x[q]), int(i[q])) for q in range(int(p[j]), int(p[j + 1]))] for j in range(n)]
    rows = [[] for _ in range(m)]
    for j in range(n):
        for q in range(int(p[j]), int(p[j + 1])):
            rows[int(i[q])].append((float(x[q]), j))
    return rows


def _fma_sub(r, a, x):
    """r - a x with one rounding (finite arguments)"""
    return float(Fraction(r) - Fraction(a) * Fraction(x))


def residual(m, n, p, i, x, k, trans, X, B, fused=False, reverse=False):
    """(R, omega, rnorm): X, B flat row-major sequences of (columns of op(A)) k and (rows of op(A)) k floats; R a flat list"""
    rows = rows_of(m, n, p, i, x, trans)
    R = [0.0] * (len(rows) * k)
    wmax, amax = [0] * k, [0] * k
    for r_i, terms in enumerate(rows):
        if reverse:
            terms = terms[::-1]
        for c in range(k):
            r = float(B[r_i * k + c])
            d = abs(r)
            for a, j in terms:
                xv = float(X[j * k + c])
                if fused:
                    r = _fma_sub(r, a, xv)
                else:
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
