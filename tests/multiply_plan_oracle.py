"""Pure-Python restatement of the multiply plan (include/csx.h, "multiply plan"), written from its definition
and not from the library's loops, plus the inputs the CPU and the GPU tests share.

    plan(A, B) -> (p, i, sp, pair)      the pattern of cs_multiply(A, B) and, per slot, its products (ia, ib) in the reference's
                                        order; pair is flat: pair[2t], pair[2t + 1]
    fold(sp, pair, ax, bx, d=None, reverse=False, fused=False, bi=None) -> x
                                        x[s] = ((b0 a0) + b1 a1) + ..., every product rounded on its own, the first assigned;
                                        with d (and bi = B.i): b_t = d[bi[ib_t]] * bx[ib_t], rounded, in place of bx[ib_t]
"""
import functools
from fractions import Fraction

import numpy as np

from assemble_oracle import as_bytes, wide  # noqa: F401  (shared with the tests)


def plan(A, B):
    """A, B: anything with m, n, p, i (the oracle's cs, the product's cs).  IndexError for an index out of range, ValueError
    when A.n != B.m."""
    if A.n != B.m:
        raise ValueError("A.n != B.m")
    Ap, Ai, Bp, Bi = A.p, A.i, B.p, B.i
    for rows, cols, P, I in ((A.m, A.n, Ap, Ai), (B.m, B.n, Bp, Bi)):
        if P[0] != 0 or any(P[j + 1] < P[j] for j in range(cols)) or any(not 0 <= int(I[t]) < rows for t in range(P[cols])):
            raise IndexError("list index out of range")
    p, rows, lists = [0], [], []
    for j in range(B.n):
        slot_of = {}                                   # row -> its slot in this column: the first touch opens it
        for ib in range(Bp[j], Bp[j + 1]):             # B(:,j) in stored order ...
            c = int(Bi[ib])
            for ia in range(Ap[c], Ap[c + 1]):         # ... and inside it A(:, B.i[ib]) in stored order
                r = Ai[ia]
                s = slot_of.get(r)
                if s is None:
                    s = slot_of[r] = len(rows)
                    rows.append(int(r))
                    lists.append([])
                lists[s] += (ia, ib)
        p.append(len(rows))
    sp, pair = [0], []
    for lst in lists:                                  # (ia, ib, ia, ib, ...) of one slot
        pair += lst
        sp.append(len(pair) // 2)
    return p, rows, sp, pair


def _fma(a, b, c):
    """a * b + c with ONE rounding (math.fma is not in this Python); finite arguments"""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    return float(exact) if exact != 0 else a * b + c   # (a zero result keeps the sign plain arithmetic gives it)


def fold(sp, pair, ax, bx, d=None, reverse=False, fused=False, bi=None):
    """reverse=True adds every slot's terms in the opposite order; fused=True forms acc + beta * a with one rounding: two
    plausible WRONG kernels the tests must be able to tell apart from the right one"""
    ax, bx = [float(v) for v in ax], [float(v) for v in bx]
    if d is not None:
        bx = [float(d[int(bi[t])]) * bx[t] for t in range(len(bx))]      # one rounding
    out = []
    for s in range(len(sp) - 1):
        prods = [(bx[pair[2 * t + 1]], ax[pair[2 * t]]) for t in range(sp[s], sp[s + 1])]
        if reverse:
            prods.reverse()
        acc = prods[0][0] * prods[0][1]
        for beta, a in prods[1:]:
            if fused:
                acc = _fma(beta, a, acc)
            else:
                term = beta * a
                acc = acc + term
        out.append(acc)
    return out


def csc(mod, m, n, p, i, x=None):
    """a CSC matrix of module `mod` (the Python oracle, or the product) from arrays"""
    nnz = int(p[n])
    A = mod.cs_spalloc(m, n, max(nnz, 1), x is not None, False)
    A.p = [int(v) for v in p]
    A.i = [int(v) for v in i[:nnz]] + [0] * (max(nnz, 1) - nnz)
    if x is not None:
        A.x = [float(v) for v in x[:nnz]] + [0.0] * (max(nnz, 1) - nnz)
    return A


def scaled(mod, B, d):
    """B2 of the definition: B's pattern, B2.x[p] = d[B.i[p]] * B.x[p]"""
    nnz = B.p[B.n]
    return csc(mod, B.m, B.n, B.p, B.i, [float(d[B.i[t]]) * B.x[t] for t in range(nnz)])


def arrays(A):
    """(p, i, x) of a cs as numpy arrays trimmed to nnz (x None for a pattern)"""
    nnz = A.p[A.n]
    return (np.asarray(A.p, np.int32), np.asarray(A.i[:nnz], np.int32),
            None if A.x is None else np.asarray(A.x[:nnz], np.float64))


def c_multiply(A, B):
    """cs_multiply(A, B) by the plain-C oracle: (p, i, x) as lists / numpy"""
    import c_oracle as CO
    ap, ai, ax = arrays(A)
    bp, bi, bx = arrays(B)
    Cp, Ci, Cx = CO.multiply(A.m, A.n, B.n, ap, ai, ax, bp, bi, bx)
    return [int(v) for v in Cp], [int(v) for v in Ci], Cx


GOLDEN = ("t1", "bcsstk01", "west0067", "ash219", "fs_183_1", "ibm32a", "ibm32b", "lp_afiro", "bcsstk16", "mbeacxc")
SMALL = GOLDEN[:8]


@functools.lru_cache(maxsize=None)
def golden_pair(name, transposed=False):
    """(A, AT) of a golden matrix as oracle matrices ((AT, A) when transposed); made once per session, never modified"""
    from conftest import golden, unpack
    import csparse_oracle as PO
    g = golden(name)
    A, AT = unpack(PO, g, "A"), unpack(PO, g, "AT")
    return (AT, A) if transposed else (A, AT)


@functools.lru_cache(maxsize=None)
def golden_plan(name, transposed=False):
    return plan(*golden_pair(name, transposed))


@functools.lru_cache(maxsize=None)
def golden_product(name, transposed=False):
    """(p, i, x) of the oracle's product: the Python oracle on the small matrices, the C oracle on the two large ones"""
    import csparse_oracle as PO
    A, B = golden_pair(name, transposed)
    if name in SMALL:
        C = PO.cs_multiply(A, B)
        nnz = C.p[C.n]
        assert len(C.i) == nnz
        return C.p, C.i, np.asarray(C.x[:nnz], np.float64)
    return c_multiply(A, B)


def synthetic_pairs():
    """(label, A, B) over the synthetic_20240601 cases: A AT and AT A (duplicates inside columns, empty columns, cancellation)"""
    from conftest import golden, unpack
    import csparse_oracle as PO
    g = golden("synthetic_20240601")
    out = []
    for c in range(len(g["cases"])):
        A, AT = unpack(PO, g, "c%d_A" % c), unpack(PO, g, "c%d_AT" % c)
        out.append(("c%d_AAT" % c, A, AT))
        out.append(("c%d_ATA" % c, AT, A))
    return out


def random_csc(rng, m, n, lens, values=wide):
    """CSC with the given column lengths: rows in random order, duplicates inside a column allowed"""
    import csparse_oracle as PO
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(p[-1])
    i = rng.integers(0, max(m, 1), nnz)
    return csc(PO, m, n, p, i, values(rng, nnz))


def wide_pairs():
    """(label, A, B): seeded random products with wide-magnitude values and long slots -- another order of the additions, or
    a fused multiply-add, changes bits"""
    rng = np.random.default_rng(18)
    out = []
    for t in range(4):
        m, k, n = 5, 40, 4
        out.append(("wide%d" % t, random_csc(rng, m, k, rng.integers(0, 6, k)), random_csc(rng, k, n, rng.integers(10, 40, n))))
    return out


def edge_pairs():
    """(label, A, B): the structural edges"""
    import csparse_oracle as PO
    rng = np.random.default_rng(19)
    out = []
    out.append(("k0", csc(PO, 4, 0, [0], [], []), csc(PO, 0, 3, [0, 0, 0, 0], [], [])))
    out.append(("n0", random_csc(rng, 4, 3, [2, 1, 2]), csc(PO, 3, 0, [0], [], [])))
    out.append(("m0", csc(PO, 0, 3, [0, 0, 0, 0], [], []), random_csc(rng, 3, 2, [2, 2])))
    # B names only empty columns of A: entries in both, no product
    out.append(("products0", csc(PO, 4, 3, [0, 0, 2, 2], [1, 3], [1.5, -2.0]), csc(PO, 3, 2, [0, 2, 3], [0, 2, 0], [1.0, 2.0, 3.0])))
    out.append(("empty_columns", random_csc(rng, 6, 5, [0, 3, 0, 4, 0]), random_csc(rng, 5, 6, [0, 3, 0, 0, 5, 0])))
    # the same row twice in a column of A, the same row twice in a column of B
    out.append(("duplicates", csc(PO, 3, 2, [0, 3, 5], [2, 0, 2, 1, 1], wide(rng, 5)),
                csc(PO, 2, 2, [0, 3, 5], [1, 0, 1, 0, 0], wide(rng, 5))))
    out.append(("negzero", csc(PO, 2, 3, [0, 1, 2, 4], [0, 0, 1, 1], [-0.0, -0.0, -0.0, 0.0]),
                csc(PO, 3, 1, [0, 3], [0, 1, 2], [1.0, 1.0, 1.0])))
    out.append(("single", csc(PO, 1, 1, [0, 1], [0], [2.5]), csc(PO, 1, 1, [0, 1], [0], [-4.0])))
    return out
