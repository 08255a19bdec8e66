"""Pure-Python restatement of the add plan (include/csx.h, "add plan"), written from its definition and not from
the library's loops, plus the inputs the CPU and the GPU tests share.

    plan(ops) -> (p, i, sp, src, off)     the pattern of the chain of cs_add over the operands and, per slot, the positions of
                                          its terms in the concatenated value arrays, in the reference's order
    fold(sp, src, off, coef, xs, reverse=False, fused=False) -> x
                                          x[s] = ((c x) + c' x') + ..., every c x rounded on its own, the first assigned
    chain(mod, ops, coef)                 the reference's chain by module `mod` (the oracle, or the product)
"""
import functools
from fractions import Fraction

import numpy as np

from assemble_oracle import as_bytes, wide  # noqa: F401  (shared with the tests)
from multiply_plan_oracle import arrays, csc, random_csc  # noqa: F401

MAX_OPERANDS = 8


def plan(ops):
    """ops: 2 .. 8 things with m, n, p, i of one shape.  IndexError for an index out of range or bad pointers, ValueError for
    an operand count outside 2 .. 8 or shapes that differ."""
    k = len(ops)
    if not 2 <= k <= MAX_OPERANDS or any((A.m, A.n) != (ops[0].m, ops[0].n) for A in ops):
        raise ValueError("2 .. 8 operands of one shape")
    m, n = ops[0].m, ops[0].n
    off = [0]
    for A in ops:
        P, I = A.p, A.i
        if P[0] != 0 or any(P[j + 1] < P[j] for j in range(n)) or any(not 0 <= int(I[t]) < m for t in range(P[n])):
            raise IndexError("list index out of range")
        off.append(off[-1] + P[n])
    p, rows, lists = [0], [], []
    for j in range(n):
        slot_of = {}                                   # row -> its slot in this column: the first touch opens it
        for r, A in enumerate(ops):                    # A_0(:,j) as stored, then A_1(:,j), ...
            for e in range(A.p[j], A.p[j + 1]):
                row = int(A.i[e])
                s = slot_of.get(row)
                if s is None:
                    s = slot_of[row] = len(rows)
                    rows.append(row)
                    lists.append([])
                lists[s].append(off[r] + e)
        p.append(len(rows))
    sp, src = [0], []
    for lst in lists:
        src += lst
        sp.append(len(src))
    return p, rows, sp, src, off


def _fma(a, b, c):
    """a * b + c with ONE rounding, exactly (fractions, then one conversion); finite arguments"""
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    return float(exact) if exact != 0 else a * b + c   # (a zero result keeps the sign plain arithmetic gives it)


def fold(sp, src, off, coef, xs, reverse=False, fused=False):
    """xs: the operands' value arrays.  reverse=True adds every slot's terms in the opposite order; fused=True forms acc + c * x
    with one rounding: two plausible WRONG kernels the tests must be able to tell apart from the right one"""
    k = len(xs)
    flat, owner = [], []
    for r in range(k):
        vals = [float(v) for v in xs[r][:off[r + 1] - off[r]]]
        assert len(vals) == off[r + 1] - off[r]
        flat += vals
        owner += [r] * len(vals)
    coef = [float(c) for c in coef]
    out = []
    for s in range(len(sp) - 1):
        terms = [(coef[owner[g]], flat[g]) for g in src[sp[s]:sp[s + 1]]]
        if reverse:
            terms.reverse()
        acc = terms[0][0] * terms[0][1]
        for c, x in terms[1:]:
            if fused:
                acc = _fma(c, x, acc)
            else:
                term = c * x
                acc = acc + term
        out.append(acc)
    return out


def chain(mod, ops, coef):
    """C_1 = cs_add(A_0, A_1, c_0, c_1), C_r = cs_add(C_{r-1}, A_r, 1, c_r)"""
    C = mod.cs_add(ops[0], ops[1], coef[0], coef[1])
    for r in range(2, len(ops)):
        C = mod.cs_add(C, ops[r], 1, coef[r])
    return C


def values(A):
    return None if A.x is None else A.x[:A.p[A.n]]


def with_values(A, x):
    """A's pattern with other values (None: pattern only), as an oracle matrix"""
    import csparse_oracle as PO
    return csc(PO, A.m, A.n, A.p, A.i, x)


GOLDEN = ("t1", "bcsstk01", "west0067", "fs_183_1", "bcsstk16")   # the square ones: A + A' exists


@functools.lru_cache(maxsize=None)
def golden_case(name, k):
    """(ops, coef, C): A + A' (k = 2) or A + 2 A' - 0.5 A (k = 3) of a golden matrix, C the oracle's chain; made once per session,
    never modified"""
    from conftest import golden, unpack
    import csparse_oracle as PO
    g = golden(name)
    A, AT = unpack(PO, g, "A"), unpack(PO, g, "AT")
    ops, coef = ((A, AT), (1.0, 1.0)) if k == 2 else ((A, AT, A), (1.0, 2.0, -0.5))
    return ops, coef, chain(PO, ops, coef)


@functools.lru_cache(maxsize=None)
def golden_plan(name, k):
    return plan(golden_case(name, k)[0])


def coefficients(rng, k):
    """full mantissas, both signs"""
    return (rng.choice([-1.0, 1.0], k) * rng.uniform(0.3, 3.0, k)).tolist()


def same_pattern(rng, A):
    import csparse_oracle as PO
    return csc(PO, A.m, A.n, A.p, A.i, wide(rng, A.p[A.n]))


def synthetic_cases():
    """(label, ops, coef): seeded random sums -- duplicates inside columns of any operand (random_csc draws rows with
    replacement), the same operand twice, disjoint and identical patterns, k = 2, 3, 8"""
    import csparse_oracle as PO
    rng = np.random.default_rng(19)
    out = []
    for k in (2, 3, 8):
        m, n = 6, 5
        ops = [random_csc(rng, m, n, rng.integers(0, 9, n)) for _ in range(k)]
        out.append(("random_k%d" % k, ops, coefficients(rng, k)))
    A = random_csc(rng, 7, 4, [5, 0, 9, 3])
    out.append(("twice", [A, A], coefficients(rng, 2)))
    out.append(("twice_k3", [A, random_csc(rng, 7, 4, [2, 2, 0, 6]), A], coefficients(rng, 3)))
    E = csc(PO, 8, 3, [0, 2, 4, 5], [0, 2, 4, 6, 0], wide(rng, 5))
    O = csc(PO, 8, 3, [0, 2, 3, 5], [1, 3, 5, 7, 1], wide(rng, 5))
    out.append(("disjoint", [E, O], coefficients(rng, 2)))
    out.append(("identical", [E, same_pattern(rng, E)], coefficients(rng, 2)))
    out.append(("identical_k3", [E, same_pattern(rng, E), same_pattern(rng, E)], coefficients(rng, 3)))
    out.append(("identical_k8", [E] + [same_pattern(rng, E) for _ in range(7)], coefficients(rng, 8)))
    # the same rows in another stored order: same pattern as a set, not aligned
    R = csc(PO, 8, 3, [0, 2, 4, 5], [2, 0, 6, 4, 0], wide(rng, 5))
    out.append(("reordered", [E, R], coefficients(rng, 2)))
    return out


def edge_cases():
    """(label, ops, coef): the structural edges"""
    import csparse_oracle as PO
    rng = np.random.default_rng(20)
    out = []
    out.append(("m0", [csc(PO, 0, 3, [0, 0, 0, 0], [], [])] * 2, [1.5, -2.0]))
    out.append(("n0", [csc(PO, 4, 0, [0], [], []), csc(PO, 4, 0, [0], [], [])], [1.5, -2.0]))
    out.append(("empty_columns", [random_csc(rng, 6, 5, [0, 3, 0, 4, 0]), random_csc(rng, 6, 5, [0, 0, 2, 5, 0])], [0.7, 1.3]))
    Z = csc(PO, 5, 3, [0, 0, 0, 0], [], [])
    F = random_csc(rng, 5, 3, [3, 0, 4])
    out.append(("empty_first", [Z, F], [2.0, 1.1]))
    out.append(("empty_last", [F, Z], [1.1, 2.0]))
    out.append(("empty_middle", [F, Z, same_pattern(rng, F)], [1.1, 2.0, -0.3]))
    out.append(("all_empty", [Z, Z, Z], [1.0, 1.0, 1.0]))
    out.append(("single", [csc(PO, 1, 1, [0, 1], [0], [2.5]), csc(PO, 1, 1, [0, 1], [0], [-4.0])], [3.0, 0.1]))
    return out


def zero_cases():
    """(label, ops, coef, expected values): the signs of zero the definition fixes"""
    import csparse_oracle as PO
    one = lambda v: csc(PO, 2, 1, [0, 2], [0, 1], v)                  # noqa: E731
    dup = csc(PO, 2, 1, [0, 4], [0, 1, 0, 1], [-0.0, 0.0, -0.0, -0.0])  # duplicates inside the column
    return [
        ("all_negzero", [dup, one([-0.0, -0.0])], [1.0, 2.0], [-0.0, 0.0]),     # slot 0: -0 -0 -0; slot 1: (0 + -0) + -0 = 0
        ("negzero_k3", [one([-0.0, 0.0]), one([-0.0, 0.0]), one([0.0, 0.0])], [1.0, 1.0, -1.0], [-0.0, 0.0]),
        ("c0", [one([3.0, -3.0]), one([-5.0, -5.0])], [0.0, 0.0], [0.0, -0.0]),  # 0 * 3 + 0 * -5 = 0 + -0; 0 * -3 + 0 * -5 = -0 + -0
        ("c0_single", [one([3.0, -3.0]), csc(PO, 2, 1, [0, 0], [], [])], [0.0, 1.0], [0.0, -0.0]),   # the product's sign
        ("cancel", [one([1.25, -7.5]), one([1.25, -7.5])], [1, -1], [0.0, 0.0]),
    ]


def boundary_case(thr, seed):
    """k = 8 operands, m = 9 rows, one column besides an empty one: slot q has lens[q] terms, dealt to the operands at random with
    at least one from every operand wherever the slot has 8 or more (its terms then come from all eight operands, interleaved with
    the other slots' in each operand's column, which is stored shuffled: duplicates inside the columns of every operand).
    Returns (ops, coef, lens of the slots in C's order)."""
    import csparse_oracle as PO
    lens = [thr - 1, thr, thr + 1, 63, 64, 65, 127, 128, 129]
    assert min(lens) >= 1
    rng = np.random.default_rng(seed)
    m, k = len(lens), MAX_OPERANDS
    share = np.zeros((m, k), np.int64)                  # share[row, r]: terms of slot `row` held by operand r
    for row, L in enumerate(lens):
        if L >= k:
            share[row] = 1 + rng.multinomial(L - k, np.ones(k) / k)
        else:
            share[row, rng.choice(k, L, replace=False)] = 1
    ops = []
    for r in range(k):
        rows = rng.permutation(np.repeat(np.arange(m), share[:, r]))
        ops.append(csc(PO, m, 2, [0, 0, len(rows)], rows, wide(rng, len(rows))))
    C = plan(ops)
    order = C[1]                                        # rows in first-touch order
    return ops, coefficients(rng, k), [lens[row] for row in order]


def edge_count_case(nnz, aligned, seed):
    """Two operands (three for odd seeds) with nnz slots in their sum: the same pattern, rows stored shuffled, in all of them
    (the aligned class); or, not aligned, the last operand with one extra entry at the head of its first column that
    duplicates a row (same slots, one more term).  Several columns wherever nnz allows."""
    import csparse_oracle as PO
    rng = np.random.default_rng(seed)
    k = 2 + seed % 2
    ncol = 1 if nnz < 8 else 3
    cuts = [0] + sorted(rng.integers(0, nnz + 1, ncol - 1).tolist()) + [nnz]
    rows = np.concatenate([rng.permutation(nnz)[:cuts[j + 1] - cuts[j]] for j in range(ncol)]).astype(np.int64)
    ops = [csc(PO, nnz, ncol, cuts, rows, wide(rng, nnz)) for _ in range(k)]
    if not aligned:
        first = next(j for j in range(ncol) if cuts[j + 1] > cuts[j])
        at = cuts[first]
        p2 = [c + (1 if j > first else 0) for j, c in enumerate(cuts)]
        i2 = np.concatenate([rows[:at], rows[at:at + 1], rows[at:]])
        ops[-1] = csc(PO, nnz, ncol, p2, i2, wide(rng, nnz + 1))
    return ops, coefficients(rng, k)


@functools.lru_cache(maxsize=None)
def pencil(side=12):
    """(K, M) of an SPD pencil on the side x side grid pattern (5-point stencil, full symmetric storage, rows ascending): K the
    stiffness-like matrix (diagonal 4 + small, off-diagonals -1 scaled), M a diagonally dominant mass-like matrix on the same
    pattern.  Values with full mantissas."""
    import csparse_oracle as PO
    rng = np.random.default_rng(12)
    n = side * side
    cols = []
    for j in range(n):
        y, x = divmod(j, side)
        nb = [j]
        if x > 0:
            nb.append(j - 1)
        if x < side - 1:
            nb.append(j + 1)
        if y > 0:
            nb.append(j - side)
        if y < side - 1:
            nb.append(j + side)
        cols.append(sorted(nb))
    p = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    i = np.concatenate(cols)
    w = {}                                              # symmetric off-diagonal weights
    kx, mx = [], []
    for j in range(n):
        for r in cols[j]:
            if r == j:
                kx.append(4.0 + rng.uniform(0.1, 0.5))
                mx.append(2.0 + rng.uniform(0.1, 0.5))
            else:
                key = (min(r, j), max(r, j))
                if key not in w:
                    w[key] = (-rng.uniform(0.5, 1.0), rng.uniform(0.05, 0.25))
                kx.append(w[key][0])
                mx.append(w[key][1])
    return csc(PO, n, n, p, i, kx), csc(PO, n, n, p, i, mx)
