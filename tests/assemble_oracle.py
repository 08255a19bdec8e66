"""Pure-Python restatement of the assembly plan (include/csx.h, "assembly plan"), written from its definition and
not from the library's loops, plus the inputs the CPU and the GPU tests share.

    plan(m, n, Ti, Tj) -> (p, i, sp, src)     the pattern of cs_dupl(cs_compress(T)) and, per slot, its triplets ascending
    fold(sp, src, v)   -> x                   x[s] = ((v[t0] + v[t1]) + v[t2]) + ..., the first term assigned
"""
import functools

import numpy as np


def plan(m, n, Ti, Tj):
    cols = [[] for _ in range(n)]
    for k in range(len(Ti)):
        i, j = int(Ti[k]), int(Tj[k])
        if not (0 <= i < m and 0 <= j < n):
            raise IndexError("list index out of range")
        cols[j].append(k)                      # a column's triplets, ascending: what a stable sort by column keeps
    p, rows, lists = [0], [], []
    for j in range(n):
        slot_of = {}                           # row -> its slot in this column: the first occurrence opens it
        for k in cols[j]:
            r = int(Ti[k])
            if r in slot_of:
                lists[slot_of[r]].append(k)
            else:
                slot_of[r] = len(rows)
                rows.append(r)
                lists.append([k])
        p.append(len(rows))
    sp, src = [0], []
    for lst in lists:
        src.extend(lst)
        sp.append(len(src))
    return p, rows, sp, src


def fold(sp, src, v, reverse=False):
    """reverse=True adds every slot's terms in the opposite order: a WRONG order the tests must be able to tell apart"""
    v = [float(t) for t in v]
    out = []
    for s in range(len(sp) - 1):
        terms = [v[src[t]] for t in range(sp[s], sp[s + 1])]
        if reverse:
            terms.reverse()
        acc = terms[0]
        for t in terms[1:]:
            acc = acc + t
        out.append(acc)
    return out


def as_bytes(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def composite(mod, m, n, Ti, Tj, Tx):
    """cs_dupl(cs_compress(T)) of module `mod` (the Python oracle, or the product)"""
    nz = len(Ti)
    T = mod.cs_spalloc(m, n, max(nz, 1), True, True)
    T.i[:nz] = [int(v) for v in Ti]
    T.p[:nz] = [int(v) for v in Tj]
    T.x[:nz] = [float(v) for v in Tx]
    T.nz = nz
    C = mod.cs_compress(T)
    assert mod.cs_dupl(C)
    return C


def triplet(mod, m, n, Ti, Tj, Tx=None):
    nz = len(Ti)
    T = mod.cs_spalloc(m, n, max(nz, 1), Tx is not None, True)
    T.i[:nz] = [int(v) for v in Ti]
    T.p[:nz] = [int(v) for v in Tj]
    if Tx is not None:
        T.x[:nz] = [float(v) for v in Tx]
    T.nz = nz
    return T


def split3(Ti, Tj, Tx, seed):
    """Every value in three parts: the first stays in place, the other two are appended after the originals in a seeded
    shuffle -- every slot then has duplicates, in an order that is not the slots'."""
    rng = np.random.default_rng(seed)
    Ti, Tj, Tx = np.asarray(Ti), np.asarray(Tj), np.asarray(Tx, dtype=np.float64)
    a = Tx * rng.uniform(0.2, 0.5, len(Tx))
    b = Tx * rng.uniform(-0.3, 0.4, len(Tx))
    c = Tx - a - b
    order = rng.permutation(2 * len(Tx))
    return (np.concatenate([Ti, np.concatenate([Ti, Ti])[order]]), np.concatenate([Tj, np.concatenate([Tj, Tj])[order]]),
            np.concatenate([a, np.concatenate([b, c])[order]]))


def wide(rng, count):
    """magnitudes 1e-8 .. 1e8, random signs: another order of additions changes bits"""
    return rng.choice([-1.0, 1.0], count) * 10.0 ** rng.uniform(-8, 8, count)


GOLDEN_WITH_TRIPLETS = ("ash219", "bcsstk01", "bcsstk16", "fs_183_1", "ibm32a", "ibm32b", "lp_afiro", "mbeacxc", "t1",
                        "west0067")


@functools.lru_cache(maxsize=None)
def golden_case(name, split):
    """(m, n, Ti, Tj, Tx, C) of a golden matrix, C = the oracle's cs_dupl(cs_compress(T)); computed once per session"""
    from conftest import golden
    import csparse_oracle as PO
    g = golden(name)
    m, n = int(g["T_mn"][0]), int(g["T_mn"][1])
    Ti, Tj, Tx = g["T_i"], g["T_j"], g["T_x"]
    if split:
        Ti, Tj, Tx = split3(Ti, Tj, Tx, 20260 + len(Ti))
    for a in (Ti, Tj, Tx):
        a.setflags(write=False)
    return m, n, Ti, Tj, Tx, composite(PO, m, n, Ti, Tj, Tx)


def random_cases():
    """(label, m, n, Ti, Tj, Tx): seeded random cases and the structural edges"""
    rng = np.random.default_rng(16)
    out = []
    for t in range(6):
        m, n, nz = 7, 5, 200
        out.append(("wide%d" % t, m, n, rng.integers(0, m, nz), rng.integers(0, n, nz), wide(rng, nz)))
    # slots of -0.0 only, and of [-0.0, 0.0]
    out.append(("negzero", 3, 2, np.array([0, 0, 0, 1, 1, 2]), np.array([0, 0, 0, 1, 1, 1]),
                np.array([-0.0, -0.0, -0.0, -0.0, 0.0, -0.0])))
    # empty first, middle and last columns
    Tj = rng.choice([1, 2, 4, 5], 60)
    out.append(("empty_columns", 6, 7, rng.integers(0, 6, 60), Tj, wide(rng, 60)))
    out.append(("nz0", 4, 3, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)))
    out.append(("n0", 4, 0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)))
    out.append(("one_column", 9, 4, rng.integers(0, 9, 150), np.full(150, 2), wide(rng, 150)))
    out.append(("m1", 1, 6, np.zeros(40, np.int64), rng.integers(0, 6, 40), wide(rng, 40)))
    out.append(("single", 5, 5, np.array([3]), np.array([1]), np.array([2.5])))
    return out


@functools.lru_cache(maxsize=None)
def golden_plan(name, split):
    """plan() of a golden case, computed once per session"""
    m, n, Ti, Tj, _, _ = golden_case(name, split)
    return plan(m, n, Ti, Tj)
