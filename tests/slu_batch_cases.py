"""Inputs shared by the tests of slusol_factor(...).batch(), on the cases of tests/slu_cases.py and the rule of
tests/slu_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

Members: the first three of every case are its value sets "A", A2[0], A2[1] (the ones tests/slu_oracle.reference caches); a wider
batch goes on with case.scaled(WIDE_SEED + m), new values of the same kind from seeds nobody else uses.

Sizes: B members and r right-hand sides a member, on both sides of every constant of _csx.slu_batch_limits():
  WALK_WAVES     a level of that many columns goes to the walker, one more to the level kernel: the cases chains4 / chains5
  SOLVE_THREADS  (row, column) pairs a solve workgroup of a wide level takes: a wide level of chains5 (WALK_WAVES + 1 rows) with
                 WIDE_EDGE_B members is the last that fits one workgroup / the first that needs two
  SOLVE_FETCH    terms of a chain a thread of a wide level fetches together: FETCH_CASES have rows and columns in wide levels with
                 one fewer, as many, one more and more than twice as many terms (the CPU test asserts it)
  RUN_WAVES      (row, right-hand side) pairs a solve walker takes at a time: a walker level of chains4 (WALK_WAVES rows) with
                 RUN_EDGE_R right-hand sides is exactly one pass / the first with two
  RUN_FETCH      terms of a chain a walker's wave fetches together: RUN_FETCH_CASES (dense triangles, every level one column) have
                 rows and columns in narrow levels on both sides of it in the same way
  MAX_MEMBERS    the most members of a batch: on the case `one` (one entry) at the limit, refused one above
and the wave's width, which no kernel here is cut by but every count passes: B r = 64 and 65."""
import numpy as np

import _csx
import slu_cases as SC
import slu_oracle as SO

LIMITS = _csx.slu_batch_limits()
WAVES, THREADS, FETCH, MAX_MEMBERS = (LIMITS[k] for k in ("WALK_WAVES", "SOLVE_THREADS", "SOLVE_FETCH", "MAX_MEMBERS"))
RUN_WAVES, RUN_FETCH = LIMITS["RUN_WAVES"], LIMITS["RUN_FETCH"]

WIDE_SEED = 20241020
B_SIZES = (1, 2, 3, 65)
R_SIZES = (1, 3)
WAVE_SHAPES = ((64, 1), (65, 1))                                   # (B, r) with B r = 64, 65
WIDE_EDGE_B = (THREADS // (WAVES + 1), THREADS // (WAVES + 1) + 1)   # r = 1 on chains5
RUN_EDGE_R = (RUN_WAVES // WAVES, RUN_WAVES // WAVES + 1)          # B = 2 on chains4
FETCH_CASES = ("grid24", "one-sided")
RUN_FETCH_CASES = ("long-column", "long-column-updated")
CPU_SWEEP_CASES = ("chain257", "grid24-shift", "west", "saddle-natural")
LAUNCH_CASES = ("chain257", "chains4", "chains5", "grid24")


def member(case, m):
    """the values of member m of a batch on `case`"""
    return case.values(SC.VALUE_SETS[m]) if m < len(SC.VALUE_SETS) else case.scaled(WIDE_SEED + m)


def members(case, B):
    """nnz x B: column m = member(case, m)"""
    return np.ascontiguousarray(np.stack([member(case, m) for m in range(B)], axis=1))


def levels_of(case):
    """the columns by height level of the elimination tree (csx_levelwalk.h's height_levels): a leaf at 0, a column one above its
    highest child; ascending inside a level"""
    parent = SO.pattern_of(case)[2]
    level = [0] * case.n
    for j in range(case.n):
        if parent[j] >= 0:
            level[parent[j]] = max(level[parent[j]], level[j] + 1)
    out = [[] for _ in range(max(level) + 1 if case.n else 0)]
    for j in range(case.n):
        out[level[j]].append(j)
    return out


def row_view(case):
    """row j of the pattern: [(k, slot of (j, k))], k ascending, the diagonal last"""
    Lp, Li, _ = SO.pattern_of(case)
    rows = [[] for _ in range(case.n)]
    for k in range(case.n):
        for q in range(Lp[k], Lp[k + 1]):
            rows[Li[q]].append((k, q))
    return rows


def chain_lengths(case, wide):
    """({terms of a row's chain}, {terms of a column's chain}) over the columns of the wide levels (more than WALK_WAVES columns:
    a thread a chain) or of the narrow ones (a walker's wave a chain)"""
    Lp, rows = SO.pattern_of(case)[0], row_view(case)
    js = [j for cols in levels_of(case) if (len(cols) > WAVES) == wide for j in cols]
    return {len(rows[j]) - 1 for j in js}, {Lp[j + 1] - Lp[j] - 1 for j in js}


def level_sweeps(case, Lx, Ux, b, trans):
    """The two sweeps of csx_slu_batch_solve between the permutations, restated in plain Python floats (every product and every
    difference rounded on its own), level by level as the device runs them:
      ascending levels, row gather:    x_j = ((x_j - v1 x_k1) - v2 x_k2) - ... over row j's entries off the diagonal, k ascending
      descending levels, column dot:   the same chain over column j's stored entries below the diagonal, in storage order
    each followed by / d_j when the factor read is Ut (L is unit: nothing).  trans: Ut first, then L."""
    Lp, Li, _ = SO.pattern_of(case)
    levels, rows = levels_of(case), row_view(case)
    x = [float(v) for v in b]
    v1, d1, v2, d2 = (Ux, True, Lx, False) if trans else (Lx, False, Ux, True)
    for cols in levels:
        for j in cols:
            s = x[j]
            for k, at in rows[j][:-1]:
                t = float(v1[at]) * x[k]
                s = s - t
            x[j] = s / float(v1[Lp[j]]) if d1 else s
    for cols in reversed(levels):
        for j in cols:
            s = x[j]
            for q in range(Lp[j] + 1, Lp[j + 1]):
                t = float(v2[q]) * x[Li[q]]
                s = s - t
            x[j] = s / float(v2[Lp[j]]) if d2 else s
    return x


def reference_sweeps(O, case, Lx, Ux, b, trans):
    """cs_lsolve then cs_ltsolve of the restated reference O on the factors: of L then Ut, or (trans) of Ut then L"""
    Lp, Li, _ = SO.pattern_of(case)

    def mat(x):
        M = O.cs_spalloc(case.n, case.n, max(len(Li), 1), True, False)
        M.p, M.i, M.x = list(Lp), list(Li), [float(v) for v in x]
        return M

    x = [float(v) for v in b]
    first, second = (Ux, Lx) if trans else (Lx, Ux)
    assert O.cs_lsolve(mat(first), x) and O.cs_ltsolve(mat(second), x)
    return x
