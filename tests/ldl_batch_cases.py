"""Inputs shared by the tests of ldlsol_factor(...).batch(), on the cases of tests/ldl_cases.py and the rule of
tests/ldl_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

Members: the first three of every case are its value sets "A", A2[0], A2[1] (the ones tests/ldl_oracle.reference caches); a wider
batch goes on with case.congruent(WIDE_SEED + m), new values of the same inertia from seeds nobody else uses.

Sizes: B members and r right-hand sides a member, on both sides of every constant of _csx.ldl_batch_limits():
  WALK_WAVES     a level of that many columns goes to the walker, one more to the level kernel: the cases chains4 / chains5
  SOLVE_THREADS  (row, column) pairs a solve workgroup of a wide level takes: a wide level of chains5 (WALK_WAVES + 1 rows) with
                 WIDE_EDGE_B members is the last that fits one workgroup / the first that needs two
  SOLVE_FETCH    terms of a chain a thread of a wide level fetches together: FETCH_CASES together have rows and columns in wide
                 levels with one fewer, as many, one more and more than twice as many terms (the CPU test asserts it)
  RUN_WAVES      (row, right-hand side) pairs a solve walker takes at a time: a walker level of chains4 (WALK_WAVES rows) with
                 RUN_EDGE_R right-hand sides is exactly one pass / the first with two
  RUN_FETCH      terms of a chain a walker's wave fetches together: RUN_FETCH_CASES (arrows whose factor is a dense triangle, every
                 level one column) have rows and columns in narrow levels on both sides of it in the same way
  MAX_MEMBERS    the most members of a batch: on the case `one` (one entry) at the limit, refused one above
and the wave's width, which no kernel here is cut by but every count passes: B r = 64 and 65.

The shift family: K - sigma_m I on the 24 x 24 grid Laplacian for sigma_m at midpoints between consecutive distinct eigenvalues
of K, only where the gap is at least 1e-3 -- a shift sweep whose inertia is known beforehand: neg(K - sigma I) counts the
eigenvalues below sigma."""
import numpy as np

import _csx
import ldl_cases as LC
import ldl_oracle as LO
from chol_refactor_cases import grid_upper

LIMITS = _csx.ldl_batch_limits()
WAVES, THREADS, FETCH, MAX_MEMBERS = (LIMITS[k] for k in ("WALK_WAVES", "SOLVE_THREADS", "SOLVE_FETCH", "MAX_MEMBERS"))
RUN_WAVES, RUN_FETCH = LIMITS["RUN_WAVES"], LIMITS["RUN_FETCH"]

WIDE_SEED = 20250611
B_SIZES = (1, 2, 3, 65)
R_SIZES = (1, 3)
WAVE_SHAPES = ((64, 1), (65, 1))                                   # (B, r) with B r = 64, 65
WIDE_EDGE_B = (THREADS // (WAVES + 1), THREADS // (WAVES + 1) + 1)   # r = 1 on chains5
RUN_EDGE_R = (RUN_WAVES // WAVES, RUN_WAVES // WAVES + 1)          # B = 2 on chains4
FETCH_CASES = ("grid24-shift", "update-batches")
RUN_FETCH_CASES = ("long-column", "long-column-updated")
CPU_SWEEP_CASES = ("chain", "grid24-shift", "dups", "kkt-sqd")
LAUNCH_CASES = ("chain", "chains4", "chains5", "grid24-shift")


def member(case, m):
    """the values of member m of a batch on `case`"""
    return case.values(LC.VALUE_SETS[m]) if m < len(LC.VALUE_SETS) else case.congruent(WIDE_SEED + m)


def members(case, B):
    """nnz x B: column m = member(case, m)"""
    return np.ascontiguousarray(np.stack([member(case, m) for m in range(B)], axis=1))


def levels_of(case):
    """the columns by height level of the elimination tree (csx_levelwalk.h's height_levels): a leaf at 0, a column one above its
    highest child; ascending inside a level"""
    parent = LO.pattern_of(case)[2]
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
    Lp, Li, _ = LO.pattern_of(case)
    rows = [[] for _ in range(case.n)]
    for k in range(case.n):
        for q in range(Lp[k], Lp[k + 1]):
            rows[Li[q]].append((k, q))
    return rows


def chain_lengths(case, wide):
    """({terms of a row's chain}, {terms of a column's chain}) over the columns of the wide levels (more than WALK_WAVES columns:
    a thread a chain) or of the narrow ones (a walker's wave a chain)"""
    Lp, rows = LO.pattern_of(case)[0], row_view(case)
    js = [j for cols in levels_of(case) if (len(cols) > WAVES) == wide for j in cols]
    return {len(rows[j]) - 1 for j in js}, {Lp[j + 1] - Lp[j] - 1 for j in js}


def level_sweeps(case, Lx, d, b):
    """The two sweeps of csx_ldl_batch_solve between the permutations, restated in plain Python floats (every product, difference
    and quotient rounded on its own), level by level as the device runs them:
      ascending levels, row gather:    x_j = ((x_j - l1 x_k1) - l2 x_k2) - ... over row j's entries off the diagonal, k ascending
      descending levels, column dot:   s = x_j / d_j FIRST, then ((s - l1 x_i1) - l2 x_i2) - ... over column j's stored entries
                                       below the diagonal, in storage order
    There is no pass of its own for D."""
    Lp, Li, _ = LO.pattern_of(case)
    levels, rows = levels_of(case), row_view(case)
    x = [float(v) for v in b]
    for cols in levels:
        for j in cols:
            s = x[j]
            for k, at in rows[j][:-1]:
                t = float(Lx[at]) * x[k]
                s = s - t
            x[j] = s
    for cols in reversed(levels):
        for j in cols:
            s = LO._div(x[j], float(d[j]))
            for q in range(Lp[j] + 1, Lp[j + 1]):
                t = float(Lx[q]) * x[Li[q]]
                s = s - t
            x[j] = s
    return x


def reference_sweeps(O, case, Lx, d, b):
    """cs_lsolve(L), the elementwise division by d, cs_ltsolve(L) of the restated reference O: the single solver's three steps"""
    Lp, Li, _ = LO.pattern_of(case)
    L = O.cs_spalloc(case.n, case.n, max(len(Li), 1), True, False)
    L.p, L.i, L.x = list(Lp), list(Li), [float(v) for v in Lx]
    x = [float(v) for v in b]
    assert O.cs_lsolve(L, x)
    x = [LO._div(x[j], float(d[j])) for j in range(case.n)]
    assert O.cs_ltsolve(L, x)
    return x


# ---- the shift family ------------------------------------------------------------------------------------------------------------

SHIFT_GRID, SHIFT_GAP = 24, 1e-3
_SHIFT = {}


def shift_family():
    """(case, sigmas, counts, V): the LDL' case of K = grid_upper(24) at order 1 (its own values are K - sigmas[0] I), the shifts
    at the midpoints of the gaps >= SHIFT_GAP between consecutive distinct eigenvalues of K, counts[m] = the eigenvalues of K
    below sigmas[m], and V (nnz x len(sigmas)) with column m the values of K - sigmas[m] I.  Computed once."""
    if not _SHIFT:
        n, p, i, x = grid_upper(SHIFT_GRID)
        K = LC.Case("shift-family-K", n, p, i, x, order=1, seed=17)
        ev = np.linalg.eigvalsh(K.dense())
        sig, cnt = [], []
        for a, b in zip(ev[:-1], ev[1:]):
            if b - a >= SHIFT_GAP:
                s = 0.5 * (a + b)
                sig.append(float(s))
                cnt.append(int(np.sum(ev < s)))
        diag = np.asarray(K.i) == K.cols
        V = np.repeat(K.x[:, None], len(sig), axis=1)
        V[diag, :] -= np.asarray(sig)[None, :]
        case = LC.Case("shift-family", n, p, i, V[:, 0].copy(), order=1, seed=17)
        _SHIFT["v"] = (case, sig, cnt, np.ascontiguousarray(V))
    return _SHIFT["v"]
