"""Inputs shared by the tests of hqrsol_factor(...).batch(), on the cases of tests/hqr_cases.py and the rule of
tests/hqr_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT.

Members: the first three of every case are its value sets "A", A2[0], A2[1] (the ones tests/hqr_oracle.reference caches); a wider
batch goes on with case.scaled(WIDE_SEED + m), new values on the pattern from seeds nobody else uses.

Sizes: B members and r right-hand sides a member, on both sides of every constant of _csx.hqr_batch_limits():
  WALK_WAVES     a level of that many columns goes to the walker, one more to the level kernel: the cases chains4 / chains5
  SOLVE_THREADS  (row, column) pairs a solve workgroup of a wide level takes: K = B r columns of X at SOLVE_THREADS - 1, exactly
                 SOLVE_THREADS and one more (THREAD_SHAPES), on chains5 (every level wide) and the two walker cases
  RUN_WAVES      (row, right-hand side) pairs a solve walker takes at a time: a walker level of chains4 (WALK_WAVES rows) with
                 RUN_EDGE_R right-hand sides is exactly one pass / the first with two, and one column of long-column-updated with
                 RUN_WAVES - 1, RUN_WAVES, RUN_WAVES + 1 right-hand sides (RUN_SHAPES)
  HAPPLY_LANES   columns of X a workgroup of the batched reflection kernels takes, a lane each: K = 64 and 65 (WAVE_SHAPES)
  HAPPLY_MAX_LEVELS  csx_happly's rule for the one-launch route: as many reflection levels as reflections (bidiagonal, where
                 every reflection shares a row with the one before) takes it, blocks (two levels of 300) does not
  MAX_MEMBERS    the most members of a batch: on the case `one` (one entry) at the limit, refused one above

The restated solve (level_solve): what csx_hqr_batch_solve runs between its permutations, in plain Python floats (every product,
sum, difference and quotient rounded on its own) --
  the reflections by house level (level[k] = 1 + the highest level of an earlier reflection that shares a row with k), inside a
    level in any order, each by cs_happly's loops;
  cs_usolve as a row gather over the height levels of the column elimination tree from the top down: row i takes the entries
    R(i, j), j > i, j DESCENDING, then the division by R(i, i), the last stored entry of column i;
  cs_utsolve as a dot over column j's entries before the diagonal in storage order, levels ascending."""
import numpy as np

import _csx
import hqr_cases as HC
import hqr_oracle as HO

LIMITS = _csx.hqr_batch_limits()
WAVES, THREADS, FETCH, MAX_MEMBERS = (LIMITS[k] for k in ("WALK_WAVES", "SOLVE_THREADS", "SOLVE_FETCH", "MAX_MEMBERS"))
RUN_WAVES, RUN_FETCH, LANES, MAX_LEVELS = (LIMITS[k] for k in ("RUN_WAVES", "RUN_FETCH", "HAPPLY_LANES", "HAPPLY_MAX_LEVELS"))

WIDE_SEED = 20250801
R_SIZES = (1, 3)
WAVE_SHAPES = ((LANES, 1), (LANES + 1, 1))                               # (B, r) with B r = 64, 65
THREAD_SHAPES = ((THREADS - 1, 1), (THREADS // 2, 2), (THREADS + 1, 1))  # B r = SOLVE_THREADS - 1, SOLVE_THREADS, + 1
RUN_EDGE_R = (RUN_WAVES // WAVES, RUN_WAVES // WAVES + 1)                # B = 2 on chains4
RUN_SHAPES = ((1, RUN_WAVES - 1), (1, RUN_WAVES), (1, RUN_WAVES + 1))    # one member's columns of one row against the waves
EDGE_CASES = ("chains4", "chains5", "long-column-updated")
LAUNCH_CASES = ("bidiagonal", "chains4", "chains5", "grid24-shift")
CPU_SOLVE_CASES = ("dense65", "bidiagonal", "chains5", "west-nd", "ash219", "lp_afiro")


def member(case, m):
    """the values of member m of a batch on `case` (A's storage order)"""
    return case.values(HC.VALUE_SETS[m]) if m < len(HC.VALUE_SETS) else case.scaled(WIDE_SEED + m)


def members(case, B):
    """nnz x B: column m = member(case, m)"""
    return np.ascontiguousarray(np.stack([member(case, m) for m in range(B)], axis=1))


def levels_of(S):
    """the columns by height level of the column elimination tree S.parent (csx_levelwalk.h's height_levels): a leaf at 0, a
    column one above its highest child; ascending inside a level"""
    parent, n = S.parent.tolist(), S.n
    level = [0] * n
    for j in range(n):
        if parent[j] >= 0:
            level[parent[j]] = max(level[parent[j]], level[j] + 1)
    out = [[] for _ in range(max(level) + 1 if n else 0)]
    for j in range(n):
        out[level[j]].append(j)
    return out


def level_of_column(S):
    out = [0] * S.n
    for l, cols in enumerate(levels_of(S)):
        for j in cols:
            out[j] = l
    return out


def house_levels(Vp, Vi, m2):
    """the reflections by level (csx_qr.hip's house_levels): reflections of one level touch disjoint rows"""
    n = len(Vp) - 1
    rowlev, level = [0] * m2, [0] * n
    for k in range(n):
        rows = [Vi[p] for p in range(Vp[k], Vp[k + 1])]
        level[k] = max([rowlev[i] for i in rows] or [0])
        for i in rows:
            rowlev[i] = level[k] + 1
    out = [[] for _ in range(max(level) + 1 if n else 0)]
    for k in range(n):
        out[level[k]].append(k)
    return out


def row_view(Rp, Ri, n, descending=True):
    """row i of R's pattern: [(j, slot of (i, j))] with the columns descending, so the diagonal last -- or, the mistake, the
    columns off the diagonal ascending and then the diagonal"""
    rows = [[] for _ in range(n)]
    for j in range(n):
        for q in range(Rp[j], Rp[j + 1]):
            rows[Ri[q]].append((j, q))
    return [list(reversed(r)) if descending else r[1:] + r[:1] for r in rows]


def apply_levels(Vp, Vi, Vx, beta, x, transpose, m2):
    """Q' x (transpose: house levels ascending) or Q x (descending), every reflection by cs_happly's loops"""
    levels = house_levels(Vp, Vi, m2)
    for cols in (levels if transpose else reversed(levels)):
        for k in (cols if transpose else reversed(cols)):
            tau = 0.0
            for p in range(Vp[k], Vp[k + 1]):
                prod = Vx[p] * x[Vi[p]]
                tau = tau + prod
            tau = tau * beta[k]
            for p in range(Vp[k], Vp[k + 1]):
                prod = Vx[p] * tau
                x[Vi[p]] = x[Vi[p]] - prod
    return x


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def usolve_levels(levels, rows, Rp, Rx, x):
    """R \\ x: the levels from the top down, a row gather, the diagonal last"""
    for cols in reversed(levels):
        for i in cols:
            s = x[i]
            for j, at in rows[i][:-1]:
                t = Rx[at] * x[j]
                s = s - t
            x[i] = _div(s, Rx[Rp[i + 1] - 1])
    return x


def utsolve_levels(levels, Rp, Ri, Rx, x):
    """R' \\ x: the levels ascending, a dot over the column's entries before the diagonal"""
    for cols in levels:
        for j in cols:
            s = x[j]
            for q in range(Rp[j], Rp[j + 1] - 1):
                t = Rx[q] * x[Ri[q]]
                s = s - t
            x[j] = _div(s, Rx[Rp[j + 1] - 1])
    return x


def level_solve(S, factors, b, second=False, descending=True):
    """csx_hqr_batch_solve of one column restated: first sequence (b of S.m entries -> S.n) or second (S.n -> S.m) on the factors
    (Vp, Vi, Vx, Rp, Ri, Rx, beta) of the factored matrix"""
    Vp, Vi, Vx, Rp, Ri, Rx, beta = (np.asarray(a).tolist() for a in factors)
    m, n = S.m, S.n
    q = list(range(n)) if S.q is None else [int(v) for v in S.q]
    pinv = [int(v) for v in S.pinv[:m]]
    levels, rows = levels_of(S), row_view(Rp, Ri, n, descending)
    w = [0.0] * S.m2
    b = [float(v) for v in b]
    if not second:
        for i in range(m):
            w[pinv[i]] = b[i]
        apply_levels(Vp, Vi, Vx, beta, w, True, S.m2)
        usolve_levels(levels, rows, Rp, Rx, w)
        out = [0.0] * n
        for k in range(n):
            out[q[k]] = w[k]
        return np.asarray(out)
    for k in range(n):
        w[k] = b[q[k]]
    utsolve_levels(levels, Rp, Ri, Rx, w)
    apply_levels(Vp, Vi, Vx, beta, w, False, S.m2)
    return np.asarray([w[pinv[i]] for i in range(m)])


def reference_solve(O, S, factors, b, second=False):
    """the reference's sequence on the same factors by the restated reference O (csparse_oracle): cs_ipvec, cs_happly
    k = 0 .. n - 1, cs_usolve, cs_ipvec; or cs_pvec, cs_utsolve, cs_happly k = n - 1 .. 0, cs_pvec"""
    Vp, Vi, Vx, Rp, Ri, Rx, beta = (np.asarray(a).tolist() for a in factors)
    m, n = S.m, S.n
    V, R = O.cs_spalloc(S.m2, n, max(len(Vi), 1), True, False), O.cs_spalloc(n, n, max(len(Ri), 1), True, False)
    V.p, V.i, V.x = Vp, Vi or [0], Vx or [0.0]
    R.p, R.i, R.x = Rp, Ri or [0], Rx or [0.0]
    q = None if S.q is None else [int(v) for v in S.q]
    pinv = [int(v) for v in S.pinv[:m]]
    x = [0.0] * S.m2
    b = [float(v) for v in b]
    with np.errstate(divide="ignore", invalid="ignore"):
        if not second:
            assert O.cs_ipvec(pinv, b, x, m)
            for k in range(n):
                assert O.cs_happly(V, k, beta[k], x)
            assert O.cs_usolve(R, x)
            out = [0.0] * n
            assert O.cs_ipvec(q, x, out, n)
            return np.asarray(out)
        assert O.cs_pvec(q, b, x, n)
        assert O.cs_utsolve(R, x)
        for k in range(n - 1, -1, -1):
            assert O.cs_happly(V, k, beta[k], x)
        out = [0.0] * m
        assert O.cs_pvec(pinv, x, out, m)
        return np.asarray(out)
