"""The inputs of the Cholesky-refactor tests (tests/chol_refactor_cases.py) held to their assumptions, without a device: every
A2 is positive definite and the marked one is not (the oracle's cs_chol says so), and the geometry a case is built for -- the
size against the small-tree limit, the band of the natural-order factor, a supernode in the ordered 24 x 24 grid, duplicates and
lower entries -- is there."""
import numpy as np
import pytest

import csparse_oracle as O
import chol_refactor_cases as RC

CH_SMALL_TREE = 512     # csx_chol.hip: trees up to this many columns go to the tree kernel
SN_MIN_WIDTH = 8        # ... supernodes of at least this many columns are factored as dense trapezoids
CLIQUE_MAX_BLOCK = 64   # csx_cholclique.h


def _pinv(case):
    if case.order == 0:
        return None
    import csparse as cs
    perm = cs.cs_amd(1, case.matrix(cs))
    assert sorted(perm) == list(range(case.n))
    pinv = [0] * case.n
    for k, v in enumerate(perm):
        pinv[v] = k
    return pinv


@pytest.mark.parametrize("name", RC.NAMES)
def test_values_share_the_pattern_and_are_spd(name):
    case = RC.BY_NAME[name]
    nnz = int(case.p[case.n])
    assert len(case.i) == nnz == len(case.x) == len(case.bad)
    assert len(case.A2) == 2 and all(len(x2) == nnz for x2 in case.A2)   # value sets on A's own p / i: identical by construction
    assert all(x2.tobytes() != case.x.tobytes() for x2 in case.A2) and case.A2[0].tobytes() != case.A2[1].tobytes()
    S = RC.oracle_symbolic(O, case, _pinv(case))
    for which in ("A", 0, 1):
        assert RC.oracle_factor(O, case, which, S) is not None, which
    assert RC.oracle_factor(O, case, "bad", S) is None
    # what the oracle factored is the effective upper triangle (of duplicates the last, lower entries ignored)
    Lp, Li, Lx = RC.oracle_factor(O, case, 0, S)
    L = np.zeros((case.n, case.n))
    L[Li, np.repeat(np.arange(case.n), np.diff(Lp))] = Lx
    U = case.effective_upper(case.A2[0])
    full = U + np.triu(U, 1).T
    if S.pinv is not None:
        perm = np.argsort(np.asarray(S.pinv))
        full = full[np.ix_(perm, perm)]
    assert np.max(np.abs(L @ L.T - full)) <= 1e-12 * np.max(np.abs(full))


def _natural_factor(case):
    S = RC.oracle_symbolic(O, case, None)
    return S, RC.oracle_factor(O, case, "A", S)


def test_small_tree_limit():
    assert RC.BY_NAME["grid22"].n == 484 <= CH_SMALL_TREE < RC.BY_NAME["grid24"].n == 576
    assert RC.BY_NAME["bcsstk01-natural"].n == 48 and RC.BY_NAME["one"].n == 1 and RC.BY_NAME["diagonal"].n == 70


def test_grid24_natural_is_a_full_narrow_band_on_a_chain():
    case = RC.BY_NAME["grid24nat"]
    S, (Lp, Li, Lx) = _natural_factor(case)
    n = case.n
    assert S.parent == list(range(1, n)) + [-1]                     # a chain: as many levels as columns
    hb = max(int(Li[Lp[j + 1] - 1]) - j for j in range(n))
    assert hb == 24 and hb + 1 <= 48                                # the narrowest register window takes it
    assert Lp[n] >= 0.5 * n * (hb + 1)                              # mostly full: the blocked dense band may take it ("chol.wband" = 2)


def test_grid24_ordered_has_a_supernode():
    case = RC.BY_NAME["grid24"]
    S = RC.oracle_symbolic(O, case, _pinv(case))
    n, parent, cp = case.n, S.parent, S.cp
    nchild = [0] * n
    for j in range(n):
        if parent[j] >= 0:
            nchild[parent[j]] += 1
    best, j = 0, 0
    while j < n:                                                    # chol_device's rule
        a = j
        while j + 1 < n and parent[j] == j + 1 and nchild[j + 1] == 1 and cp[j + 2] - cp[j + 1] == cp[j + 1] - cp[j] - 1:
            j += 1
        best = max(best, j - a + 1)
        j += 1
    assert best >= SN_MIN_WIDTH
    # one tree, too big for the tree kernel: level lists
    assert sum(1 for v in parent if v < 0) == 1


def test_grid22_ordered_is_one_small_sparse_tree():
    case = RC.BY_NAME["grid22"]
    S = RC.oracle_symbolic(O, case, _pinv(case))
    assert sum(1 for v in S.parent if v < 0) == 1
    assert S.cp[case.n] < case.n * (case.n + 1) // 2               # not a dense block


def test_dups_has_duplicates_and_a_lower_triangle():
    case, plain = RC.BY_NAME["dups"], RC.BY_NAME["grid24"]
    upper = case.i <= case.cols
    assert int(np.sum(~upper)) == int(plain.p[plain.n]) - plain.n   # the whole strict lower triangle
    keys = case.cols[upper] * case.n + case.i[upper]
    assert len(keys) - len(np.unique(keys)) == (int(plain.p[plain.n]) + 4) // 5
    # last wins: the effective matrix is the plain grid's
    P = plain.effective_upper()
    assert np.array_equal(case.effective_upper(), P)
    # ... and the lower values are not the mirror of the upper ones
    assert np.min(case.x[~upper]) >= 20.0


def test_forest_cases_are_blocks_of_at_most_64_consecutive_columns():
    for name in ("cliques16-exact", "ragged", "sparse_trees"):
        case = RC.BY_NAME[name]
        S, (Lp, Li, Lx) = _natural_factor(case)
        roots = [j for j in range(case.n) if S.parent[j] < 0]
        starts = [0] + [r + 1 for r in roots[:-1]]
        assert all(S.parent[j] == j + 1 for j in range(case.n) if j not in set(roots)), name   # consecutive columns
        assert max(r - s + 1 for r, s in zip(roots, starts)) <= CLIQUE_MAX_BLOCK, name
        dense = all(Lp[j + 1] - Lp[j] == roots[np.searchsorted(roots, j)] - j + 1 for j in range(case.n))
        assert dense == (name != "sparse_trees"), name
