"""ldlsol_factor(...).batch() without a device: the limits the implementation is cut by are readable and the size
table of tests/ldl_batch_cases.py sits on their edges; the rule the GPU test relies on -- the two sweeps of a batched solve, run
level by level as a row gather and a column dot with the division by D opening each backward chain, give the bytes of the
reference's cs_lsolve, elementwise division, cs_ltsolve; and the shift family's inertia under the host rule is the eigenvalue
count it is built to have."""
import numpy as np
import pytest

import ldl_batch_cases as BC
import ldl_cases as LC
import ldl_oracle as LO


def test_limits_are_readable_and_the_table_sits_on_their_edges():
    import _csx
    lim = _csx.ldl_batch_limits()
    assert sorted(lim) == sorted(_csx.SLU_BATCH_LIMITS) and all(isinstance(v, int) and v >= 1 for v in lim.values())
    assert lim == BC.LIMITS == _csx.slu_batch_limits()          # one level walk, one set of sweeps
    assert _csx.load().csx_ldl_batch_limits(None) == _csx.EINVAL
    waves, threads, fetch, run_fetch = lim["WALK_WAVES"], lim["SOLVE_THREADS"], lim["SOLVE_FETCH"], lim["RUN_FETCH"]
    # the walker's width: a case whose every level is exactly that wide, and one with one column more
    for name, width in (("chains4", waves), ("chains5", waves + 1)):
        assert {len(c) for c in BC.levels_of(LC.BY_NAME[name])} == {width}
    # a workgroup of a wide level: (rows of the level) x B x r on both sides of its threads
    lo, hi = BC.WIDE_EDGE_B
    assert hi == lo + 1 and (waves + 1) * lo <= threads < (waves + 1) * hi
    # one pass of a walker: (rows of the level) x r exactly its waves, and one more right-hand side
    lo, hi = BC.RUN_EDGE_R
    assert hi == lo + 1 and lo >= 1 and waves * lo == lim["RUN_WAVES"] < waves * hi
    # the terms a thread of a wide level fetches together: on the grid, rows and columns with one term fewer, exactly as many,
    # one more and more than twice as many; on the stars, rows at the second and the fourth fetch boundary (and no column beyond
    # one term: a leaf's column is its hub's row alone)
    rows, cols = BC.chain_lengths(LC.BY_NAME["grid24-shift"], True)
    for have in (rows, cols):
        assert {fetch - 1, fetch, fetch + 1} <= have and max(have) > 2 * fetch
    rows, cols = BC.chain_lengths(LC.BY_NAME["update-batches"], True)
    assert {2 * fetch - 1, 2 * fetch, 2 * fetch + 1, 4 * fetch, 4 * fetch + 1} <= rows and cols == {0, 1}
    assert set(BC.FETCH_CASES) == {"grid24-shift", "update-batches"}
    # ... and a wave of a walker: the dense triangles, every level one column
    for name in BC.RUN_FETCH_CASES:
        assert {len(c) for c in BC.levels_of(LC.BY_NAME[name])} == {1}
        for have in BC.chain_lengths(LC.BY_NAME[name], False):
            assert {run_fetch - 1, run_fetch, run_fetch + 1} <= have and max(have) > 2 * run_fetch, name
        assert BC.chain_lengths(LC.BY_NAME[name], True) == (set(), set())
    # the issue's sizes
    assert set(BC.B_SIZES) >= {1, 2, 3, 65} and set(BC.R_SIZES) >= {1, 3}
    assert sorted(b * r for b, r in BC.WAVE_SHAPES) == [64, 65]
    assert lim["MAX_MEMBERS"] == BC.MAX_MEMBERS >= max(BC.B_SIZES)


def test_members_are_the_cached_value_sets_then_new_ones():
    case = LC.BY_NAME["grid24-shift"]
    V = BC.members(case, 5)
    assert V.shape == (len(case.x), 5) and V.flags["C_CONTIGUOUS"]
    for m, which in enumerate(LC.VALUE_SETS):
        assert V[:, m].tobytes() == case.values(which).tobytes()
    assert V[:, 3].tobytes() != V[:, 4].tobytes() and V[:, 3].tobytes() == BC.member(case, 3).tobytes()
    assert BC.WIDE_SEED > 100 * (len(LC.CASES) + 2) + 2          # Case.A2's seeds are (1 .. cases) * 100 + 1, 2: far below


@pytest.mark.parametrize("name", BC.CPU_SWEEP_CASES)
def test_level_sweeps_are_the_reference_loops(name):
    import csparse_oracle as O
    case = LC.BY_NAME[name]
    assert len(BC.levels_of(case)) > 1
    for which in LC.VALUE_SETS:
        Lx, d, _ = LO.reference(case, which)
        for b in LC.rhs(case, 2):
            got = BC.level_sweeps(case, Lx, d, b)
            ref = BC.reference_sweeps(O, case, Lx, d, b)
            assert np.asarray(got).tobytes() == np.asarray(ref).tobytes(), which
            assert np.isfinite(got).all() and np.asarray(got).tobytes() != np.asarray(b).tobytes()


def test_dividing_at_the_end_of_the_forward_sweep_is_another_solve():
    """the mistake the fused step must not make: x_j / d_j as row j's forward chain closes, where later rows still read x_j"""
    case = LC.BY_NAME["grid24-shift"]
    Lx, d, _ = LO.reference(case, "A")
    Lp, Li, _ = LO.pattern_of(case)
    rows = BC.row_view(case)
    b = LC.rhs(case, 1)[0]
    x = [float(v) for v in b]
    for cols in BC.levels_of(case):
        for j in cols:
            s = x[j]
            for k, at in rows[j][:-1]:
                s = s - float(Lx[at]) * x[k]
            x[j] = s / float(d[j])
    for cols in reversed(BC.levels_of(case)):
        for j in cols:
            s = x[j]
            for q in range(Lp[j] + 1, Lp[j + 1]):
                s = s - float(Lx[q]) * x[Li[q]]
            x[j] = s
    right = np.asarray(BC.level_sweeps(case, Lx, d, b))
    assert not np.allclose(np.asarray(x), right, rtol=1e-6, atol=0.0)


def test_the_shift_family_counts_eigenvalues_under_the_host_rule():
    case, sigmas, counts, V = BC.shift_family()
    assert len(sigmas) >= 65 and V.shape == (len(case.x), len(sigmas)) and counts == sorted(counts)
    assert 0 < counts[0] and counts[-1] < case.n and len(set(counts)) == len(counts)
    assert V[:, 0].tobytes() == case.x.tobytes()
    for m in range(len(sigmas)):
        st, _, d, (pos, neg, perturbed, broke) = LO.host(case, V[:, m], 0.0)
        assert st == 0 and broke == -1 and perturbed == 0, m
        assert (pos, neg) == (case.n - counts[m], counts[m]), (m, sigmas[m])
