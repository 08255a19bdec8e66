"""hqrsol_factor(...).batch() without a device: the limits the implementation is cut by are readable and the size
table of tests/hqr_batch_cases.py sits on their edges; the rule the GPU test relies on -- the batched solve restated level by
level (the reflections by house level, cs_usolve as a row gather with the columns descending from the top level down, cs_utsolve
as a column dot from the leaves up, the diagonal of R the last stored entry of its column) gives the bytes of the reference's
sequence on factors from csx_hqr_host; a row view with the columns ascending does not; and every nonzero R(i, j) has j on a
higher level of the column elimination tree than i, which is why the factor's own levels order both sweeps."""
import numpy as np
import pytest

import hqr_batch_cases as BC
import hqr_cases as HC
import hqr_oracle as HO


def test_limits_are_readable_and_the_table_sits_on_their_edges():
    import _csx
    lim = _csx.hqr_batch_limits()
    assert sorted(lim) == sorted(_csx.HQR_BATCH_LIMITS) and all(isinstance(v, int) and v >= 1 for v in lim.values())
    assert lim == BC.LIMITS
    assert {k: lim[k] for k in _csx.SLU_BATCH_LIMITS} == _csx.slu_batch_limits() == _csx.ldl_batch_limits()   # one walk, one set of sweeps
    assert _csx.load().csx_hqr_batch_limits(None) == _csx.EINVAL
    waves, threads, run_waves, lanes = lim["WALK_WAVES"], lim["SOLVE_THREADS"], lim["RUN_WAVES"], lim["HAPPLY_LANES"]
    # the walker's width: a case whose every level is exactly that wide, and one with one column more
    for name, width in (("chains4", waves), ("chains5", waves + 1)):
        assert {len(c) for c in BC.levels_of(HC.BY_NAME[name].analysis)} == {width}
    # the reflection kernel's lane chunk, the threads of a wide level's workgroup, the waves of a walker
    assert sorted(b * r for b, r in BC.WAVE_SHAPES) == [lanes, lanes + 1]
    assert sorted(b * r for b, r in BC.THREAD_SHAPES) == [threads - 1, threads, threads + 1]
    assert sorted(b * r for b, r in BC.RUN_SHAPES) == [run_waves - 1, run_waves, run_waves + 1]
    lo, hi = BC.RUN_EDGE_R
    assert hi == lo + 1 and lo >= 1 and waves * lo == run_waves < waves * hi
    assert set(BC.EDGE_CASES) == {"chains4", "chains5", "long-column-updated"} and set(BC.R_SIZES) >= {1, 3}
    # long-column-updated: two columns, each a level of its own (the walker), the second with one entry of R off the diagonal
    S = HC.BY_NAME["long-column-updated"].analysis
    assert [len(c) for c in BC.levels_of(S)] == [1, 1]
    # csx_happly's one-launch rule: as many reflection levels as reflections on the bidiagonal case, two levels on blocks
    for name, chain in (("bidiagonal", True), ("blocks", False), ("chains5", False)):
        case = HC.BY_NAME[name]
        Vp, Vi, _, _ = HO.pattern_of(case)
        nlev = len(BC.house_levels(Vp, Vi, case.analysis.m2))
        assert (nlev == case.analysis.n or nlev > lim["HAPPLY_MAX_LEVELS"]) is chain, name
    assert lim["MAX_MEMBERS"] == BC.MAX_MEMBERS >= 65 and set(BC.LAUNCH_CASES) == {"bidiagonal", "chains4", "chains5", "grid24-shift"}
    assert len(BC.levels_of(HC.BY_NAME["bidiagonal"].analysis)) == HC.RUN_LEVELS + 1 == 257


def test_members_are_the_cached_value_sets_then_new_ones():
    case = HC.BY_NAME["grid24-shift"]
    V = BC.members(case, 5)
    assert V.shape == (len(case.x), 5) and V.flags["C_CONTIGUOUS"]
    for m, which in enumerate(HC.VALUE_SETS):
        assert V[:, m].tobytes() == case.values(which).tobytes()
    assert V[:, 3].tobytes() != V[:, 4].tobytes() and V[:, 3].tobytes() == BC.member(case, 3).tobytes()
    assert V[:, 3].tobytes() == case.scaled(BC.WIDE_SEED + 3).tobytes()
    assert BC.WIDE_SEED > 100 * (len(HC.CASES) + 2) + 2          # Case.A2's seeds are (1 .. cases) * 100 + 1, 2: far below


@pytest.mark.parametrize("name", BC.CPU_SOLVE_CASES)
def test_the_level_solve_is_the_reference_sequence(name):
    import csparse_oracle as O
    case = HC.BY_NAME[name]
    S = case.analysis
    seconds = (False, True) if case.m == case.n else ((True,) if case.m < case.n else (False,))
    for which in HC.VALUE_SETS:
        factors = HO.reference(case, which)
        for second in seconds:
            rows_in = S.n if second else S.m
            for b in HC.rhs(case, 2, rows_in):
                got = BC.level_solve(S, factors, b, second)
                ref = BC.reference_solve(O, S, factors, b, second)
                assert got.tobytes() == ref.tobytes(), (which, second)
                assert np.isfinite(got).all() and len(got) == (S.m if second else S.n)
    # both sequences are exercised over the cases, and both kinds of level
    assert name != "lp_afiro" or seconds == (True,)
    assert name != "west-nd" or seconds == (False, True)


def test_a_row_view_with_the_columns_ascending_is_another_solve():
    """the mistake the row gather must not make: R(i, j) x_j subtracted in ascending j, where cs_usolve reaches row i from the
    last column down"""
    case = HC.BY_NAME["west-nd"]
    S, factors = case.analysis, HO.reference(case, "A")
    b = HC.rhs(case, 1)[0]
    right = BC.level_solve(S, factors, b)
    wrong = BC.level_solve(S, factors, b, descending=False)
    assert np.isfinite(wrong).all() and right.tobytes() != wrong.tobytes()
    assert np.allclose(right, wrong, rtol=1e-6, atol=0.0)        # the same solve in exact arithmetic: another rounding


@pytest.mark.parametrize("name", HC.NAMES)
def test_every_entry_of_r_points_up_the_tree(name):
    case = HC.BY_NAME[name]
    S = case.analysis
    _, _, Rp, Ri = HO.pattern_of(case)
    level = BC.level_of_column(S)
    for j in range(S.n):
        assert Ri[Rp[j + 1] - 1] == j                            # the diagonal is the last stored entry of its column
        for q in range(Rp[j], Rp[j + 1] - 1):
            assert Ri[q] < j and level[j] > level[Ri[q]], (name, j, Ri[q])
    rows = BC.row_view(Rp, Ri, S.n)
    for i in range(S.n):
        cols = [j for j, _ in rows[i]]
        assert cols == sorted(cols, reverse=True) and cols[-1] == i and rows[i][-1][1] == Rp[i + 1] - 1
