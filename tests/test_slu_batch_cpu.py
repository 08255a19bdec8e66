"""slusol_factor(...).batch() without a device: the limits the implementation is cut by are readable and the size
table of tests/slu_batch_cases.py sits on their edges; and the rule the GPU test relies on -- the two sweeps of a batched solve,
run level by level as a row gather and a column dot, give the bytes of the reference's cs_lsolve / cs_ltsolve loops."""
import numpy as np
import pytest

import slu_batch_cases as BC
import slu_cases as SC
import slu_oracle as SO


def test_limits_are_readable_and_the_table_sits_on_their_edges():
    import _csx
    lim = _csx.slu_batch_limits()
    assert sorted(lim) == sorted(_csx.SLU_BATCH_LIMITS) and all(isinstance(v, int) and v >= 1 for v in lim.values())
    assert lim == BC.LIMITS
    waves, threads, fetch = lim["WALK_WAVES"], lim["SOLVE_THREADS"], lim["SOLVE_FETCH"]
    # the walker's width: a case whose every level is exactly that wide, and one with one column more
    for name, width in (("chains4", waves), ("chains5", waves + 1)):
        assert {len(c) for c in BC.levels_of(SC.BY_NAME[name])} == {width}
    # a workgroup of a wide level: (rows of the level) x B x r on both sides of its threads
    lo, hi = BC.WIDE_EDGE_B
    assert hi == lo + 1 and (waves + 1) * lo <= threads < (waves + 1) * hi
    # one pass of a walker: (rows of the level) x r exactly its waves, and one more right-hand side
    lo, hi = BC.RUN_EDGE_R
    assert hi == lo + 1 and lo >= 1 and waves * lo == lim["RUN_WAVES"] < waves * hi
    # the terms fetched together, by a thread of a wide level and by a wave of a walker: chains with one term fewer, exactly as
    # many, one more, and more than twice as many
    for names, wide, width in ((BC.FETCH_CASES, True, fetch), (BC.RUN_FETCH_CASES, False, lim["RUN_FETCH"])):
        for name in names:
            for have in BC.chain_lengths(SC.BY_NAME[name], wide):
                assert {width - 1, width, width + 1} <= have and max(have) > 2 * width, (name, wide)
    # the issue's sizes
    assert set(BC.B_SIZES) >= {1, 2, 3, 65} and set(BC.R_SIZES) >= {1, 3}
    assert sorted(b * r for b, r in BC.WAVE_SHAPES) == [64, 65]
    assert lim["MAX_MEMBERS"] == BC.MAX_MEMBERS >= max(BC.B_SIZES)


def test_members_are_the_cached_value_sets_then_new_ones():
    case = SC.BY_NAME["grid24-shift"]
    V = BC.members(case, 5)
    assert V.shape == (len(case.x), 5) and V.flags["C_CONTIGUOUS"]
    for m, which in enumerate(SC.VALUE_SETS):
        assert V[:, m].tobytes() == case.values(which).tobytes()
    assert V[:, 3].tobytes() != V[:, 4].tobytes() and V[:, 3].tobytes() == BC.member(case, 3).tobytes()


@pytest.mark.parametrize("name", BC.CPU_SWEEP_CASES)
def test_level_sweeps_are_the_reference_loops(name):
    import csparse_oracle as O
    case = SC.BY_NAME[name]
    Lx, Ux, _ = SO.reference(case, "A")
    assert len(BC.levels_of(case)) > 1
    for b in SC.rhs(case, 2):
        for trans in (False, True):
            got = BC.level_sweeps(case, Lx, Ux, b, trans)
            ref = BC.reference_sweeps(O, case, Lx, Ux, b, trans)
            assert np.asarray(got).tobytes() == np.asarray(ref).tobytes(), trans
            assert np.isfinite(got).all() and np.asarray(got).tobytes() != np.asarray(b).tobytes()
