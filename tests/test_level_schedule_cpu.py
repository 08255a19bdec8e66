"""csx_level_schedule (the launches of the level walk of ldlsol / schur / slusol / hqrsol_factor, DESIGN.md §22 "The level walk")
against a model of the rule written from that paragraph: every case must give the model's launches, cover every level exactly
once and in order, and keep wide levels out of the walker.  The caps are arguments, so the work cut -- which the QR factor takes
at 2^24 slot updates and no test matrix reaches -- is cut here at a handful.  No device."""
import numpy as np
import pytest

import _csx

WAVES, CAP, UNCAPPED = 4, 256, 2 ** 31 - 1


def model(widths, waves, run_levels, work=None, run_work=0):
    """a level of more than `waves` columns is a launch of its own; otherwise a walker launch starts here, always
    takes this level, and takes the following narrow levels until it holds run_levels of them or the next one would take the
    sum of the work figures past run_work"""
    out, l, n = [], 0, len(widths)
    while l < n:
        if widths[l] > waves:
            out.append((True, l, l + 1))
            l += 1
            continue
        end, total = l + 1, 0 if work is None else work[l]
        while end < n and widths[end] <= waves and end - l < run_levels:
            if work is not None:
                if total + work[end] > run_work:
                    break
                total += work[end]
            end += 1
        out.append((False, l, end))
        l = end
    return out


def schedule(widths, waves=WAVES, run_levels=CAP, work=None, run_work=0):
    ptr = np.concatenate([[0], np.cumsum(widths)]).astype(np.int32)
    got = _csx.level_schedule(ptr, waves, run_levels, work, run_work)
    # every level exactly once, in order; a wide launch is one level; no walker launch holds a level wider than the wave count
    at = 0
    for wide, l0, l1 in got:
        assert l0 == at and l1 > l0
        assert (l1 == l0 + 1 and widths[l0] > waves) if wide else all(w <= waves for w in widths[l0:l1])
        at = l1
    assert at == len(widths)
    assert got == model(list(widths), waves, run_levels, None if work is None else list(work), run_work)
    return got


def test_no_levels_and_one_level():
    assert schedule([]) == []
    assert schedule([1]) == [(False, 0, 1)]
    assert schedule([4]) == [(False, 0, 1)]          # four columns: the walker still
    assert schedule([5]) == [(True, 0, 1)]           # five: a wave per column
    assert schedule([0]) == [(False, 0, 1)]          # (an empty level is narrow)


def test_widths_at_the_wave_count():
    assert schedule([4, 4, 4]) == [(False, 0, 3)]
    assert schedule([5, 5, 5]) == [(True, 0, 1), (True, 1, 2), (True, 2, 3)]
    assert schedule([5, 4, 4]) == [(True, 0, 1), (False, 1, 3)]
    assert schedule([2, 2], waves=1) == [(True, 0, 1), (True, 1, 2)]


@pytest.mark.parametrize("run,launches", [(255, 1), (256, 1), (257, 2), (512, 2), (513, 3)])
def test_a_wide_prefix_then_a_narrow_run(run, launches):
    widths = [300, 17, 5] + [4, 3, 1] * (run // 3) + [2] * (run % 3)
    got = schedule(widths)
    assert [g[0] for g in got] == [True] * 3 + [False] * launches
    assert [g[2] - g[1] for g in got[3:]] == [CAP] * (launches - 1) + [run - CAP * (launches - 1)]
    # uncapped: the whole run is one launch
    assert schedule(widths, run_levels=UNCAPPED) == [(True, 0, 1), (True, 1, 2), (True, 2, 3), (False, 3, 3 + run)]


def test_the_work_cut():
    w = [3, 3, 4, 1, 1, 1]
    assert schedule([1] * 6, work=w, run_work=10) == [(False, 0, 3), (False, 3, 6)]        # 3 + 3 + 4: exactly the cap
    assert schedule([1] * 6, work=w, run_work=9) == [(False, 0, 2), (False, 2, 6)]         # ... one over it
    assert schedule([1] * 6, work=w, run_work=2) == [(False, l, l + 1) for l in range(3)] + [(False, 3, 5), (False, 5, 6)]
    # a first level that alone exceeds the cap is still taken, alone
    assert schedule([2, 2, 2], work=[50, 1, 1], run_work=10) == [(False, 0, 1), (False, 1, 3)]
    assert schedule([2, 2, 2], work=[1, 50, 1], run_work=10) == [(False, 0, 1), (False, 1, 2), (False, 2, 3)]
    # a work cut and a level cut on the same level: one cut, not two
    assert schedule([1] * 5, run_levels=3, work=[2, 2, 2, 5, 1], run_work=6) == [(False, 0, 3), (False, 3, 5)]
    # the work figure of a wide level does not count, and a wide level restarts the sum
    assert schedule([1, 9, 1, 1], work=[6, 1000, 6, 4], run_work=10) == [(False, 0, 1), (True, 1, 2), (False, 2, 4)]
    # no work figures: no cut
    assert schedule([1] * 6, run_work=0) == [(False, 0, 6)]


def test_widths_need_not_shrink_with_height():
    """a real tree's levels never grow with height (every column has a child one level down); the rule does not rely on it"""
    widths = [2, 9, 1, 1, 7, 3, 4, 5, 0, 6]
    assert schedule(widths) == [(False, 0, 1), (True, 1, 2), (False, 2, 4), (True, 4, 5), (False, 5, 7), (True, 7, 8),
                                (False, 8, 9), (True, 9, 10)]
    assert schedule(widths, run_levels=1)[2:4] == [(False, 2, 3), (False, 3, 4)]


def test_random_widths_are_the_model():
    rng = np.random.default_rng(20241101)
    for _ in range(50):
        n = int(rng.integers(0, 40))
        widths = rng.integers(0, 9, n).tolist()
        work = rng.integers(0, 12, n).tolist()
        schedule(widths, run_levels=int(rng.integers(1, 6)))
        schedule(widths, run_levels=int(rng.integers(1, 6)), work=work, run_work=int(rng.integers(0, 30)))


def test_bad_arguments():
    lib, C = _csx.load(), _csx.C
    ptr, out, count = _csx.i32([0, 1, 3]), np.zeros(6, np.int32), C.c_int32(0)

    def call(nlev=2, p=ptr, waves=WAVES, run_levels=CAP, o=out, c=count):
        return lib.csx_level_schedule(nlev, _csx.pi(p), waves, run_levels, None, 0, _csx.pi(o), None if c is None else C.byref(c))

    assert call() == _csx.OK and count.value == 1
    assert call(nlev=-1) == _csx.EINVAL and call(p=None) == _csx.EINVAL and call(o=None) == _csx.EINVAL and call(c=None) == _csx.EINVAL
    assert call(waves=0) == _csx.EINVAL and call(run_levels=0) == _csx.EINVAL
    assert call(p=_csx.i32([0, 3, 1])) == _csx.EINVAL            # offsets that decrease
    assert call(nlev=0, o=None) == _csx.OK and count.value == 0
