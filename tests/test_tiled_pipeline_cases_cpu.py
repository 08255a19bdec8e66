"""The inputs of tests/test_gpu_gaxpy_tiled_pipeline.py, checked where no device is needed: every case of
tests/tiled_pipeline_cases.py has the geometry it was built for (under tiled_cases' mirror of gaxpy_tiled_prepare, for 64, 256
and 304 compute units) and a result that is the same bytes in any order of summation, the way tests/test_tiled_cases_cpu.py
checks the cases of tests/tiled_cases.py."""
import numpy as np
import pytest

import tiled_cases as TC
import tiled_pipeline_cases as PC
from test_tiled_cases_cpu import CUS, any_order_is_exact


@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("cus", CUS)
def test_ring_ladder(cus, shape):
    case = PC.ring_ladder(cus, shape)
    m, n, Ap, Ai = case[:4]
    p = TC.plan(m, n, cus, Ap, Ai)
    assert (p["row_block"], p["nrb"], p["nslab"], p["rounds"], p["key_bytes"]) == (8, cus, 1, 1, 3)
    blocks = PC.ring_blocks(cus, shape)
    assert p["groups"].tolist() == [blocks[b][0] if b in blocks else 0 for b in range(cus)]
    assert p["tile_counts"][:, 0].tolist() == [256 * (blocks[b][0] - 1) + blocks[b][1] if b in blocks else 0
                                               for b in range(cus)]
    NW, NG = TC.SHAPES[shape]
    K = NW * NG
    have = set(blocks.values())
    for k in range(1, 8):                                 # 1 .. 5 steps and, for the ring of period 6, its wrap
        assert {(k * K, 256), (k * K - NW, 256), ((k - 1) * K + 1, 1)} <= have
    assert (1, 1) in have and 1 < NW                      # a workgroup with fewer groups than waves
    assert p["groups"][-1] > 0                            # the plan's last group ends a row block
    ref, ints = any_order_is_exact(case)
    assert 0 < ints.sum() < m


@pytest.mark.parametrize("cus", CUS)
def test_two_rounds_restart(cus):
    case = PC.two_rounds_restart(cus)
    m, n, Ap, Ai = case[:4]
    p = TC.plan(m, n, cus, Ap, Ai)
    assert p["rounds"] == 2 and cus < p["nrb"] <= 2 * cus and p["key_bytes"] == 3 and p["nslab"] == 1
    for b in PC.restart_empty_blocks(cus):
        assert p["groups"][b] == 0
    assert p["groups"][5 + cus] > 0 and p["groups"][7] > 0 and p["groups"][9 + cus] == 0 == p["groups"][9]
    assert sorted(set(p["groups"][:8].tolist()) - {0}) == [40, 41, 42]      # 2 - 3 steps of 4 x 5
    assert np.delete(p["groups"], PC.restart_empty_blocks(cus)).min() >= 2
    ref, ints = any_order_is_exact(case)
    assert 0 < ints.sum() < m


@pytest.mark.parametrize("R", PC.TILE_ROWS + tuple(r for s in range(4) for r in PC.batch_edge_rows(s)))
@pytest.mark.parametrize("cus", CUS)
def test_tile_rows(cus, R):
    case = PC.tile_rows(cus, R)
    m, n, Ap, Ai, Ax, x, y0 = case
    p = TC.plan(m, n, cus, Ap, Ai)
    assert (p["row_block"], p["nrb"], p["rounds"], p["nslab"]) == (R, cus, 1, 1)
    assert m - (p["nrb"] - 1) * R == (R - 1 if R >= 2 else 1)
    assert np.unique(y0).size == m and not np.any(y0 == 0)
    rows = np.bincount(Ai, minlength=m)
    if R >= 3:
        assert 0 < np.count_nonzero(rows) < m
        first, last = rows[0::R], rows[R - 1::R]
        assert first[0::2].all() and not first[1::2].any() and last[0::2].all()
    ref, ints = any_order_is_exact(case)
    assert np.abs(ref[ints]).max() < 2.0 ** 53
    if R >= 3:
        assert 0 < ints.sum() < m


@pytest.mark.parametrize("cus", CUS)
def test_last_block_of_one_row(cus):
    case = PC.tile_rows(cus, 3, True)
    p = TC.plan(case[0], case[1], cus, case[2], case[3])
    assert (p["row_block"], p["nrb"]) == (3, cus) and case[0] - (cus - 1) * 3 == 1
    any_order_is_exact(case)


@pytest.mark.parametrize("cus", CUS)
def test_untouched_tiles(cus):
    case, rows = PC.untouched_tiles(cus)
    m, n, Ap, Ai, Ax, x, y0 = case
    p = TC.plan(m, n, cus, Ap, Ai)
    assert p["row_block"] == PC.UNTOUCHED_R and p["nrb"] == cus
    groups = p["groups"]
    assert (groups[0::3] > 0).all() and not groups[1::3].any() and not groups[2::3].any()
    blocks = rows // PC.UNTOUCHED_R
    assert set(blocks.tolist()) == {1, 2} and not groups[blocks].any()
    assert (PC.UNTOUCHED_R * 1) % 2 == 1 and (PC.UNTOUCHED_R * 2) % 2 == 0      # a block beginning odd and one even
    any_order_is_exact(case)
    sp = PC.with_specials(case, rows)[6]
    bits = sp[rows].view(np.uint64)
    assert bits[0] == 1 << 63 and np.isnan(sp[rows[1:4]]).all() and np.unique(bits).size == 4
