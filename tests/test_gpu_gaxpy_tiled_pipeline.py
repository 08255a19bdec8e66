"""The pipelined step and the bulk tile copy of the tiled cs_gaxpy kernel (csx_gaxpy_tiled.hip) where they can go wrong: walks
of 1 to 7 steps (both register sets, and every phase and the wrap of the three-set key ring of the ablation build), the last
step full, short and of one entry, the loads ahead clamped at the end of the plan's arrays, a walk that starts after a row
block without a step, and row blocks whose length puts the 16-byte pairs of the tile copy at every edge.

Inputs from tests/tiled_pipeline_cases.py (checked on the CPU by tests/test_tiled_pipeline_cases_cpu.py): sums exact in any
order, so every result is held to the BYTES of the plain-C oracle, as in tests/test_gpu_gaxpy_tiled.py, whose helpers run
the cases here.  Through the C ABI with numpy arrays; needs an MI355X."""
import functools

import numpy as np
import pytest

import c_oracle as CO
import tiled_cases as TC
import tiled_pipeline_cases as PC
from test_gpu_gaxpy_tiled import cs, cus, gaxpy, geometry, lib, prepared, same_bytes  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def built(builder, *args):
    return getattr(PC, builder)(*args)


def groups_of(blocks, nrb):
    return [blocks[b][0] if b in blocks else 0 for b in range(nrb)]


# --------------------------------------------------------------------------------------------------------------- ring phase

@pytest.mark.parametrize("keys24", [1, 0])
@pytest.mark.parametrize("shape", range(4))
def test_ring_ladder_at_each_shape(lib, cs, cus, shape, keys24):
    """walks of 1 .. 7 steps (six phases of the key ring and the wrap), the last step full, one group per wave short, and one
    group of one entry; row blocks with fewer groups than waves and with none; the plan's last group ends a row block"""
    import _csx
    case = built("ring_ladder", cus, shape)
    hA, geo = prepared(lib, cs, case, cus, keys24)
    try:
        NW, NG = TC.SHAPES[shape]
        assert (geo["row_block"], geo["nrb"], geo["nslab"], geo["key_bytes"]) == (8, cus, 1, 3 if keys24 else 4)
        assert geo["groups"] == groups_of(PC.ring_blocks(cus, shape), cus)
        assert geo["groups"][-1] > 0 and geo["groups_min"] == 0 and 1 in geo["groups"] and 1 < NW
        assert geo["groups_max"] == 7 * NW * NG
        with _csx.option("gaxpy.shape", shape):
            assert geometry(lib, hA)["shape"] == shape
            same_bytes(gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED), case)
    finally:
        _csx.free(hA)


@pytest.mark.parametrize("ladder", range(4))
def test_each_ring_ladder_on_one_plan_at_all_four_shapes(lib, cs, cus, ladder):
    """shape x part: the ladder built round one shape's step, run at every shape (each has its own step length NW NG and its
    own thread count in the tile copy)"""
    import _csx
    case = built("ring_ladder", cus, ladder)
    hA, geo = prepared(lib, cs, case, cus)
    try:
        for s in range(4):
            with _csx.option("gaxpy.shape", s):
                assert geometry(lib, hA)["shape"] == s
                same_bytes(gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED), case)
    finally:
        _csx.free(hA)


# ------------------------------------------------------------------------------------------------- look-ahead past the end

@pytest.mark.parametrize("shape", range(4))
def test_ring_restarts_after_a_row_block_without_a_step(lib, cs, cus, shape):
    """two row blocks per workgroup: a first block without entries, a second one, both; the keys and values a walk asked for
    past its end must not reach the next walk"""
    import _csx
    case = built("two_rounds_restart", cus)
    hA, geo = prepared(lib, cs, case, cus)
    try:
        assert geo["nrb"] > cus and geo["key_bytes"] == 3 and geo["nslab"] == 1
        for b in PC.restart_empty_blocks(cus):
            assert geo["groups"][b] == 0
        assert geo["groups"][5 + cus] > 0 and geo["groups"][7] > 0 and geo["groups_max"] >= 42
        with _csx.option("gaxpy.shape", shape):
            same_bytes(gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED), case)
    finally:
        _csx.free(hA)


# ----------------------------------------------------------------------------------------------------------- fill and drain

def run_tile_rows(lib, cs, cus, case, R, shape):
    import _csx
    hA, geo = prepared(lib, cs, case, cus)
    try:
        assert geo["row_block"] == R and geo["nrb"] == min(cus, case[0])
        with _csx.option("gaxpy.shape", shape):
            got = gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED)
    finally:
        _csx.free(hA)
    same_bytes(got, case)
    return got


@pytest.mark.parametrize("R", PC.TILE_ROWS)
def test_tile_copy_at_each_row_block_length(lib, cs, cus, R):
    """row blocks of 1, 2, 3, 255, 256, 257, 4095 and 4097 rows (odd lengths: every second block begins at an odd row of y),
    the last block a row shorter; y0 distinct in every row, most rows without an entry"""
    case = built("tile_rows", cus, R)
    got = run_tile_rows(lib, cs, cus, case, R, 0)
    empty = np.bincount(case[3], minlength=case[0]) == 0
    assert empty.sum() > 0 and got[empty].tobytes() == case[6][empty].tobytes()


@pytest.mark.parametrize("shape", range(4))
def test_tile_copy_round_a_full_batch_at_each_shape(lib, cs, cus, shape):
    """one row either side of eight 16-byte pairs per thread, at the thread count of every shape"""
    for R in PC.batch_edge_rows(shape):
        run_tile_rows(lib, cs, cus, built("tile_rows", cus, R), R, shape)


def test_last_row_block_of_one_row(lib, cs, cus):
    case = built("tile_rows", cus, 3, True)
    assert case[0] % 3 == 1
    run_tile_rows(lib, cs, cus, case, 3, 0)


@pytest.mark.parametrize("shape", range(4))
def test_tile_without_entries_comes_back_bit_for_bit(lib, cs, cus, shape):
    """workgroups whose row block has no entry: y passes through LDS and back unchanged, -0.0 and NaN payloads included"""
    base, rows = built("untouched_tiles", cus)
    case = PC.with_specials(base, rows)
    got = run_tile_rows(lib, cs, cus, case, PC.UNTOUCHED_R, shape)
    assert got[rows].tobytes() == case[6][rows].tobytes()
    assert np.signbit(got[rows[0]]) and got[rows[0]] == 0 and np.isnan(got[rows[1]])
    untouched = (np.arange(case[0]) // PC.UNTOUCHED_R) % PC.UNTOUCHED_EVERY != 0
    assert got[untouched].tobytes() == case[6][untouched].tobytes()
    assert CO.gaxpy(*case)[rows].tobytes() == case[6][rows].tobytes()
