"""The inputs of tests/test_gpu_gaxpy_tiled.py, checked where no device is needed: every case of tests/tiled_cases.py has the
geometry it was built for (under the mirror of gaxpy_tiled_prepare's arithmetic, for 64, 256 and 304 compute units), and its
result is the same bytes in any order of summation -- the condition under which an atomic kernel can be held to the
oracle's bytes."""
import functools

import numpy as np
import pytest

import c_oracle as CO
import tiled_cases as TC

CUS = (64, 256, 304)


def any_order_is_exact(case):
    """the oracle's y (columns ascending, storage order inside a column) == the terms added in three random orders"""
    m, n, Ap, Ai, Ax, x, y0 = case
    ref = CO.gaxpy(m, n, Ap, Ai, Ax, x, y0)
    terms = Ax * np.repeat(x, np.diff(Ap))
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(Ai.size)
        y = y0.copy()
        np.add.at(y, Ai[perm], terms[perm])          # unbuffered: one rounded addition per term, in this order
        assert y.tobytes() == ref.tobytes(), seed
    assert not np.any((ref == 0) & np.signbit(ref))
    ints = TC.is_integer_row(case)
    single_rows = np.flatnonzero(~ints)
    assert (np.bincount(Ai, minlength=m)[single_rows] == 1).all()
    return ref, ints


@functools.lru_cache(maxsize=None)
def ladder(cus, shape):
    return TC.group_ladder(cus, shape)


@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("cus", CUS)
def test_group_ladder(cus, shape):
    case = ladder(cus, shape)
    m, n, Ap, Ai = case[:4]
    p = TC.plan(m, n, cus, Ap, Ai)
    assert (p["row_block"], p["nrb"], p["nslab"], p["rounds"], p["key_bytes"]) == (8, cus, 1, 1, 3)
    want = TC.ladder_groups(cus, shape)
    assert p["groups"].tolist() == [G for G, r in want]
    assert p["tile_counts"][:, 0].tolist() == [max(256 * G - r, 0) for G, r in want]
    NW, NG = TC.SHAPES[shape]
    for G in (0, 1, NW - 1, NW, NW + 1, NW * NG - 1, NW * NG, NW * NG + 1, 2 * NW * NG - 1, 2 * NW * NG, 2 * NW * NG + 1):
        for r in (0, 1, 255):
            assert (G, r) in want or G == 0
    col = np.repeat(np.arange(n), np.diff(Ap))
    pairs = col.astype(np.int64) * m + Ai
    assert np.unique(pairs).size < pairs.size                        # duplicates of one (i, j)
    assert any(np.any(np.diff(Ai[Ap[j]:Ap[j + 1]]) < 0) for j in range(n))   # rows unsorted inside a column
    ref, ints = any_order_is_exact(case)
    assert 0 < ints.sum() < m


@pytest.mark.parametrize("cus", CUS)
def test_slabs(cus):
    case = TC.slabs(cus)
    m, n, Ap, Ai, Ax, x, y0 = case
    p = TC.plan(m, n, cus, Ap, Ai)
    assert (p["nslab"], p["slab_cols"], p["rounds"], p["key_bytes"]) == (3, 131072, 1, 3)
    assert n - 2 * p["slab_cols"] == 5 and m % p["row_block"] != 0 and p["nrb"] > 1
    assert (p["tile_counts"] > 0).all() and (p["tile_counts"] % 256 != 0).all()
    assert (p["tile_counts"][:, :2].max(axis=0) > 256).all() and p["tile_counts"][:, 2].max() > 256
    for j in (0, 131071, 131072, 262143, 262144, 262148):
        assert Ap[j + 1] > Ap[j], j
    used = np.flatnonzero(np.diff(Ap[:131073]) > 0)
    both = used[np.diff(Ap)[used + 131072] > 0]
    assert both.size > 100 and (x[both] != x[both + 131072]).all()
    assert (x[262144:] != x[:5]).all() and (x[262144:] != x[131072:131077]).all()
    ref, ints = any_order_is_exact(case)
    assert 0 < ints.sum() < m


@pytest.mark.parametrize("cus", CUS)
def test_key_edges(cus):
    cases = TC.key_edges(cus)
    assert [(label, kb) for label, kb, case in cases] == [("run_511_wide", 3), ("run_512_wide", 4), ("two_narrow_runs", 3)]
    for label, kb, case in cases:
        m, n, Ap, Ai = case[:4]
        p = TC.plan(m, n, cus, Ap, Ai)
        assert p["key_bytes"] == kb and p["nslab"] == 1, label
        assert np.count_nonzero(p["tile_counts"]) == 1, label                     # one row block, one slab
        assert p["max_offset"] == {"run_511_wide": 511, "run_512_wide": 512, "two_narrow_runs": 63}[label]
        ref, ints = any_order_is_exact(case)
        assert 0 < ints.sum() < m
    m, n, Ap, Ai = cases[2][2][:4]
    assert Ap[600] == 64 and Ap[601] == 65                                       # the second run starts at column 600


@pytest.mark.parametrize("two_rounds", [False, True])
@pytest.mark.parametrize("cus", CUS)
def test_lds_edges(cus, two_rounds):
    case = TC.lds_edges(cus, two_rounds)
    m, n, Ap, Ai = case[:4]
    p = TC.plan(m, n, cus, Ap, Ai)
    assert 2e5 * cus / 256 < Ai.size < 5e5 * cus / 256 and n == 1000 and p["key_bytes"] == 3
    counts = p["tile_counts"][:, 0]
    rows = set(Ai.tolist())
    if not two_rounds:
        assert (p["row_block"], p["nrb"], p["rounds"]) == (TC.TL_LDS_ROWS, cus, 1)
        assert p["lds_bytes"] == TC.TL_LDS_BYTES == 163584
        assert p["saturated"] and p["max_offset"] == 511
        assert (counts > 0).all()
    else:
        assert p["row_block"] < TC.TL_LDS_ROWS and cus < p["nrb"] <= 2 * cus and p["rounds"] == 2
        second = counts[cus:]
        first = counts[:second.size]
        assert counts[3] == 0 and counts[3 + cus] > 0
        assert (second > 0).all() and (np.delete(first, 3) > 0).all() and (first != second).all()
        assert (p["groups"][:second.size] != p["groups"][cus:]).all()
        assert not p["saturated"]
    rb = p["row_block"]
    for r in (0, rb - 1, (p["nrb"] - 1) * rb, m - 1):
        assert r in rows, r
    ref, ints = any_order_is_exact(case)
    assert 0 < ints.sum() < m


@pytest.mark.parametrize("cus", CUS)
def test_degenerate(cus):
    cases = dict(TC.degenerate(cus))
    assert list(cases) == ["no_entries", "one_by_one", "m_below_cus", "m_cus_plus_1", "one_column", "one_row",
                           "last_row_block_only"]
    for label, case in cases.items():
        any_order_is_exact(case)
    plans = {label: TC.plan(c[0], c[1], cus, c[2], c[3]) for label, c in cases.items()}
    assert plans["no_entries"]["ngroups"] == 0 and cases["no_entries"][2][-1] == 0
    assert cases["one_by_one"][:2] == (1, 1)
    assert cases["m_below_cus"][0] < cus and plans["m_below_cus"]["row_block"] == 1
    assert cases["m_cus_plus_1"][0] == cus + 1 and plans["m_cus_plus_1"]["row_block"] == 2
    assert cases["one_column"][1] == 1 and cases["one_row"][0] == 1
    last = plans["last_row_block_only"]
    assert last["groups"][-1] > 0 and last["groups"][:-1].sum() == 0 and last["nrb"] == cus


@pytest.mark.parametrize("avg", TC.DENSITIES)
def test_density_ladder(avg):
    case = TC.density_ladder(avg)
    m, n, Ap, Ai = case[:4]
    assert Ai.size == avg * m and np.bincount(Ai, minlength=m).min() >= 1
    any_order_is_exact(case)


def test_geometry_of_the_benchmarked_size():
    g = TC.geometry(5000000, 5000000, 256)
    assert (g["row_block"], g["nrb"], g["rb_bits"], g["nslab"], g["rounds"]) == (19532, 256, 15, 39, 1)
    assert TC.geometry(256 * 20446 + 1, 1000, 256)["rounds"] == 2
