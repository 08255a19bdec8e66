"""The table of tests/sort_cases.py, held to its own claims without a device: by the Python model of the host decisions in
csx_sort.hip every case sits on the edge it names and has its named neighbour on the other side; together the cases launch
every k_rs_scatter instance, take every branch of the column expansion, read keys with both histogram kernels on both of their
load paths and recurse the scan and the reverse minimum to every depth up to three -- or the table says why not.  The constants
come from the library (csx_prim_limits), which needs no device."""
import numpy as np
import pytest

import _csx
import sort_cases as SC

LIM = SC.LIM
SORT = SC.NAMES["sort"]


def test_the_limits_are_the_documented_ones():
    assert tuple(LIM) == _csx.PRIM_LIMITS and all(isinstance(v, int) and v > 0 for v in LIM.values())
    assert LIM["RS_BINS"] == 256                                    # a digit is at most 8 bits (key_bits / 8 passes)
    assert LIM["RS_DESC_STARTS"] < LIM["RS_TILE"] < 1 << 16         # a start relative to its tile fits the descriptor's 16 bits
    assert LIM["RS_DESC_STARTS"] % 4 == 0                           # the descriptor is two equal registers of words
    assert _csx.load().csx_prim_limits(None) == _csx.EINVAL


def test_bad_arguments_are_refused_before_the_device():
    """(no device here: a call that got as far as the device would not return CSX_EINVAL but a runtime error)"""
    lib, C = _csx.load(), _csx.C
    k = np.zeros(8, np.uint32)
    o = np.zeros(8, np.uint32)
    p = np.zeros(9, np.int32)
    v = np.zeros(8)
    kp, op = k.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p)
    assert lib.csx_prim_scan(_csx.pi(p), _csx.pi(p), -1, 0, None) == _csx.EINVAL
    assert lib.csx_prim_scan(_csx.pi(p), None, 4, 0, None) == _csx.EINVAL
    assert lib.csx_prim_suffix_min(_csx.pi(p), -1) == _csx.EINVAL
    assert lib.csx_prim_expand_columns(_csx.pi(p), -1, 0, _csx.pi(p)) == _csx.EINVAL
    assert lib.csx_prim_expand_columns(_csx.pi(p), 8, 5, _csx.pi(p)) == _csx.EINVAL            # Ap[n] is not nnz
    for mis in (-1, 4):
        assert lib.csx_prim_boundaries(kp, 8, 1, _csx.pi(p), mis) == _csx.EINVAL
        assert lib.csx_prim_sort(kp, None, None, 8, 1, op, None, None, None, 0, None, 0, mis) == _csx.EINVAL
    assert lib.csx_prim_boundaries(kp, -1, 1, _csx.pi(p), 0) == _csx.EINVAL
    assert lib.csx_prim_boundaries(kp, 8, 0, _csx.pi(p), 0) == _csx.EINVAL                     # key 0 is not below nkeys = 0
    assert lib.csx_prim_sort(kp, None, None, -1, 1, op, None, None, None, 0, None, 0, 0) == _csx.EINVAL
    assert lib.csx_prim_sort(kp, kp, None, 8, 1, op, None, None, None, 0, None, 0, 0) == _csx.EINVAL       # a without out_a
    assert lib.csx_prim_sort(kp, None, _csx.pd(v), 8, 1, op, None, None, None, 0, None, 0, 0) == _csx.EINVAL   # v without out_v
    assert lib.csx_prim_sort(kp, None, None, 8, 1, op, None, None, _csx.pi(p), 8, None, 0, 0) == _csx.EINVAL   # columns, no out_a
    assert lib.csx_prim_sort(kp, None, None, 8, 1, op, None, None, None, 0, _csx.pi(p), 0, 0) == _csx.EINVAL   # keys not below nkeys
    assert lib.csx_prim_sort_info(None, 17) == _csx.EINVAL


def test_model_of_the_digit_widths():
    """digits as even as the key allows; the two uneven splits the kernels' comments name"""
    assert SC.digit_widths(17) == (6, 6, 5) and SC.digit_widths(25) == (7, 6, 6, 6) and SC.digit_widths(32) == (8, 8, 8, 8)
    for bits in range(1, 33):
        w = SC.digit_widths(bits)
        assert sum(w) == bits and max(w) <= 8 and max(w) - min(w) <= 1 and list(w) == sorted(w, reverse=True)
    assert [SC.key_bits(x) for x in (0, 1, 2, 3, 256, 257, 1 << 31, (1 << 31) + 1, 0xFFFFFFFF)] == [1, 1, 1, 2, 8, 9, 31, 32, 32]


@pytest.mark.parametrize("nblocks", [1, 7, 8, 9, 15, 16, 17, 64, 65, 257])
def test_model_of_the_tile_remap_is_a_permutation(nblocks):
    assert sorted(SC.remap_tiles(nblocks).tolist()) == list(range(nblocks))


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_case_sits_on_its_edge(name):
    case, f = SC.BY_NAME[name], SC.facts(name)
    assert case.edge, name
    for key, want in case.edge.items():
        assert f[key] == want, (name, key, f[key], want)
    d = SC.inputs(name)
    if case.prim == "sort":
        key = d["key"]
        assert key.dtype == np.uint32 and (len(key) == 0 or int(key.max()) < d["key_limit"])
        if len(key) > 1:
            assert len(np.unique(key)) < len(key), name                      # duplicates: stability is under test
        if d.get("nkeys") is not None:
            assert len(key) == 0 or int(key.max()) < d["nkeys"]
        xp = d.get("expand_ptr")
        if xp is not None:
            assert xp[0] == 0 and xp[-1] == len(key) and np.all(np.diff(xp.astype(np.int64)) >= 0)
    if case.prim == "boundaries":
        key = d["key"].astype(np.int64)
        assert np.all(np.diff(key) >= 0) and (len(key) == 0 or key[-1] < d["nkeys"])


@pytest.mark.parametrize("name", [c.name for c in SC.CASES if c.other])
def test_the_neighbour_is_on_the_other_side(name):
    other = SC.BY_NAME[name].other
    assert other in SC.BY_NAME and SC.BY_NAME[other].prim == SC.BY_NAME[name].prim, (name, other)
    assert SC.differs(name, other), (name, other, SC.BY_NAME[name].cut)


def test_scan_and_suffix_min_reach_every_depth():
    for prim, tile in (("scan", LIM["SCAN_TILE"]), ("sufmin", LIM["SM_TILE"])):
        by_n = {SC.facts(n)["n"]: SC.facts(n)["depth"] for n in SC.NAMES[prim]}
        assert {0, 1, 2, tile - 1, tile, tile + 1, 3 * tile + 5, tile * tile - 1, tile * tile, tile * tile + 1} <= set(by_n)
        assert set(by_n.values()) == {0, 1, 2, 3}
        assert (by_n[tile], by_n[tile + 1], by_n[tile * tile], by_n[tile * tile + 1]) == (1, 2, 2, 3)


def test_boundaries_cover_every_remainder_path_and_closing():
    seen = {(SC.facts(n)["rem4"], SC.facts(n)["misalign"]) for n in SC.NAMES["boundaries"]}
    assert seen == {(r, m) for r in range(4) for m in range(4)}
    counts = {SC.facts(n)["count"] for n in SC.NAMES["boundaries"]}
    assert set(SC.BOUNDARY_COUNTS) <= counts and 0 in counts
    paths = set()
    for n in SC.NAMES["boundaries"]:
        paths |= SC.facts(n)["paths"]
    assert paths == {"vector", "scalar", "tail"}
    assert max(SC.facts(n)["longest_gap"] for n in SC.NAMES["boundaries"]) >= 5000
    assert any(SC.facts(n)["closing"] > 9000 for n in SC.NAMES["boundaries"])        # thousands of trailing keys closed by the last thread
    assert any(SC.facts(n)["nkeys"] == 1 and SC.facts(n)["count"] > 1000 for n in SC.NAMES["boundaries"])


def test_expand_covers_the_rounds_of_a_wave_and_the_wrap():
    lengths, wraps = set(), set()
    for n in SC.NAMES["expand"]:
        f = SC.facts(n)
        lengths |= f["lengths"]
        wraps.add(f["wraps"])
    assert {0, 1, 63, 64, 65, 200} <= lengths and wraps == {False, True}
    assert SC.facts("exp_grid_wraps")["n"] == 4 * LIM["EXPAND_GRID_MAX"] + 3 and SC.facts("exp_nnz0")["nnz"] == 0


def test_together_the_sort_cases_launch_everything():
    instances, branches, hist, passes, remaps, nchunks, chunks = set(), set(), set(), set(), set(), set(), set()
    chains = set()
    for n in SORT:
        f = SC.facts(n)
        instances |= set(f["instances"])
        chains.add(f["instances"])
        branches |= f["branches"]
        hist |= f["hist"]
        passes.add(f["passes"])
        remaps.add((f["q"] == 0, f["rem"] != 0))
        nchunks.add(f["nchunks"])
        chunks.add(f["chunk"])
    assert instances == set(_csx.SORT_INSTANCES) - {"none"}
    assert branches == {"paint", "lds", "search"}
    assert hist == {("hist", "vector"), ("hist", "scalar"), ("hist16", "vector"), ("hist16", "scalar")}
    assert passes == {0, 1, 2, 3, 4}
    assert remaps >= {(True, True), (False, False), (False, True)}            # q = 0; rem = 0; both nonzero
    segs = LIM["RS_SEGS"]
    assert {1, 2, segs, segs + 1} <= nchunks                                     # fewer than, as many as, more than the segments
    # every chain of record layouts a sort of (a, v) can take: one to four passes
    assert {("av_flat_flat",), ("av_flat_packed", "av_packed_flat"), ("av_flat_packed", "av_packed_packed", "av_packed_flat"),
            ("av_flat_packed", "av_packed_packed", "av_packed_packed", "av_packed_flat"),
            ("short_first", "short_middle", "short_last")} <= chains
    # the one edge left out, and the one path no input can take
    assert chunks - {0} == {LIM["RS_CHUNK_MIN"]}
    assert list(SC.NOT_REACHED) == ["chunk > RS_CHUNK_MIN", "k_rs_hist16 on a misaligned array"] and all(SC.NOT_REACHED.values())
    assert max(SC.facts(n)["nblocks"] for n in SORT) <= LIM["RS_CHUNK_MIN"] * LIM["RS_CHUNK_DIV"]


def test_expansion_cases_sit_on_every_start_count():
    tile, desc = LIM["RS_TILE"], LIM["RS_DESC_STARTS"]
    for sfx in ("_v", "_pattern"):
        Ks = set()
        for n in SORT:
            if n.startswith("x_") and n.endswith(sfx):
                Ks |= set(SC.facts(n)["K"])
        half = desc // 2 - 2
        assert {0, 1, half - 1, half, half + 1, desc, desc + 1, tile - 1, tile, tile + 1} <= Ks and max(Ks) >= 3 * tile
        assert SC.desc_half_of_last_start(half) == 0 and SC.desc_half_of_last_start(half + 1) == 1
        # a column on a tile base without and with empty columns before it; empty columns in front and at the end; one column
        Ap = SC.inputs("x_base_start" + sfx)["expand_ptr"]
        assert np.count_nonzero(Ap == tile) == 1 and np.count_nonzero(Ap == 2 * tile) == 1
        Ap = SC.inputs("x_base_start_after_empties" + sfx)["expand_ptr"]
        assert np.count_nonzero(Ap == tile) == 6 and np.count_nonzero(Ap == 2 * tile) == 3
        Ap = SC.inputs("x_empties_front_end" + sfx)["expand_ptr"]
        assert np.count_nonzero(Ap == 0) == 9 and np.count_nonzero(Ap == Ap[-1]) == 12
        assert len(SC.inputs("x_one_column" + sfx)["expand_ptr"]) == 2
        Ap = SC.inputs("x_long_column" + sfx)["expand_ptr"]
        assert int(np.diff(Ap).max()) > 5 * tile
        # equal starts (empty columns) among the painted ones and in the searched list
        for n in ("x_dups_painted", "x_starts%d" % tile):
            Ap = SC.inputs(n + sfx)["expand_ptr"]
            mid = Ap[(Ap > tile) & (Ap < 2 * tile)]
            assert len(np.unique(mid)) < len(mid), n


def test_short_key_cases_hold_the_first_and_last_key_of_every_digit():
    for name in ("x_short17_on", "x_short17_off", "x_short24_on", "x_short24_off"):
        d, f = SC.inputs(name), SC.facts(name)
        m, w0 = d["key_limit"], f["widths"][0]
        key = d["key"].astype(np.int64)
        assert f["count"] > 2 * LIM["RS_TILE"] and f["count"] % LIM["RS_TILE"]        # hist16 on both of its load paths
        for dg in range(1 << w0):
            mine = key[(key & ((1 << w0) - 1)) == dg]
            assert mine.min() == dg and mine.max() == ((m - 1 - dg) >> w0 << w0) + dg
            assert np.count_nonzero(key == mine.min()) >= 2 and np.count_nonzero(key == mine.max()) >= 2
    fit, more = SC.facts("x_columns_fit"), SC.facts("x_columns_one_more")
    assert (fit["k16"], more["k16"]) == (1, 0) and fit["instances"][0] == "short_first" and more["instances"][0] == "av_flat_packed"
    assert "search" in fit["branches"] and len(SC.inputs("x_columns_fit")["expand_ptr"]) - 1 == 1 << (32 - fit["widths"][0])
