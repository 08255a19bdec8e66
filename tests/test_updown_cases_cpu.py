"""The cases of tests/updown_cases.py on the CPU: for every case the column-fused order (updown_block_oracle.updown_block, the
device kernel's order with its chunks, dead terms, restore and replay) is byte-equal to the reference loop of
csparse_oracle.cs_updown and returns the same count, with all or nothing too; and the model of the schedule
(updown_block_oracle.schedule) reports the edge the case is named for: the class vector, the chunk and group counts, the
popcounts of the masks, the trips of the lanes and the ucnt * nterm products at the 60 KB limit.  No GPU."""
import numpy as np
import pytest

import updown_block_oracle as UB
import updown_cases as UC


def _sched(c):
    return UB.schedule(c.oracle_L(), c.oracle_C())


@pytest.mark.parametrize("name", UC.NAMES)
def test_fused_order_is_the_reference_loop(name):
    c = UC.get(name)
    assert c.applied == c.want and c.fails == (name in UC.FAILING)
    L = c.oracle_L()
    assert UB.updown_block(L, c.sigma, c.oracle_C()) == c.applied
    assert np.asarray(L.x[:len(c.x)]).tobytes() == c.ref_x
    if c.fails:
        L = c.oracle_L()
        assert UB.updown_block(L, c.sigma, c.oracle_C(), None, True) == c.applied
        assert np.asarray(L.x[:len(c.x)]).tobytes() == c.x.tobytes()
        # the loop's partial state is not the untouched factor (but for the lone term that fails at its first column)
        assert (c.ref_x != c.x.tobytes()) == (name != "zero_beta2_only")


@pytest.mark.parametrize("name", UC.NAMES)
def test_model_reports_the_stated_edge(name):
    c = UC.get(name)
    sched = _sched(c)
    facts = UB.schedule_facts(sched)
    assert [len(ch["groups"]) for ch in sched] == c.expect["groups"]
    assert facts["chunks"] == c.expect["chunks"] and facts["groups"] == sum(c.expect["groups"])
    for key in ("classes", "union_columns"):
        if key in c.expect:
            assert facts[key] == c.expect[key]
    if "tree_groups" in c.expect:
        assert [ch["groups"] for ch in sched] == c.expect["tree_groups"]
    if "w_doubles" in c.expect:
        assert [g[0] * g[1] for g in sched[0]["groups"]] == c.expect["w_doubles"]
    for ch in sched:                                            # every mask within the chunk's terms, every term on a column
        for nterm, ucnt, maxlen, cls in ch["groups"]:
            assert 1 <= nterm <= 64 and ucnt >= 1
        assert all(0 < m < (1 << 64) for m in ch["masks"].values())


def test_the_lds_limit_is_met_exactly():
    """7680 doubles are 61440 bytes, the last W that stays in LDS; 7744 (and 7808) are the first that do not"""
    assert 7680 * 8 == UB.UD_LDS_W and 120 * 64 == 7680 and 128 * 60 == 7680
    for name in ("four_classes", "lds_edge_by_terms"):
        for nterm, ucnt, maxlen, cls in _sched(UC.get(name))[0]["groups"]:
            assert (cls >= 2) == (nterm * ucnt <= 7680)
            assert (cls & 1) == (maxlen > 64)
    assert sorted(g[2] for g in _sched(UC.get("four_classes"))[0]["groups"]) == [64, 64, 65, 65]


def test_staggered_has_every_popcount():
    sched = _sched(UC.get("staggered"))
    pops = {bin(m).count("1") for m in sched[0]["masks"].values()}
    assert pops == set(range(1, 65))                            # 16 / 17, 32 / 33 and 48 / 49: the refills of 16 terms
    assert sched[0]["masks"][139] == (1 << 64) - 1
    assert [ch["groups"][0][0] for ch in sched] == [64, 64, 2]


def test_sparse_masks_are_single_bits_and_all_ones():
    sched = _sched(UC.get("sparse_masks"))
    m = sched[0]["masks"]
    assert all(m[b] == 1 << b for b in range(64)) and m[0] == 1 and m[63] == 1 << 63
    assert all(m[s] == (1 << 64) - 1 for s in range(64, 69))
    assert sorted(sched[1]["masks"]) == [0, 9, 63, 64, 65, 66, 67, 68]
    assert sched[1]["masks"][0] == 0b1001001 and sched[1]["masks"][9] == 0b0010010 and sched[1]["masks"][64] == 0b1111111


def test_trip_counts():
    """entries below the diagonal over the lanes: 256 -> one trip of 256, 257 -> two; 1029 -> five, and two of k_updown's 1024"""
    trips = lambda maxlen, lanes: (maxlen - 1 + lanes - 1) // lanes
    g = _sched(UC.get("block_trips"))[0]["groups"]
    assert [trips(x[2], 256 if x[3] & 1 else 64) for x in g] == [1, 2, 1, 1]
    d = _sched(UC.get("dense_1030"))[0]["groups"][0]
    assert trips(d[2], 256) == 5 and trips(d[2], 1024) == 2 and len(UC.get("dense_1030").x) == 1030 * 1031 // 2


def test_failure_cases_fail_where_they_are_meant_to():
    """the ranks and trees the failure cases are named for, read off the model's trees"""
    c = UC.get("fail_chunk0_skips_chunk1")
    sched = _sched(c)
    assert [g[0] for g in sched[0]["groups"]] == [64, 64] and [g[0] for g in sched[1]["groups"]] == [36, 6]
    assert c.applied == 20 and min(c.cols[20][0]) < 16          # tree A's rank-10 term
    assert sum(1 for t in range(20) if min(c.cols[t][0]) >= 16) == 10 and min(c.cols[139][0]) >= 16   # B on both sides
    c = UC.get("two_trees_fail")
    assert c.applied == 25 and min(c.cols[25][0]) >= 16 and min(c.cols[40][0]) < 16
    alone = UC.columns(UC.O, c.n, c.cols[:26])                  # without term 40 the loop stops at 25 with the same bytes
    L = c.oracle_L()
    assert UB.loop(L, c.sigma[:26], alone, UB.tree_of(L), UC.O) == 25
    assert np.asarray(L.x[:len(c.x)]).tobytes() == c.ref_x
    only_a = UC.columns(UC.O, c.n, c.cols[:25] + [c.cols[40]])  # and term 40 does fail by itself
    L = c.oracle_L()
    assert UB.loop(L, c.sigma[:25] + [c.sigma[40]], only_a, UB.tree_of(L), UC.O) == 25
    for name, rank in (("fail_bit63", 63), ("fail_bit0_chunk1", 64)):
        assert UC.get(name).applied == rank
    for cl in range(4):
        c = UC.get("fail_in_class%d" % cl)
        assert c.applied == 256 and c.k == 257
        assert [g[3] for g in _sched(c)[0]["groups"]] == [2, 3, 0, 1]
    for name in ("zero_beta2_only", "zero_beta2_mid"):
        c = UC.get(name)
        t = c.applied
        assert c.sigma[t] == -1 and c.cols[t] == ([0], [float(c.x[0])])    # alpha = 1, beta2 = 1 - 1 = 0.0


def test_parent_given_is_parent_read():
    for name in ("off_path", "isolated_root", "chunks_uneven"):
        c = UC.get(name)
        L = c.oracle_L()
        par = UB.tree_of(L)
        assert UB.updown_block(L, c.sigma, c.oracle_C(), par) == c.applied
        assert np.asarray(L.x[:len(c.x)]).tobytes() == c.ref_x
        assert UB.schedule(c.oracle_L(), c.oracle_C(), par) == _sched(c)
