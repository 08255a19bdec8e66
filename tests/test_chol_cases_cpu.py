"""The inputs of tests/test_gpu_chol_edges.py (tests/chol_cases.py) held to what they are named for, without a device: with
the oracle's schol and chol alone every case is positive definite (and its marked value sets are not), has the tree shape and
falls on the side of the band gates it claims, and by the model of the schedule sits exactly on its edge; the table as a whole
reaches every launch kind, every window class and both sides of every constant; the oracle's own distance from a longdouble
factor stays under tol.CHOL_EPS_UNITS; and no update of a case is small enough to hide inside that bound.

The one exception to the last: the fill of a five-point grid decays geometrically across its band (band175: the smallest update
is 6e-132 roundings of its entry's terms), whatever values of one magnitude the grid is given.  The grid cases therefore show
the windows on the workload they were made for; the full bands without fill (dband*) stand on the same window classes and do
meet the condition."""
import re

import numpy as np
import pytest

import chol_cases as CC
import tol as TOL

GRIDS = [n for n in CC.NAMES if re.match(r"band\d", n)]
CHEAP = [n for n in CC.NAMES if int(CC.symbolic(n)[1][-1]) <= 60000]


def _row_lists(name):
    """for every row of L the columns k < row with l_rk != 0, ascending"""
    c = CC.BY_NAME[name]
    Lp, Li, _ = CC.oracle(name)
    cols = np.repeat(np.arange(c.n), np.diff(Lp))
    off = Li != cols
    order = np.lexsort((cols[off], Li[off]))
    rows, ks = Li[off][order], cols[off][order]
    ptr = np.searchsorted(rows, np.arange(c.n + 1))
    return lambda r: ks[ptr[r]:ptr[r + 1]]


@pytest.mark.parametrize("name", CC.NAMES)
def test_values_are_spd_and_the_marked_ones_are_not(name):
    c = CC.BY_NAME[name]
    parent, cp = CC.symbolic(name)
    assert int(np.sum(parent < 0)) == (len(c.marks["cliques"]) if "cliques" in c.marks else c.marks.get("forest", 1))
    if "cliques" not in c.marks and "bintree" not in c.marks:
        assert np.bincount(_roots(parent)).max() > CC.CH_SMALL_TREE
    for which in ("A", 0, 1):
        assert CC.oracle(name, which) is not None, which
    assert c.A2[0].tobytes() != c.A2[1].tobytes() != c.x.tobytes()
    for j in c.bad_at:
        assert CC.oracle(name, ("bad", j)) is None, j
    # diagonally dominant, off-diagonals of one magnitude
    off = c.x[c.i != c.cols]
    assert np.all(off < 0) and np.max(-off) / np.min(-off) <= 1.1
    Lp, Li, Lx = CC.oracle(name)
    cols = np.repeat(np.arange(c.n), np.diff(Lp))
    assert np.all(Lx[Li != cols] < 0)                       # so every update has the same sign


def _roots(parent):
    root = np.arange(len(parent))
    for j in range(len(parent) - 1, -1, -1):
        if parent[j] >= 0:
            root[j] = root[parent[j]]
    return root


@pytest.mark.parametrize("name", CC.NAMES)
def test_route_and_band_gates(name):
    c, m = CC.BY_NAME[name], CC.model(name)
    kind, window, hb = CC.decision(name)
    assert (kind, window) == (c.expect["band"], c.expect["window"])
    assert (m["trees"], m["dense"]) == (c.expect["trees"], c.expect["dense_trees"])
    if kind == 0:
        assert len(m["sns"]) == c.expect["supernodes"]
    if "levels" in c.expect:
        assert CC.expected_levels(name) == c.expect["levels"]
    Lp = CC.oracle(name)[0]
    chain_like = m["big_cols"] * 2 > c.n and m["nlev"] * 4 > m["big_cols"]
    if "need" in c.marks:                                  # a band case: the gates pass, the need is the named one
        assert chain_like and hb + 1 == c.marks["need"]
        full = Lp[c.n] >= 0.5 * c.n * (hb + 1)
        assert full == ("holes" not in c.marks)
        assert (c.option("chol.wband") == 0) == (name.split("-")[-1] != "default")
    elif "arrow" in c.marks:                               # the gates pass; too wide for a window, too empty for the blocked band
        assert chain_like and hb + 1 > CC.MAX_NEED and Lp[c.n] < 0.5 * c.n * (hb + 1) and c.options == ()
    else:
        assert c.option("chol.band") == 0 or not chain_like


def test_both_sides_of_the_default_band_decision():
    assert CC.decision("band79-default")[:2] == (1, 80) and CC.decision("band80-default")[:2] == (2, 0)
    assert CC.BY_NAME["band79-default"].marks["need"] == CC.WBAND_MIN_NEED == CC.BY_NAME["band80-default"].marks["need"] - 1


@pytest.mark.parametrize("name", [n for n in CC.NAMES if "hub" in CC.BY_NAME[n].marks])
def test_hub_edges(name):
    c, m = CC.BY_NAME[name], CC.model(name)
    where, children, long_len = c.marks["hub"], c.marks["children"], c.marks["long_len"]
    Lp, Li, _ = CC.oracle(name)
    cnt = np.diff(Lp)
    b0, q0, K = where["b"], where["q"], long_len - 1
    assert cnt[b0] == long_len and c.n == q0 + K
    level = m["level"]
    assert np.all(level[:where["b"]] == 0) and np.all(level[b0:q0] == 1) and np.array_equal(level[q0:], 2 + np.arange(K))
    assert int(np.sum(level == 1)) == c.marks["level1"] == len(children)
    row = _row_lists(name)
    assert len(row(where["childless"])) == 0
    assert [len(row(b0 + t)) for t in range(len(children))] == children      # the updates every b takes: its leaves
    if len(children) > 4:
        assert sorted(set([0] + children)) == [0, 1, CC.UQ - 1, CC.UQ, CC.UQ + 1, 2 * CC.UQ, 2 * CC.UQ + 1]
    # a_0 is a source column longer than one wave below row b_0, and its update lands on that many rows of the long column
    a0 = Li[Lp[0]:Lp[1]]
    assert a0[1] == b0 and len(a0) - 2 > 64 and row(b0)[0] == 0
    launch1 = [k for k in m["launches"] if k[0] == "coop" and k[1] in (0, 2) and k[2:] == (1, 2, len(children))]
    if c.marks["kind"] == "level":
        assert ("level", 1, CC.CH_NARROW + 1) in m["launches"]
        assert long_len in (CC.CH_ACC, CC.CH_ACC + 1)
    else:
        assert len(children) <= CC.CH_NARROW and len(launch1) == 1
        W = min(CC.CC_WAVES, CC.CC_ACC // long_len)
        assert (long_len, W) in ((512, 16), (513, 15), (1024, 8), (1025, 7))
        assert (W * long_len == CC.CC_ACC) == (long_len in (512, 1024))       # the partials fill CC_ACC exactly | one wave less
    if c.option("chol.supernodes"):
        assert m["sns"] == [(2, q0, K, 0)]
        assert ("coop", 1, 2, 3, K) in m["launches"] and m["levels"] == 3
    else:
        assert m["sns"] == [] and m["widths"][2:].tolist() == [1] * K
        two = [k for k in m["launches"] if k[0] == "coop" and k[1] == 2]
        assert two and not [k for k in m["launches"][:-1] if k[0] == "coop" and k[1] == 0]


WALKS = {15: [("level", 0), ("coop", 0, 1, 16)],
         16: [("level", 0), ("coop", 1, 1, 17), ("coop", 2, 1, 17)],
         64: [("level", 0), ("coop", 1, 1, 65), ("coop", 2, 1, 65)],
         65: [("level", 0), ("coop", 1, 1, 65), ("coop", 2, 1, 65), ("coop", 0, 65, 66)],
         80: [("level", 0), ("coop", 1, 1, 65), ("coop", 2, 1, 65), ("coop", 1, 65, 81), ("coop", 2, 65, 81)]}


@pytest.mark.parametrize("c", sorted(WALKS))
def test_comb_walks(c):
    name = "comb%d" % c
    case, m = CC.BY_NAME[name], CC.model(name)
    assert c in (CC.CC_RUN_MIN - 1, CC.CC_RUN_MIN, CC.CC_RUN_MAX, CC.CC_RUN_MAX + 1, CC.CC_RUN_MAX + CC.CC_RUN_MIN)
    assert [k[:-1] for k in m["launches"]] == WALKS[c] and m["sns"] == []
    assert m["widths"][0] > CC.CH_NARROW and m["widths"][1:].tolist() == [1] * c
    t, level = case.marks["t"], m["level"]
    assert level[t].tolist() == list(range(1, c + 1))
    row = _row_lists(name)
    last = row(t[-1])
    inside = level[last] >= 1                                  # (the first run starts at level 1)
    assert len(last) == 2 * c - 3                              # u_1, t_1, u_2, t_2, ... u_{c-1}
    assert inside.any() and (~inside).any()
    first_inside = int(np.argmax(inside))
    assert (~inside[first_inside:]).any()                      # the outside updates are not a prefix of the list: split[] at work
    assert len(row(t[0])) == 520                               # a row of many single-entry updates
    if c == 80:                                                # the second run's outside holds chain columns of the first
        lf = 65
        assert np.any((level[last] >= 1) & (level[last] < lf))


@pytest.mark.parametrize("name", [n for n in CC.NAMES if "sns" in CC.BY_NAME[n].marks])
def test_supernode_lists(name):
    c, m = CC.BY_NAME[name], CC.model(name)
    assert [s[1:] for s in m["sns"]] == c.marks["sns"]
    groups = [k[2] for k in m["launches"] if k[0] == "sn"]
    assert sum(len(g) for g in groups) == len(m["sns"])
    if "group" in c.marks:
        assert len(groups[0]) == c.marks["group"] and len({w for _, w, _ in groups[0]}) == 2      # unequal: each clips by its own w
        widest = max(groups[0], key=lambda g: g[1])
        tallest = max(groups[0], key=lambda g: g[1] + g[2])
        assert widest != tallest                               # the grid is sized by one supernode's w and the other's w + r
    if not c.marks["sns"]:
        assert m["widths"][1:].tolist() == [1] * (CC.SN_MIN_WIDTH - 1)         # the chain stays in the level lists


def test_small_tree_cases():
    for n in (CC.CH_SMALL_TREE, CC.CH_SMALL_TREE + 1):
        m = CC.model("bintree%d" % n)
        assert CC.BY_NAME["bintree%d" % n].n == n
        assert (m["trees"], m["big_cols"]) == ((1, 0) if n <= CC.CH_SMALL_TREE else (0, n))
    w = CC.model("bintree%d" % (CC.CH_SMALL_TREE + 1))["widths"].tolist()
    assert w[:4] == [256, 128, CC.CH_NARROW, 32] and w[-3:] == [1, 1, 1]
    m = CC.model("cliques")
    assert CC.BY_NAME["cliques"].marks["cliques"] == (1, 2, CC.CD_MAX - 1, CC.CD_MAX, CC.CD_MAX + 1)
    assert (m["dense"], m["trees"], m["big_cols"]) == (4, 1, 0)
    assert CC.BY_NAME["cliques"].bytes_upto == 1 + 2 + 2 * CC.CD_MAX - 1


def test_arrows_straddle_the_row_map():
    for n in (CC.CC_MAP, CC.CC_MAP + 1):
        m = CC.model("arrow%d" % n)
        assert CC.BY_NAME["arrow%d" % n].n == n and all(k[0] == "coop" and k[1] in (1, 2) for k in m["launches"][:-2])


def _edges():
    """what the table reaches: launch kinds, windows, and for every constant the values that occur"""
    kinds, windows, seen = set(), set(), {k: set() for k in ("need", "level_len", "coop_len", "width", "tree", "dense", "run0", "run1",
                                                            "coop_n", "chain", "sn_w", "sn_r", "below")}
    for name in CC.NAMES:
        c, m = CC.BY_NAME[name], CC.model(name)
        kind, window, hb = CC.decision(name)
        parent, cp = CC.symbolic(name)
        cnt = np.diff(cp)
        if "need" in c.marks:
            seen["need"].add(c.marks["need"])
        seen["tree"] |= set(np.bincount(_roots(parent))[parent < 0].tolist())
        if "cliques" in c.marks:
            seen["dense"] |= set(c.marks["cliques"])
        if kind:
            kinds.add("band%d" % kind)
            windows.add(window)
            continue
        kinds |= {"trees"} if m["trees"] else set()
        kinds |= {"dense"} if m["dense"] else set()
        member = np.zeros(c.n, bool)
        for _, a, w, r in m["sns"]:
            member[a:a + w] = True
            seen["sn_w"].add(w)
            seen["sn_r"].add(r)
        for k in m["launches"]:
            if k[0] == "sn":
                kinds.add("sn")
                seen["below"].add(max(w + r for _, w, r in k[2]) - CC.SN_NB)
                continue
            kinds.add(k[0] if k[0] == "level" else "coop%d" % k[1])
            seen["width"].add(k[-1])
            if k[0] == "level":
                seen["level_len"] |= set(cnt[(m["level"] == k[1]) & ~member].tolist())
            else:
                seen["coop_n"].add(c.n)
                seen["run1" if k[1] == 1 else "run0" if k[1] == 0 else "chain"].add(k[3] - k[2])
                if k[1] != 1:
                    lv = (m["level"] >= k[2]) & (m["level"] < k[3]) & ~member
                    seen["coop_len"] |= set(cnt[lv].tolist())
        if "sns" in c.marks and not c.marks["sns"]:
            seen["sn_w"].add(CC.SN_MIN_WIDTH - 1)
    return kinds, windows, seen


def test_the_table_is_complete():
    kinds, windows, seen = _edges()
    assert kinds == {"band1", "band2", "trees", "dense", "level", "coop0", "coop1", "coop2", "sn"}
    assert windows >= set(CC.WINDOWS)
    for w in CC.WINDOWS:                                     # both sides of every window class, 176 | 177 included
        assert {w, w + 1} <= seen["need"], w

    def both(values, limit):
        return {limit, limit + 1} <= values

    assert both(seen["level_len"], CC.CH_ACC)                # chol_column in LDS | in place, under k_chol_level
    assert both(seen["width"], CC.CH_NARROW)                 # a level for k_chol_coop | for k_chol_level
    assert both(seen["tree"], CC.CH_SMALL_TREE)
    assert both(seen["dense"], CC.CD_MAX)
    assert both(seen["coop_len"], CC.CC_ACC // CC.CC_WAVES)  # W = 16 | 15
    assert both(seen["coop_len"], CC.CC_ACC // 8)            # W = 8, the partials filling CC_ACC | W = 7
    assert both(seen["coop_n"], CC.CC_MAP)
    assert CC.CC_RUN_MIN - 1 in seen["run0"] and CC.CC_RUN_MIN in seen["run1"]
    assert CC.CC_RUN_MAX in seen["run1"] and 1 in seen["run0"]             # 64 levels in one run | the 65th in a run of its own
    assert {CC.SN_MIN_WIDTH - 1, CC.SN_MIN_WIDTH, CC.SN_NB - 1, CC.SN_NB, CC.SN_NB + 1} <= seen["sn_w"] and 0 in seen["sn_r"]
    assert both(seen["below"], CC.WB_PANEL_ROWS)
    assert CC.CC_WAVES == 16 and CC.CC_ACC == 8 * CC.CH_ACC  # (what the W = 8 | 7 cut at 1024 | 1025 rests on)


@pytest.mark.parametrize("name", [n for n in CHEAP if n in CC.ROUNDING])
def test_the_oracle_is_within_the_bound_of_a_longdouble_factor(name):
    c = CC.BY_NAME[name]
    Lp, Li, _ = CC.oracle(name)
    units = CC.rounding_units(name, "A", CC.longdouble_factor(c, c.x, Lp, Li))
    print("%s: the oracle is %.2f eps units from the longdouble factor" % (name, units))
    assert 4.0 * units <= TOL.CHOL_EPS_UNITS


@pytest.mark.parametrize("name", [n for n in CC.NAMES if n not in GRIDS])
def test_no_update_hides_inside_the_bound(name):
    """every update (a seeded sample of 10^6 where there are more) moves its entry by at least 100 x the bound"""
    small, seen, total = CC.smallest_update(name)
    print("%s: smallest update %.3e eps units (%d of %d looked at)" % (name, small, seen, total))
    assert small >= 100.0 * TOL.CHOL_EPS_UNITS


def test_the_grids_are_the_exception():
    small, _, _ = CC.smallest_update("band47")
    assert small < 1.0                                       # (see the module docstring)
