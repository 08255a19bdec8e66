"""The table of tests/block_cases.py held to its claims without a device: every case sits on the side of its cut it says (by a
union-find and the cuts the library hands out, csx_block_limits) with its neighbour across; csx_lu_host -- what the device route is
compared with in tests/test_gpu_block_factor.py -- has the oracle's bits on every LU case, and both give None on every singular
one; the tie cases tie; the QR cases have m2 == n and the tail2 == 0 cases give beta 0 or 2 exactly; the csx_happly cases have the
levels, and so the route, they claim."""
import numpy as np
import pytest

import _csx
import block_cases as BC
from test_lu_oracle import host_lu, oracle_lu, same


def test_limits_come_from_the_library_without_a_device():
    assert tuple(BC.LIM) == _csx.BLOCK_LIMITS and all(isinstance(v, int) and v > 0 for v in BC.LIM.values())
    assert _csx.load().csx_block_limits(None) == _csx.EINVAL
    # the table is built on one pair of cuts for both routes
    assert (BC.QR_MAX_M, BC.QR_MIN_COMPONENTS) == (BC.LU_MAX_M, BC.LU_MIN_COMPONENTS)
    # 25 B per row and lane (x 8, reach / stack / pos / pinv 4 each, seen 1) + 64 must fit what k_lu_blocks asks the device for
    assert BC.LU_MAX_M * BC.WAVE * 25 + 64 <= 160 * 1024 - 256


def test_prim_components_refuses_bad_pointers_before_the_device():
    lib, C = _csx.load(), _csx.C
    out = [np.zeros(4, np.int32) for _ in range(4)]
    nodes = np.zeros(4, np.uint32)
    nc, mc, bad = C.c_int32(0), C.c_int32(0), C.c_int(0)

    def call(n, p, i, sf=0, sl=0, order=0, root=out[0]):
        p, i = np.asarray(p, np.int32), np.asarray(i, np.int32)
        return lib.csx_prim_components(n, _csx.pi(p), _csx.pi(i), sf, sl, order, _csx.pi(root), nodes.ctypes.data_as(C.c_void_p),
                                       _csx.pi(out[1]), _csx.pi(out[2]), _csx.pi(out[3]), C.byref(nc), C.byref(mc), C.byref(bad))

    assert call(-1, [0], [0]) == _csx.EINVAL
    assert call(2, [1, 1, 2], [0, 1]) == _csx.EINVAL                      # p[0] != 0
    assert call(2, [0, 2, 1], [0, 1]) == _csx.EINVAL                      # p decreases
    assert call(2, [0, 1, 2], [0, 1], sf=2) == _csx.EINVAL
    assert call(2, [0, 1, 2], [0, 1], sl=-1) == _csx.EINVAL
    assert call(2, [0, 1, 2], [0, 1], order=3) == _csx.EINVAL
    assert call(2, [0, 1, 2], [0, 1], root=None) == _csx.EINVAL
    assert lib.csx_prim_components(2, None, None, 0, 0, 0, *([None] * 8)) == _csx.EINVAL
    assert call(0, [0], []) == _csx.OK and (nc.value, mc.value, bad.value) == (0, 0, 0)     # nothing to do: no device either


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_sits_on_its_edge(name):
    c, M = BC.CASES[name], BC.get(name)
    f = BC.facts(M["n"], M["Ap"], M["Ai"])
    for key, want in c["claims"].items():
        if key in f:
            assert f[key] == want, (name, key, f[key], want)
    if c["other"]:
        O = BC.get(c["other"])
        g = BC.facts(O["n"], O["Ap"], O["Ai"])
        assert f[c["cut"]] != g[c["cut"]], (name, c["other"], c["cut"])
        assert BC.CASES[c["other"]]["claims"].get("route") == g["route"]
    if "mems" in M:                                                       # the components are the blocks the case was built from
        want = np.empty(M["n"], np.int32)
        for mem in M["mems"]:
            want[mem] = mem.min()
        assert np.array_equal(f["root"], want), name
    if "target" in c["claims"]:                                           # the singular block is component 0 / the last lane
        lows = sorted(int(mem[0]) for mem in M["mems"])
        assert lows.index(int(M["mems"][M["target"]][0])) == c["claims"]["target"]
    finite = np.isfinite(M["Ax"])
    assert finite.all() or name.startswith("sing_nan_")


def _columns(M):
    return [(M["Ai"][a:b], M["Ax"][a:b]) for a, b in zip(M["Ap"][:-1], M["Ap"][1:])]


def test_the_special_shapes_are_what_they_say():
    M = BC.get("wave_96_and_ones")
    counts = BC.facts(M["n"], M["Ap"], M["Ai"])["counts"]
    big = int(np.argmax(counts))
    assert counts[big] == BC.MAX_M and 0 < big < len(counts) - 1 and (np.delete(counts, big) == 1).all()
    M = BC.get("stride_members")
    root = BC.roots(M["n"], M["Ap"], M["Ai"])
    assert np.array_equal(root, np.arange(M["n"]) % 70)
    M = BC.get("root_via_last")
    cols = _columns(M)
    col_of = np.repeat(np.arange(M["n"]), np.diff(M["Ap"]))
    for mem in M["mems"]:
        v, last = int(mem[0]), int(mem[-1])
        assert cols[v][0].tolist() == [v]                                 # only the diagonal in its column
        assert sorted(col_of[M["Ai"] == v].tolist()) == [v, last]         # reached through A(v, last) alone
    M = BC.get("halves_one_link")
    i, j = M["link"]
    cols = _columns(M)
    assert i in cols[j][0] and j not in cols[i][0]
    Ai = M["Ai"].copy()
    Ai[M["Ap"][j] + int(np.flatnonzero(cols[j][0] == i)[0])] = j          # without the link: two halves
    h = BC.facts(M["n"], M["Ap"], Ai)
    assert h["ncomp"] == BC.MIN_C + 2 and h["maxc"] == BC.MAX_M // 2
    path = BC.get("path_scrambled")
    deg = np.diff(path["Ap"]) - 1                                         # (without the diagonal)
    assert all(sorted(deg[mem].tolist()) == [1, 1] + [2] * (len(mem) - 2) for mem in path["mems"])
    ends_first = sum(deg[mem[0]] == 1 and deg[mem[-1]] == 1 for mem in path["mems"])
    assert ends_first < len(path["mems"]) // 2                            # the labelling does not follow the path
    star = BC.get("star_scrambled")
    deg = np.diff(star["Ap"]) - 1
    assert all(int(np.argmax(deg[mem])) != 0 and deg[mem].max() == len(mem) - 1 for mem in star["mems"])   # centre not the smallest
    cols = _columns(BC.get("storage_desc"))
    assert all((np.diff(r) < 0).all() for r, _ in cols) and any(len(r) > 2 for r, _ in cols)
    cols = _columns(BC.get("storage_shuffled"))
    assert any((np.diff(r) < 0).any() and (np.diff(r) > 0).any() for r, _ in cols)
    ndup = 0
    for r, x in _columns(BC.get("storage_dups")):
        for row in np.unique(r):
            vals = x[r == row]
            assert len(vals) <= 2
            if len(vals) == 2:
                assert vals[0] != vals[1]
                ndup += 1
    assert ndup > 100
    M = BC.get("no_diagonal")
    assert all(j not in r for j, (r, _) in enumerate(_columns(M)))
    for name in BC.SINGULAR_CASES:
        M = BC.get(name)
        v1 = int(M["mems"][M["target"]][1])
        r, x = _columns(M)[v1]
        if "_empty_" in name:
            assert len(r) == 0
        elif "_zero_" in name:
            assert x.tolist() == [0.0]
        elif "_nan_" in name:
            assert len(x) >= 2 and np.isnan(x).all() and np.isnan(M["Ax"]).sum() == len(x)
        else:
            r0, x0 = _columns(M)[int(M["mems"][M["target"]][0])]
            assert r.tolist() == r0.tolist() and x.tolist() == x0.tolist() and set(np.abs(x).tolist()) <= {1.0, 2.0}


@pytest.mark.parametrize("name,tol", BC.LU_CASES)
def test_host_lu_has_the_oracles_bits(name, tol):
    M = BC.get(name)
    ref = oracle_lu(M["n"], M["Ap"], M["Ai"], M["Ax"], tol)
    same(host_lu(M["n"], M["Ap"], M["Ai"], M["Ax"], tol), ref)
    if name == "row_k_taken_early":
        pinv = ref[6]
        assert (pinv < np.arange(M["n"])).sum() >= 70                     # rows that are pivotal before their own column comes


@pytest.mark.parametrize("name", BC.SINGULAR_CASES)
def test_singular_cases_give_none_twice(name):
    M = BC.get(name)
    assert host_lu(M["n"], M["Ap"], M["Ai"], M["Ax"], 1.0) is None
    assert oracle_lu(M["n"], M["Ap"], M["Ai"], M["Ax"], 1.0) is None
    # the block alone is what is singular: with the target's column repaired by a strong diagonal both codes factor
    t = M["mems"][M["target"]]
    keep = np.repeat(np.arange(M["n"]), np.diff(M["Ap"])) != int(t[1])
    Ai = np.concatenate([M["Ai"][keep], [int(t[1])]]).astype(np.int32)
    Ax = np.concatenate([M["Ax"][keep], [7.0]])
    cols = np.concatenate([np.repeat(np.arange(M["n"]), np.diff(M["Ap"]))[keep], [int(t[1])]])
    order = np.argsort(cols, kind="stable")
    Ap = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M["n"]))]).astype(np.int32)
    assert host_lu(M["n"], Ap, Ai[order], Ax[order], 1.0) is not None


@pytest.mark.parametrize("name", BC.TIE_CASES)
def test_tie_cases_really_tie(name):
    M = BC.get(name)
    n, Ap, Ai, Ax = M["n"], M["Ap"], M["Ai"], M["Ax"]
    pinv = oracle_lu(n, Ap, Ai, Ax, 1.0)[6]
    mem = M["mems"][0]
    for r, c in BC.TIE_BREAKERS:
        rows = Ai[Ap[mem[c]]:Ap[mem[c] + 1]]
        q = int(Ap[mem[c]]) + int(np.flatnonzero(rows == mem[r])[0])
        Bx = Ax.copy()
        Bx[q] *= 1.0 + 2.0 ** -40
        other = oracle_lu(n, Ap, Ai, Bx, 1.0)[6]
        assert other[mem].tolist() != pinv[mem].tolist(), (r, c)          # the later candidate now wins: it was a tie
        rest = np.setdiff1d(np.arange(n), mem)
        assert other[rest].tolist() == pinv[rest].tolist()


def host_qr(n, Ap, Ai, Ax):
    """(S, Vp, Vi, Vx, Rp, Ri, Rx, beta) of csx_qr_host on the product's own analysis (cs_sqr, host code)"""
    import csparse as cs
    A = cs.cs_spalloc(n, n, max(len(Ai), 1), True, False)
    A.p, A.i, A.x = Ap.tolist(), Ai.tolist(), Ax.tolist()
    S = cs.cs_sqr(0, A, True)
    assert S is not None
    parent, pinv, leftmost = _csx.i32(S.parent), _csx.i32(S.pinv), _csx.i32(S.leftmost)
    vcap, rcap = max(int(S.lnz), 1), max(int(S.unz), 1)
    Vp, Rp = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    Vi, Ri = np.zeros(vcap, np.int32), np.zeros(rcap, np.int32)
    Vx, Rx, beta = np.zeros(vcap), np.zeros(rcap), np.zeros(n)
    st = _csx.load().csx_qr_host(n, n, S.m2, _csx.pi(Ap), _csx.pi(Ai), _csx.pd(Ax), None, _csx.pi(parent), _csx.pi(pinv),
                                 _csx.pi(leftmost), vcap, rcap, _csx.pi(Vp), _csx.pi(Vi), _csx.pd(Vx), _csx.pi(Rp),
                                 _csx.pi(Ri), _csx.pd(Rx), _csx.pd(beta))
    assert st == 0
    return S, Vp, Vi[:Vp[n]], Vx[:Vp[n]], Rp, Ri[:Rp[n]], Rx[:Rp[n]], beta


@pytest.mark.parametrize("name", BC.QR_CASES)
def test_qr_cases_have_no_fictitious_rows(name):
    M = BC.get(name)
    S, Vp, Vi, Vx, Rp, Ri, Rx, beta = host_qr(M["n"], M["Ap"], M["Ai"], M["Ax"])
    assert S.m2 == M["n"] and S.q is None
    if BC.CASES[name]["claims"].get("tail2_zero"):
        assert np.array_equal(np.diff(Vp), np.ones(M["n"]))               # nothing below any diagonal
        assert set(beta.tolist()) == {0.0, 2.0}
        # beta is 2 exactly where the head of the column, after the sign flips of the reflections before it, is <= 0; all four
        # heads occur: R's diagonal is 0 under some beta = 2 (head +-0.0) and positive under others (head < 0), also under beta = 0
        rdiag = Rx[Rp[1:] - 1]
        assert ((beta == 2.0) & (rdiag == 0.0)).sum() >= 8 and ((beta == 2.0) & (rdiag > 0.0)).sum() >= 8
        assert ((beta == 0.0) & (rdiag > 0.0)).sum() >= 8 and not ((beta == 0.0) & (rdiag == 0.0)).any()
        zeros = M["Ax"][(M["Ax"] == 0.0)]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()    # +0.0 and -0.0 are both stored


    if BC.CASES[name]["claims"].get("zero_head"):
        differ = 0
        for mem in M["mems"]:
            j = int(mem[0])
            assert M["Ax"][M["Ap"][j]] == 0.0 and Vp[j + 1] - Vp[j] >= 3 and Rp[j + 1] - Rp[j] == 1
            tail2 = 0.0
            for p in range(Vp[j] + 1, Vp[j + 1]):
                tail2 = tail2 + float(Vx[p]) * float(Vx[p])
            s = float(np.sqrt(tail2))
            assert Rx[Rp[j]] == s and Vx[Vp[j]] == -s                     # head - s with head = +-0.0
            differ += (-tail2 / (0.0 + s)) != -s                          # what the other branch would have stored
        assert differ >= 8


@pytest.mark.parametrize("name", list(BC.HAPPLY_CASES))
def test_happly_cases_have_the_levels_they_claim(name):
    M = BC.happly_matrix(name)
    _, nlevels, route = BC.HAPPLY_CASES[name]
    S, Vp, Vi = host_qr(M["n"], M["Ap"], M["Ai"], M["Ax"])[:3]
    got = BC.house_levels(M["n"], Vp, Vi, S.m2)
    if nlevels is not None:
        assert got == nlevels
    else:
        assert 1 < got < M["n"] and M["n"] / got > 10                    # many reflections to a level
    assert BC.happly_route(got, M["n"]) == route
    assert BC.route(**{k: BC.facts(M["n"], M["Ap"], M["Ai"])[k] for k in ("n", "ncomp", "maxc")}) == \
        ("device" if name == "ncomp_65" else "host")


@pytest.mark.parametrize("name", list(BC.COMPONENT_CASES))
def test_component_cases_are_malformed_exactly_where_they_say(name):
    n, Ap, Ai, sf, sl, order, malformed = BC.component_case(name)
    bad = False
    for r in range(n):
        idx = Ai[Ap[r] + sf:max(Ap[r + 1] - sl, Ap[r] + sf)]
        bad |= bool(((idx < 0) | (idx >= n)).any()) or (order == 1 and bool((idx >= r).any())) or (order == 2 and bool((idx <= r).any()))
    assert bad == malformed
    if not malformed:
        _, _, _, _, ncomp, maxc = BC.grouping(BC.roots(n, Ap, Ai, sf, sl))
        if name in ("comp_long_path", "comp_one_star", "comp_n1", "comp_n1_empty"):
            assert (ncomp, maxc) == (1, n)
        if name == "comp_no_entries":
            assert (ncomp, maxc) == (n, 1)
        if name in ("comp_lower_order2", "comp_upper_order1"):           # a triangle has the components of the whole pattern
            full = BC.get("stride_members" if "lower" in name else "path_scrambled")
            assert np.array_equal(BC.roots(n, Ap, Ai, sf, sl), BC.roots(n, full["Ap"], full["Ai"]))


def test_not_reached_gives_its_reasons():
    assert all(len(why) > 40 for why in BC.NOT_REACHED.values())
