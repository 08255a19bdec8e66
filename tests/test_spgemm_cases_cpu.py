"""The table of tests/spgemm_cases.py, held to its own claims without a device: by the Python model of the host decisions in
csx_spgemm.hip every case sits on the edge it names with its neighbour across it; a limit moved by one in the model breaks some
case's claim; together the cases launch every site csx_spgemm_info counts; the probe chains of the chain cases pass from the last
slot to slot 0; the mixed values of the ordered cases would show a wrong summation order; the plain-C oracle, the pure-Python
oracle and the table's own first-touch walk agree.  The constants come from the library (csx_spgemm_limits): no device needed."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import _csx
import c_oracle as CO
import csparse_oracle as O
import spgemm_cases as SC

CUS = (256, 4)                      # an MI355X, and a device so small that every grid is cut
NAMES = SC.names()


def test_the_limits_are_the_documented_ones():
    L = SC.LIM
    assert tuple(L) == _csx.SPGEMM_LIMITS and all(isinstance(v, int) and v > 0 for v in L.values())
    assert list(SC.HASH_LIMIT) == sorted(set(SC.HASH_LIMIT)) and SC.HASH_LIMIT[-1] == SC.HASH_MAXP == SC.H1_MAXP
    assert SC.H2_MAXP == SC.H2_MAXSEG * SC.H2_MAXLEN and SC.H2_MAXP in SC.HASH_LIMIT[:SC.NNARROW]
    assert SC.SGO_MAX == SC.ORD_CLASSES[2][1] and all(s >= 2 * c for s, c, _ in SC.ORD_CLASSES)      # tables at most half full
    assert all(SC.slots_two_pass(hb) >= 2 * SC.HASH_LIMIT[hb] for hb in range(SC.NHASH))
    assert max(SC.slots_one_pass(hb) for hb in range(SC.NHASH)) < 1 << 16                            # inv[] holds slots in 16 bits
    assert L["LAUNCH_SITES"] == len(_csx.SPGEMM_SITES) and L["INFO_FIELDS"] == 40 + 2 * len(_csx.SPGEMM_SITES)
    assert _csx.load().csx_spgemm_limits(None) == _csx.EINVAL


def test_info_without_a_product_is_empty_and_bad_arguments_are_refused():
    """(a fresh process: another test of this one may have multiplied on a device)"""
    code = ("import sys; sys.path[:0] = %r; import _csx; i = _csx.spgemm_info(); "
            "assert i == {'bins': (0,) * 32, 'one_pass': 0, 'global_wgs': 0, 'cus': 0, 'ordered': 0, 'classes': (0, 0, 0, 0), "
            "'launches': {}, 'grids': {}}, i" % [os.path.dirname(_csx.__file__)])
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
    lib, C = _csx.load(), _csx.C
    out, count = (C.c_int64 * 4)(7, 7, 7, 7), C.c_int32(0)
    assert lib.csx_spgemm_info(None, 4, count) == _csx.EINVAL and lib.csx_spgemm_info(out, -1, count) == _csx.EINVAL
    assert lib.csx_spgemm_info(out, 2, count) == _csx.OK and count.value == SC.LIM["INFO_FIELDS"] and list(out)[2:] == [7, 7]
    assert lib.csx_spgemm_info(out, 4, None) == _csx.OK


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("name", NAMES)
def test_case_sits_on_its_edge(name, cus):
    case = SC.by_name(cus, name)
    f = SC.facts(case)
    assert case.edge, name
    for key, want in case.edge.items():
        if key != "grid":                                                     # (the grids: test_hand_over_cases_...)
            assert f[key] == want, (name, key)
    assert max(len(case.Ai), len(case.Bi), sum(f["cnt"])) < 600000            # (the matrices travel as Python lists)
    assert case.k <= 300 and all(np.diff(case.Bp) >= 0)


def _hand_over(cus):
    """every hand-over case has more than twice the columns its persistent grid has workgroups, by the model's grid; the
    columns a workgroup takes one after the other share some of their rows and never all of either's"""
    for case in SC.tables(cus):
        if case.family != "hand-over":
            continue
        kernel, which, G = case.edge["grid"]
        info = SC.model(case.m, case.k, case.n, case.Ap, case.Bp, case.Bi, True, cus, one_pass=kernel != "spgemm")
        site = {"hash1": "hash1_values_0", "hash2": "hash2_values_0", "spgemm": "spgemm_values_" + ("dense", "hash")[which]}[kernel]
        assert info["grids"][site] == G and case.n > 2 * G, (case.name, info["grids"], G)
        assert case.n == {"hash2": 3 * G + 2, "hash1": 2 * G + 2, "spgemm": 2 * G + 1}[kernel]
        rows = [SC.column_rows(case, j) for j in range(case.n)]
        for j in range(case.n - G):
            assert 0 < len(rows[j] & rows[j + G]) < min(len(rows[j]), len(rows[j + G])), (case.name, j)


@pytest.mark.parametrize("cus", CUS)
def test_hand_over_cases_outnumber_their_grid_and_overlap_their_predecessor(cus):
    _hand_over(cus)


def _grid_caps():
    case = SC.by_name(4, "global-reuse")
    info = SC.model(case.m, case.k, case.n, case.Ap, case.Bp, case.Bi, True, 4)
    assert case.n == 2 * SC.GLOBAL_WGS + 2 and info["global_wgs"] == info["grids"]["spgemm_values_global"] == SC.GLOBAL_WGS
    case = SC.by_name(4, "ordered-dense-map-m8192")
    Cp = SC.first_touch(case)[0]
    info = SC.model(case.m, case.k, case.n, case.Ap, case.Bp, case.Bi, True, 4, ordered=True, Cp=Cp)
    assert case.n == SC.DENSE_WAVES + 2 == info["grids"]["ordered_dense"] + 2


def _edges():
    for c in SC.tables(4):
        f = SC.facts(c)
        for k, v in c.edge.items():
            assert k == "grid" or f[k] == v, (c.name, k)


def _claims():
    """the claims of the table, each as held / broken"""
    def held(fn, *a):
        try:
            fn(*a)
            return True
        except (AssertionError, IndexError, KeyError):   # (IndexError: a column beyond the last hash bin, and no bin to take
            #                                                it; KeyError: the kernel a case is named for was not launched)
            return False
    return {"edges": held(_edges), "staging": held(test_staging_cases_cut_their_segments_where_they_say),
            "hand-over": held(_hand_over, 4), "grid caps": held(_grid_caps),
            "chains": held(test_every_table_size_is_probed_across_its_end)}


SCALARS = ["DENSE_MAX", "HASH_MAXP", "H2_MAXSEG", "H2_MAXLEN", "H2_MAXP", "SEG", "H1_SEG", "STEP", "GLOBAL_WGS", "GRID_PER_CU",
           "WGS_PER_CU_MAX", "DENSE_WAVES", "MIN_SLOTS", "LDS_BUDGET"]
MOVED = SCALARS + ["HASH_LIMIT%d" % b for b in range(SC.NHASH)] + ["SGO_CNT%d" % c for c in range(3)]


@pytest.mark.parametrize("what", MOVED)
@pytest.mark.parametrize("step", [-1, 1])
def test_a_limit_moved_by_one_breaks_some_claim(monkeypatch, what, step):
    """the cases are built from the library's constants; the model that judges them is moved.  Every constant the model decides
    by is moved: the bin, narrow and class cuts, the staging sizes, the grid caps and factors, the table sizes.  (The others
    csx_spgemm_limits hands out decide nothing in the model: SG_THREADS enters through STEP only, H1_MAXP through a byte count
    that LDS_BUDGET is divided by, H1_UN and the waves per CU of the ordered classes cut no case; the slot counts of the
    ordered classes only choose the rows of the chain cases, and with a hash that scales row * GOLDEN by the table size one
    slot more or less moves no home by more than a slot, so the rows still lie in the last eight.)"""
    if (what, step) == ("H2_MAXP", 1):
        # no column can sit on the far side of this cut: H2_MAXSEG entries of B that name columns of at most H2_MAXLEN entries
        # have at most H2_MAXSEG * H2_MAXLEN = H2_MAXP products (test_the_limits_are_the_documented_ones holds that equality)
        assert SC.H2_MAXSEG * SC.H2_MAXLEN == SC.H2_MAXP
        return
    SC.tables(4)
    if what == "LDS_BUDGET":
        # the budget only enters as budget // (LDS of a workgroup + 256), capped at WGS_PER_CU_MAX: one byte more or less
        # changes that quotient at no table size of either kernel, so no case can tell; the cap beside it is moved above
        before = [SC.one_pass_grid(kn, SC.slots_one_pass(hb), v, 1 << 30, 1) for kn in (1, 2) for hb in range(SC.NHASH) for v in (0, 1)]
        monkeypatch.setattr(SC, what, SC.LDS_BUDGET + step)
        assert before == [SC.one_pass_grid(kn, SC.slots_one_pass(hb), v, 1 << 30, 1) for kn in (1, 2) for hb in range(SC.NHASH)
                          for v in (0, 1)]
        return
    assert all(_claims().values())
    if what in SCALARS:
        monkeypatch.setattr(SC, what, getattr(SC, what) + step)
    elif what.startswith("HASH_LIMIT"):
        b = int(what[10:])
        monkeypatch.setattr(SC, "HASH_LIMIT", SC.HASH_LIMIT[:b] + (SC.HASH_LIMIT[b] + step,) + SC.HASH_LIMIT[b + 1:])
    else:
        c = int(what[7:])
        cl = list(SC.ORD_CLASSES)
        cl[c] = (cl[c][0], cl[c][1] + step, cl[c][2])
        monkeypatch.setattr(SC, "ORD_CLASSES", tuple(cl))
    broken = [k for k, ok in _claims().items() if not ok]
    assert broken, what


def _runs(case, cus):
    """the model of every run the GPU test makes of a case"""
    Cp = SC.first_touch(case)[0]
    a = (case.m, case.k, case.n, case.Ap, case.Bp, case.Bi)
    out = [SC.model(*a, True, cus), SC.model(*a, False, cus), SC.model(*a, True, cus, ordered=True, Cp=Cp)]
    if case.two_pass_too:
        out += [SC.model(*a, True, cus, one_pass=False), SC.model(*a, False, cus, one_pass=False)]
    return out


@pytest.mark.parametrize("cus", CUS)
def test_the_cases_launch_every_site(cus):
    seen = set()
    for case in SC.tables(cus):
        for info in _runs(case, cus):
            seen |= set(info["launches"])
    assert seen == set(_csx.SPGEMM_SITES), sorted(set(_csx.SPGEMM_SITES) - seen)
    assert set(SC.NOT_REACHED) == {"P just below 2^32", "more than 2^31 entries in C", "more than 2^31 products over the hash bins",
                                   "the memory-pressure fallback from one-pass"}
    big = SC.too_big_case()
    info = SC.model(big.m, big.k, big.n, big.Ap, big.Bp, big.Bi, True, cus)
    assert info["launches"] == {"products": 1} and info["one_pass"] == 0
    assert SC.column_bins(big.m, big.Ap, big.Bp, big.Bi)[0].tolist() == [1 << 32] and big.edge == {"P": [1 << 32]}


def test_every_table_size_is_probed_across_its_end():
    """replay of the insertion with the model's hashes: at least 24 distinct rows have their home in the last 8 slots of the
    table, so whatever order the device inserts them in the chain passes from the last slot to slot 0"""
    tables = set()
    for case in SC.tables(4):
        if case.family != "chains":
            continue
        f = SC.facts(case)
        hb = (f["bins"][0] - SC.BIN_HASH0) % SC.NHASH if f["bins"][0] < SC.BIN_NARROW0 else f["bins"][0] - SC.BIN_NARROW0
        todo = [("one-%s" % ("h2" if f["bins"][0] >= SC.BIN_NARROW0 else "h1"), SC.slots_one_pass(hb), SC.hash_one_pass),
                ("two", SC.slots_two_pass(hb), SC.hash_two_pass)]
        if f["classes"][0] < 3:
            todo.append(("ordered", SC.ORD_CLASSES[f["classes"][0]][0], SC.hash_ordered))
        for j in range(case.n):
            rows = [int(r) for c in case.Bi[case.Bp[j]:case.Bp[j + 1]] for r in case.Ai[case.Ap[c]:case.Ap[c + 1]]]
            for kind, slots, home in todo:
                h = home(np.asarray(rows), slots)
                assert len(set(np.asarray(rows)[h >= slots - 8].tolist())) >= 24 and (h == 0).any(), (case.name, kind)
                where = SC.insert(rows, slots, home)
                wrapped = {r for r, hr in zip(rows, h.tolist()) if hr >= slots - 8 and where[r] < hr}
                assert len(wrapped) >= 16 and max(where.values()) == slots - 1, (case.name, kind, slots)
                tables.add((kind, slots))
    want = {("one-h1", SC.slots_one_pass(hb)) for hb in range(SC.NHASH)} | {("one-h2", SC.slots_one_pass(hb)) for hb in range(SC.NNARROW)}
    want |= {("two", SC.slots_two_pass(hb)) for hb in range(SC.NHASH)} | {("ordered", s) for s, _, _ in SC.ORD_CLASSES}
    assert want <= tables


def test_staging_cases_cut_their_segments_where_they_say():
    f = SC.facts(SC.by_name(4, "staging-hash"))
    segs = [f["seg_products"](j) for j in range(13)]
    assert [s[0] for s in segs[8:11]] == [SC.STEP - 1, SC.STEP, SC.STEP + 1]          # a step of products | one more
    assert segs[11][1] == 0 and segs[11][0] > 0 and segs[11][2] > 0                   # a segment without products between live ones
    assert [len(s) for s in segs[:8]] == [1, 1, 1, 1, 1, 1, 2, 3]
    f = SC.facts(SC.by_name(4, "h1-zero-lengths"))
    assert f["h1_seg_products"](2)[1] == 0 and len(f["h1_seg_products"](2)) == 3
    f = SC.facts(SC.by_name(4, "staging-global"))
    assert f["seg_products"](1)[1] == 0 and min(f["P"]) > SC.HASH_MAXP


def test_global_columns_on_one_workgroup_share_half_their_rows_at_other_product_numbers():
    case = SC.by_name(4, "global-reuse")
    G = SC.GLOBAL_WGS

    def touched(j):                                   # row -> product number of its first touch
        t, out = 0, {}
        for c in case.Bi[case.Bp[j]:case.Bp[j + 1]]:
            for r in case.Ai[case.Ap[c]:case.Ap[c + 1]].tolist():
                out.setdefault(r, t)
                t += 1
        return out
    for j in range(case.n - G):
        a, b = touched(j), touched(j + G)
        shared = set(a) & set(b)
        assert 0.3 < len(shared) / len(a) < 0.7, j
        assert sum(a[r] != b[r] for r in shared) > 0.9 * len(shared), j


def _oracle(case, Ax, Bx):
    return CO.multiply(case.m, case.k, case.n, case.Ap, case.Ai, Ax, case.Bp, case.Bi, Bx)


@pytest.mark.parametrize("name", NAMES)
def test_the_oracles_agree_on_the_pattern_and_on_small_cases_the_values(name):
    case = SC.by_name(4, name)
    Ax, Bx = SC.values_for(case, "mixed")
    Cp, Ci, Cx = _oracle(case, Ax, Bx)
    fp, fi, terms = SC.first_touch(case)
    assert Cp.tolist() == fp.tolist() and Ci.tolist() == fi.tolist()
    if terms.sum() > 20000:
        return

    def host(m, n, p, i, x):
        A = O.cs_spalloc(m, n, max(len(i), 1), True, False)
        A.p, A.i, A.x = p.tolist(), i.tolist() + [0] * (A.nzmax - len(i)), x.tolist() + [0.0] * (A.nzmax - len(i))
        return A
    Cr = O.cs_multiply(host(case.m, case.k, case.Ap, case.Ai, Ax), host(case.k, case.n, case.Bp, case.Bi, Bx))
    nnz = int(Cp[-1])
    assert Cr.p == Cp.tolist() and Cr.i[:nnz] == Ci.tolist()
    assert np.asarray(Cr.x[:nnz]).tobytes() == Cx.tobytes()


def test_the_exact_reference_is_the_sum_of_fractions():
    case = SC.by_name(4, "ordered-equal-rows-m8192")
    Ax, Bx = SC.values_for(case, "mixed")
    sums, mags, terms = SC.exact_entries(case, Ax, Bx)
    at = 0
    for j in range(case.n):
        ref, order = {}, []
        for p in range(case.Bp[j], case.Bp[j + 1]):
            for q in range(case.Ap[case.Bi[p]], case.Ap[case.Bi[p] + 1]):
                r = int(case.Ai[q])
                if r not in ref:
                    ref[r] = [Fraction(0), Fraction(0), 0]
                    order.append(r)
                t = Fraction(float(Ax[q])) * Fraction(float(Bx[p]))
                ref[r][0] += t
                ref[r][1] += abs(t)
                ref[r][2] += 1
        for r in order:
            assert (sums[at], mags[at], terms[at]) == tuple(ref[r])
            at += 1
    assert at == len(sums)
    # the bound itself: a correctly rounded sum passes, one that lost its smallest product does not
    ok, _ = SC.within_bound(float(sums[0]), sums[0], mags[0], terms[0])
    assert ok and SC.gamma(3) == Fraction(3, 2 ** 53 - 3)
    k = max(range(len(sums)), key=lambda e: terms[e])
    assert not SC.within_bound(float(sums[k]) + 2.0 ** -40, sums[k], mags[k], terms[k])[0]


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("ordered-")])
def test_mixed_values_of_the_ordered_cases_show_the_order(name):
    """at least a quarter of the entries with three or more products change bits when their products are added in reverse"""
    case = SC.by_name(4, name)
    Ax, Bx = SC.values_for(case, "mixed")
    Cp, Ci, Cx = _oracle(case, Ax, Bx)
    terms = SC.first_touch(case)[2]
    rev_b = np.concatenate([np.arange(case.Bp[j], case.Bp[j + 1])[::-1] for j in range(case.n)]).astype(np.int64)
    rev_a = np.concatenate([np.arange(case.Ap[c], case.Ap[c + 1])[::-1] for c in range(case.k)]).astype(np.int64)
    Rp, Ri, Rx = CO.multiply(case.m, case.k, case.n, case.Ap, case.Ai[rev_a], Ax[rev_a], case.Bp, case.Bi[rev_b], Bx[rev_b])
    changed = total = 0
    for j in range(case.n):
        fwd = dict(zip(Ci[Cp[j]:Cp[j + 1]].tolist(), zip(Cx[Cp[j]:Cp[j + 1]].tolist(), terms[Cp[j]:Cp[j + 1]].tolist())))
        for r, x in zip(Ri[Rp[j]:Rp[j + 1]].tolist(), Rx[Rp[j]:Rp[j + 1]].tolist()):
            if fwd[r][1] >= 3:
                total += 1
                changed += fwd[r][0] != x
    assert total > 0 and changed >= total / 4, (name, changed, total)
