"""The table of tests/tri_cases.py, held to its own claims without a device: by the Python model of tri_route, make_segments and
walk_levels every case takes the route and launches the kernel instances it is named for, sits on the edge it declares and has
its neighbour on the other side; together the cases launch every instance csx_tri_launches counts (or the table says why not);
every matrix is a proper triangle of its kind, or deliberately not; and the values are diagonally dominant by rows and by columns.
The constants come from the library (csx_tri_limits), which needs no device."""
import numpy as np
import pytest

import _csx
import tri_cases as TC

LIM = TC.LIM


def _fact(case, value):
    return value[0 if case.kind in TC.PUSH else 1] if isinstance(value, tuple) else value


def test_the_limits_are_the_documented_ones():
    assert set(LIM) == set(_csx.TRI_LIMITS) and LIM["LAUNCH_COUNTERS"] == len(_csx.TRI_LAUNCHES)
    assert all(isinstance(v, int) and v > 0 for v in LIM.values())
    assert LIM["TRW_MAX_RHS"] + 1 == LIM["TR64_MIN_RHS"]          # no count of right-hand sides between the two wave flavours
    assert LIM["CHB"] - 1 <= LIM["CH_SUF"]                         # the relaxed walker's staging holds a row's in-block sources
    assert _csx.load().csx_tri_limits(None) == _csx.EINVAL


@pytest.mark.parametrize("cid", TC.IDS)
def test_case_takes_its_route_on_its_edge(cid):
    case = TC.BY_ID[cid]
    info, launches = TC.predicted(cid)
    assert info["route"] == case.route, (cid, info)
    assert set(launches) == set(case.must), (cid, launches)
    for key, want in case.facts.items():
        assert info[key] == _fact(case, want), (cid, key, info[key])
    assert info["kind"] == TC.KIND_ID[case.kind] and info["n"] == TC.matrix(case)[0]


# (an edge inside a kernel or inside analyse shows in no decision: the cases with a `check` of their own have a test of their own below)
@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.other and c.check not in ("remainder", "strip")])
def test_the_neighbour_is_on_the_other_side(cid):
    case = TC.BY_ID[cid]
    others = [c for c in TC.CASES if c.name == case.other and c.kind == case.kind] or \
        [c for c in TC.CASES if c.name == case.other and (c.kind in TC.PUSH) == (case.kind in TC.PUSH)]     # or of its group
    assert others, (cid, case.other)
    for o in others:
        a, b = TC.predicted(cid), TC.predicted(o.id)
        decided = ("route", "window", "threads", "rounds", "levels", "schedule", "ncomp", "waves", "tile_rows", "chunks", "lds",
                   "chain_ok")
        if case.system == o.system and case.nrhs != o.nrhs and a[0]["route"] == "Levels":
            # the same matrix on the level walk: the edge is a second block of 64 lanes inside the walker
            assert (case.nrhs - 1) // 64 != (o.nrhs - 1) // 64, (cid, o.id)
            continue
        assert a[1] != b[1] or any(a[0][k] != b[0][k] for k in decided), (cid, o.id)


def test_every_kernel_instance_is_launched_by_some_case():
    reached = set()
    for cid in TC.IDS:
        reached |= set(TC.predicted(cid)[1])
    routes = {TC.predicted(cid)[0]["route"] for cid in TC.IDS}
    assert routes == set(_csx.TRI_ROUTES) - {"Ragged"} and reached == set(_csx.TRI_LAUNCHES) - {"ragged"}     # the exact order
    for r in TC.ROUNDING:                                                                                     # the rounding-equal one
        info, launches, _ = TC.model(TC.rounding_matrix(r.id), r.kind, r.nrhs, guard=r.guard)
        reached |= set(launches)
        routes.add(info["route"])
    assert not reached & set(TC.UNREACHED)
    assert reached | set(TC.UNREACHED) == set(_csx.TRI_LAUNCHES), set(_csx.TRI_LAUNCHES) - reached - set(TC.UNREACHED)
    assert routes == set(_csx.TRI_ROUTES)


@pytest.mark.parametrize("key", sorted({(c.system, c.kind, c.seed, c.spoil) for c in TC.CASES} |
                                        {(r.system, r.kind, r.seed, None) for r in TC.ROUNDING}, key=str))
def test_matrix_is_a_triangle_of_its_kind_and_dominant(key):
    n, Tp, Ti, Tx = TC._matrix(*key)
    lower = key[1] in ("lsolve", "ltsolve")
    Tp64 = Tp.astype(np.int64)
    col = np.repeat(np.arange(n), np.diff(Tp64))
    diag = np.zeros(len(Ti), bool)
    diag[Tp64[:-1] if lower else Tp64[1:] - 1] = True
    assert np.all(np.diff(Tp64) >= 1) and np.array_equal(Ti[diag], np.arange(n))
    proper = bool(np.all((Ti[~diag] > col[~diag]) if lower else (Ti[~diag] < col[~diag])))
    assert proper == (key[3] is None)
    assert np.all(np.abs(Tx[diag]) >= 1.0) and np.all(np.abs(Tx[diag]) <= 2.0)
    by_row = np.bincount(Ti[~diag], weights=np.abs(Tx[~diag]), minlength=n)
    by_col = np.bincount(col[~diag], weights=np.abs(Tx[~diag]), minlength=n)
    assert by_row.max(initial=0.0) <= 0.5 + 1e-12 and by_col.max(initial=0.0) <= 0.5 + 1e-12
    if key[3] is None and n <= 4000 and key[1] in TC.PUSH:          # somewhere the rows of a column are NOT sorted
        lens = np.diff(Tp64)
        if lens.max() >= 4:
            assert any(np.any(np.diff(Ti[Tp64[j] + (1 if lower else 0):Tp64[j + 1] - (0 if lower else 1)]) < 0)
                       for j in np.flatnonzero(lens >= 4))


@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.check == "runs" and c.nrhs in (1, 64)])
def test_runs_of_narrow_levels_and_the_three_prefix_outcomes(cid):
    case = TC.BY_ID[cid]
    P = TC.plan_model(case)
    runs = P.runs(case.nrhs)
    lengths = [(b - a, two) for a, b, two in runs]
    lo, run = LIM["TR64_RUN_MIN"], LIM["TR64_RUN"]
    assert lengths == [(lo - 1, False), (lo, True), (run, True), (run, True), (1, False)], lengths
    a, b, _ = runs[1]
    stops = P.prefix_stops(a, b)
    assert any(stop == 0 and terms > 0 for _, stop, terms in stops)            # resumes at the row's start
    assert any(stop == terms and terms > 0 for _, stop, terms in stops)        # no term inside the run: the walker only divides
    assert any(stop == 64 and terms > 64 for _, stop, terms in stops)          # stops on a block boundary
    lens = set(np.diff(P.ptr).tolist())
    assert {0, 1, 8, 9, 16, 17, 48, 49, 64, 65, 128, 129} <= lens
    mean = LIM["TRW_MIN_ROW"] * P.n
    assert P.gnnz == mean
    other = TC.plan_model(next(c for c in TC.CASES if c.name == case.other and c.kind == case.kind))
    assert other.gnnz == mean - 1


@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.check == "unaligned"])
def test_chain_segment_starts_inside_a_block(cid):
    case = TC.BY_ID[cid]
    P = TC.plan_model(case)
    segs = P.segments(case.nrhs)
    assert [s[2] for s in segs] == [False, True]
    p0 = int(P.level_ptr[segs[1][0]])
    blk = p0 & ~(LIM["CHB"] - 1)
    assert blk < p0
    pos_of = np.empty(P.n, np.int64)
    pos_of[P.order] = np.arange(P.n)
    reads = [pos_of[P.idx[P.ptr[r]:P.ptr[r + 1]]] for r in P.order[p0:p0 + LIM["CHB"] - (p0 - blk)]]
    assert any(np.any((s >= blk) & (s < p0)) for s in reads)      # a row of the segment reads a row the wide launch solved


@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.check == "remainder"])
def test_longest_remainder_of_the_chain_walker(cid):
    case = TC.BY_ID[cid]
    P = TC.plan_model(case)
    want = LIM["CH_SUF"] + (1 if case.name.endswith("33") else 0)
    assert int((np.diff(P.ptr) - P.npre).max()) == want


@pytest.mark.parametrize("cid", [c.id for c in TC.CASES if c.check == "strip"])
def test_strip_cases_sit_on_the_column_length_cut(cid):
    case = TC.BY_ID[cid]
    n, Tp = TC.matrix(case)[:2]
    assert int(Tp[n]) == LIM["STRIP_SHORT_COLS"] * n - (1 if case.name == "strip_short" else 0)


def test_model_of_the_pairs_of_the_fused_lu_solve():
    for name, sl, su, nrhs, fused in TC.LU_PAIRS:
        L, U = TC.to_matrix(TC._system(sl), "lsolve", 1), TC.to_matrix(TC._system(su), "usolve", 2)
        assert L[0] == U[0]
        routes = (TC.model(L, "lsolve", nrhs)[0]["route"], TC.model(U, "usolve", nrhs)[0]["route"])
        assert (routes == ("Local", "Local")) == fused, (name, routes)
        routes = (TC.model(U, "utsolve", nrhs)[0]["route"], TC.model(L, "ltsolve", nrhs)[0]["route"])
        assert (routes == ("Local", "Local")) == fused, (name, routes)


def test_rounding_cases_by_the_model_and_the_guards_three_outcomes():
    assert {r.guard for r in TC.ROUNDING} == {0, 1, 2, 3}
    for r in TC.ROUNDING:
        info, launches, _ = TC.model(TC.rounding_matrix(r.id), r.kind, r.nrhs, guard=r.guard)
        assert info["route"] == r.route and set(launches) == set(r.must), (r.id, info, launches)
        assert (info["guard"] != 0) == (r.nrhs > LIM["PUSH_MAX_RHS"])
        assert info["comp_max"] <= 80 or r.guard == 2
    sizes = set(TC._RAG_SIZES)
    assert {16, 17, 32, 33, 48, 49, 64, 65, 80} <= sizes            # both sides of every size class of the matrix-core sweep


def test_the_bound_of_the_rounding_equal_order_comes_from_the_oracle_column():
    import json
    import os

    import tol as TOL
    from conftest import ROOT
    rows = [json.loads(line) for line in open(os.path.join(ROOT, "profiles", "trisolve_edges.jsonl"))]
    assert [row["case"] for row in rows] == TC.ROUNDING_MEASURED + list(TC.PAIRS)
    worst = max(rows, key=lambda row: row["oracle_eps_units"])
    assert abs(TOL.TRI_EPS_UNITS - 4 * worst["oracle_eps_units"]) < 1e-3
    assert abs(TC.oracle_eps_units(worst["case"]) - worst["oracle_eps_units"]) < 1e-9     # and the column is reproducible
    for name in TC.PAIRS:
        assert abs(TC.pair_oracle_units(name) - next(r for r in rows if r["case"] == name)["oracle_eps_units"]) < 1e-9
    assert all(row["device_eps_units"] is not None for row in rows)                        # filled by a run on a device


@pytest.mark.parametrize("name", ["col15360", "wlong"])
def test_gathered_columns_sit_on_every_count_of_the_product_chain(name):
    """tch_chain_lds leaves its loop after 16, 32 and 48 products and wraps its prefetch at 64; k_tri_colchain and
    k_tri_wcolchain<., 2> hold two rounds of 64 entries of a column ahead"""
    lens = set(len(s) for s in TC._system(name).src)
    assert {0, 1, 2, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193} <= lens
