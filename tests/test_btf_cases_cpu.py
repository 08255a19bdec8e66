"""The table of tests/btf_cases.py held to its claims without a device: the intended blocks are the strong components and have the
levels they say; every claim follows from the model (csx_btf_plan, csx_btf_info and refactor_build restated, the cuts handed out by
csx_btf_limits); every cut pair differs in the named fact alone; the table as a whole holds every block size, term count, F count,
level mix and group count the device test is there for; and every case is admitted by the CPU restatements alone: factored by
csx_lu_host in the intended order, solved forward and transposed by btf_oracle / trans_oracle below the backward-error bound, and,
for the refactor cases, with new values that pivot as the old ones do."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import _csx
import btf_cases as BC
import btf_oracle
import refactor_oracle
import trans_oracle
from test_lu_oracle import host_lu


def test_limits_come_from_the_library_without_a_device():
    assert tuple(BC.LIM) == _csx.BTF_LIMITS and all(isinstance(v, int) and v > 0 for v in BC.LIM.values())
    assert _csx.load().csx_btf_limits(None) == _csx.EINVAL
    # "csx_lu_blocks' limit": a block the solve keeps in LDS and a group the refactor keeps on the device are what cs_lu's block
    # route takes
    assert BC.BTF_SMALL == BC.RF_MAX == _csx.block_limits()["LU_MAX_M"]
    assert BC.RHS_TILE == BC.TERM_CHUNK == 64                      # one lane per right-hand side and per loaded term
    assert BC.TERM_CHUNK % BC.TERM_GROUP == 0
    assert BC.BTF_SMALL * BC.RHS_TILE * 8 <= 64 * 1024            # the largest tile k_btf_small asks for without opting in to more
    assert BC.BTF_SMALL > BC.TERM_CHUNK + 1                        # a small block can hold a row of more than one chunk


def _split(M, S0):
    """D and F of S0 in the intended order (p = q = the identity) as sorted CSC"""
    bof = np.repeat(np.arange(len(M["sizes"])), M["sizes"])
    C = S0.tocoo()
    inside = bof[C.row] == bof[C.col]
    assert np.all(bof[C.row[~inside]] < bof[C.col[~inside]])       # block upper triangular
    out = []
    for keep in (inside, ~inside):
        X = sp.csc_matrix((C.data[keep], (C.row[keep], C.col[keep])), shape=S0.shape)
        X.sort_indices()
        out.append(X)
    return out


def _lu(D, tol):
    return host_lu(D.shape[0], D.indptr.astype(np.int32), D.indices.astype(np.int32), D.data.astype(np.float64), tol)


def _t(X):
    return (X.indptr, X.indices, X.data)


@functools.lru_cache(maxsize=None)
def cpu_factors(name):
    M = BC.get(name)
    D, F = _split(M, M["S0"])
    f = _lu(D, M["tol"])
    assert f is not None
    return D, F, f


def backward_error(S, x, b):
    return np.max(np.abs(S @ x - b)) / (abs(S).sum(axis=1).max() * np.max(np.abs(x)) + np.max(np.abs(b)))


def _counts(name):
    D, F, f = cpu_factors(name)
    return BC.term_counts(f[0:3], f[3:6], _t(F), BC.get(name)["starts"])


def _facts(name):
    return BC.facts(BC.get(name), _counts(name))


@pytest.mark.parametrize("name", list(BC.CASES))
def test_blocks_and_levels_are_the_intended_ones(name):
    M = BC.get(name)
    n, S0 = M["n"], M["S0"]
    bof = np.repeat(np.arange(len(M["sizes"])), M["sizes"])
    assert S0.diagonal().all()                                     # the identity is a perfect matching of the unpermuted matrix
    ncomp, lab = connected_components(S0, directed=True, connection="strong")
    assert ncomp == len(M["sizes"])
    assert len(set(zip(bof.tolist(), lab.tolist()))) == ncomp      # the same partition
    # the level rule of csx_btf_split: 0 without entries outside the block in its rows, else 1 + the highest level reached
    _, F = _split(M, S0)
    C = F.tocoo()
    assert C.nnz == M["fnz"]
    lev = np.zeros(len(M["sizes"]), np.int64)
    for b in range(len(lev) - 1, -1, -1):
        to = bof[C.col[bof[C.row] == b]]
        lev[b] = lev[to].max() + 1 if len(to) else 0
    assert np.array_equal(lev, M["levels"])
    # the permuted matrix is the unpermuted one
    assert (M["S"] != S0[M["pr"]][:, M["pc"]]).nnz == 0 and M["S"].has_sorted_indices
    assert np.isfinite(M["S"].data).all() and (M["S"].data != 0).all()
    assert n <= 2000 and set(M["widths"]) <= set(BC.WIDTHS)


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_sits_on_its_edge(name):
    c = BC.CASES[name]
    f = _facts(name)
    for key, want in c["claims"].items():
        if key in f:
            assert f[key] == want, (name, key, f[key], want)
    BC.check_counts(c["claims"], _counts(name))
    if c["other"]:
        o = BC.CASES[c["other"]]
        assert o["other"] == name and o["cut"] == c["cut"] and c["cut"] in BC.ROUTE_FACTS
        g = _facts(c["other"])
        differ = [k for k in BC.ROUTE_FACTS if f[k] != g[k]]
        assert differ == [c["cut"]], (name, c["other"], differ)
    if c["claims"].get("pivots_move"):
        M = BC.get(name)
        pinv = cpu_factors(name)[2][6]
        b = int(np.flatnonzero(M["sizes"] == BC.BTF_SMALL)[0])
        a, e = M["starts"][b], M["starts"][b + 1]
        assert (pinv[a:e] != np.arange(a, e)).sum() > BC.BTF_SMALL // 2


def test_the_table_covers_every_edge():
    """a later edit cannot silently drop an edge: every size, term count, F count, level mix, width and group count is somewhere"""
    sizes, widths, groups = set(), set(), set()
    counts = {k: set() for k in ("L", "U", "UT", "LT", "F", "FC")}
    mixes = set()
    for name in BC.CASES:
        M = BC.get(name)
        D, F, f = cpu_factors(name)
        tc = BC.term_counts(f[0:3], f[3:6], _t(F), M["starts"])
        sizes |= set(M["sizes"].tolist())
        widths |= set(M["widths"])
        for k in counts:
            counts[k] |= set(tc[k][tc["small"]].tolist())
        if M["refactor"]:
            groups.add(BC.refactor_model(M["sizes"])["device_groups"])
        per = BC.plan_model(M["sizes"], M["levels"], M["fnz"])["per_level"]
        lds = [p["lds_rows"] for p in per]
        large_rows_with_f = tc["F"][~tc["small"]]
        for l, p in enumerate(per):
            mixes |= {"small and large in a level"} if p["small"] and p["large"] else set()
            mixes |= {"two large in a level"} if len(p["large"]) >= 2 else set()
            mixes |= {"only large in a level"} if p["large"] and not p["small"] else set()
            mixes |= {"largest small block of a level is 1 row"} if p["lds_rows"] == 1 else set()
        if per[0]["large"] and len(per) > 2 and per[2]["large"] and large_rows_with_f.max(initial=0) > 0:
            mixes.add("large at level 0 and at level 2 with F rows")
        if len(per) >= 5 and all(lds[l] == (BC.BTF_SMALL if l % 2 == 0 else 1) for l in range(5)):
            mixes.add("LDS rows alternate over five levels")
        if M["refactor"] and BC.BTF_SMALL in M["sizes"].tolist() and BC.BTF_SMALL + 1 in M["sizes"].tolist():
            mixes.add("host loop and k_refactor in one refactor")
        if M["refactor"] and BC.BTF_SMALL in M["sizes"].tolist() and (M["sizes"] == 1).sum() >= 2 * BC.RF_WAVES:
            mixes.add("one large group beside many 1-row groups")
        if M["refactor"] == "singular":
            mixes.add("failing refactor")
    assert sizes >= set(BC.BLOCK_SIZES)
    assert widths == set(BC.WIDTHS)
    for k in ("L", "U", "UT", "LT"):
        assert counts[k] >= set(BC.TERM_COUNTS), (k, sorted(set(BC.TERM_COUNTS) - counts[k]))
    assert counts["F"] >= set(BC.F_ROW_COUNTS) and counts["FC"] >= set(BC.F_COL_COUNTS)
    assert groups >= set(BC.RF_GROUP_COUNTS)
    assert mixes == {"small and large in a level", "two large in a level", "only large in a level",
                     "largest small block of a level is 1 row", "large at level 0 and at level 2 with F rows",
                     "LDS rows alternate over five levels", "host loop and k_refactor in one refactor",
                     "one large group beside many 1-row groups", "failing refactor"}
    assert all(len(why) > 40 for why in BC.NOT_REACHED.values())


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_is_admitted_by_the_reference_alone(name):
    M = BC.get(name)
    n, S0 = M["n"], M["S0"]
    D, F, (Lp, Li, Lx, Up, Ui, Ux, pinv) = cpu_factors(name)
    ident, r = np.arange(n), M["starts"]
    rng = np.random.default_rng(M["seed"])
    b = rng.uniform(-1, 1, n)
    x = np.asarray(btf_oracle.solve((Lp, Li, Lx), (Up, Ui, Ux), _t(F), pinv, ident, ident, r, b.tolist()))
    assert backward_error(S0, x, b) < BC.BOUND
    xt = np.asarray(trans_oracle.btf_solve_trans((Lp, Li, Lx), (Up, Ui, Ux), _t(F), pinv, ident, ident, r, b.tolist()))
    assert backward_error(S0.T.tocsc(), xt, b) < BC.BOUND
    if M["refactor"] is not None:                                         # (the failing case goes on to a good refactor as well)
        S2 = BC.perturbed(S0, M["seed"] + 1000)
        D2, F2 = _split(M, S2)
        assert np.array_equal(D2.indices, D.indices) and np.array_equal(D2.indptr, D.indptr)
        fresh = _lu(D2, M["tol"])
        assert fresh is not None and np.array_equal(fresh[6], pinv)      # the same pivots: "equals a fresh factor" says something
        nLx, nUx, ok, ratio = refactor_oracle.refactor((Lp, Li, Lx), (Up, Ui, Ux), pinv, _t(D2))
        assert ok and 0.0 < ratio <= 1.0
        assert np.asarray(nLx).tobytes() == fresh[2].tobytes() and np.asarray(nUx).tobytes() == fresh[5].tobytes()
        x2 = np.asarray(btf_oracle.solve((Lp, Li, nLx), (Up, Ui, nUx), _t(F2), pinv, ident, ident, r, b.tolist()))
        assert backward_error(S2, x2, b) < BC.BOUND
    if M["refactor"] == "singular":
        rows, cols = BC.block_of(M, False)
        m = len(rows)
        S2 = BC.singular_values(S0, rows, cols, m - 1, m - 2, M["seed"] + 1000)
        assert np.array_equal(S2.indices, S0.indices) and np.array_equal(S2.indptr, S0.indptr)
        assert np.array_equal(pinv[rows], rows)                           # the dominant entries are the pivots
        D2, _ = _split(M, S2)
        _, nUx, ok, _ = refactor_oracle.refactor((Lp, Li, Lx), (Up, Ui, Ux), pinv, _t(D2))
        assert not ok
        piv = np.asarray(nUx)[Up[cols + 1] - 1]                           # the oracle stops at the first zero pivot: the last one
        assert piv[-1] == 0.0 and np.all(piv[:-1] == 1.0) and cols[-1] == m - 1


def test_lusol_components_are_what_they_say():
    S, S2, sizes = BC.lusol_components()
    n = S.shape[0]
    ncomp, lab = connected_components(S, directed=False)
    assert ncomp == len(sizes) and np.array_equal(np.bincount(lab), sizes)
    assert set(sizes.tolist()) == {BC.TERM_CHUNK + 2, BC.RF_MAX, BC.RF_MAX + 1}
    assert all((sizes == s).sum() >= 2 for s in set(sizes.tolist()))
    m = BC.refactor_model(sizes)
    assert m["host_columns"] == 2 * (BC.RF_MAX + 1) and m["device_columns"] == n - m["host_columns"] and m["device_groups"] == 4
    f, fresh = _lu(S, 1.0), _lu(S2, 1.0)
    assert np.array_equal(f[6], fresh[6])
    nLx, nUx, ok, ratio = refactor_oracle.refactor(f[0:3], f[3:6], f[6], _t(S2))
    assert ok and np.asarray(nLx).tobytes() == fresh[2].tobytes() and np.asarray(nUx).tobytes() == fresh[5].tobytes()
    # dense blocks: every component's L and U have columns of more than one chunk
    assert np.diff(f[0]).max() > BC.TERM_CHUNK and np.diff(f[3]).max() > BC.TERM_CHUNK
