"""eigsh() and the csx_bgs_* rule without a device: csx_bgs_host is byte-equal to the restatement of
tests/eig_oracle.py on every kernel case of tests/eig_cases.py and the two kept mistakes are not; the limits are sane and every
case sits on its edge; and the restated loop, on dense numpy solves of the pencils the GPU tests use, finds the eigenvalues
nearest the shift -- all of them, none missed -- within the block bound of the issue.  NaNs compare by position, not by payload."""
import numpy as np
import pytest

import _csx
import eig_cases as EC
import eig_oracle as EO

TOL = EC.TOL


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()


def test_limits_are_sane_and_every_case_sits_on_its_edge():
    L = _csx.bgs_limits()
    assert sorted(L) == sorted(_csx.BGS_LIMITS)
    C, F, W, G = L["GS_CHUNK"], L["GS_FAN"], L["BGS_MAXW"], L["BGS_GROUP"]
    assert (C, F) == (_csx.gmres_limits()["GS_CHUNK"], _csx.gmres_limits()["GS_FAN"])          # §28's tree, unchanged
    assert 8 <= W <= 64 and 1 <= G <= 8 and L["BGS_TILE"] >= W and L["BGS_TILE"] // W >= 1
    assert G * ((W + 3) // 4) ** 2 <= 256                            # a group's 4 x 4 thread tiles fit a workgroup
    assert _csx.load().csx_bgs_limits(None) == _csx.EINVAL
    # the partial sums of a group stay below one rows x max(b, q) block
    for b, q in ((8, 8), (W, W), (W, 1), (1, W)):
        n = 5_000_000
        assert _csx.bgs_work_len(n, b, q, 17) - 2 * 17 * b * q < n * max(b, q)
    assert _csx.bgs_work_len(0, 1, 1, 0) == 2 * G and _csx.bgs_work_len(0, 2, 3, 1) == 6 * (2 + 2 * G)
    out = _csx.C.c_int64(0)
    for bad in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, W + 1, 1, 1), (1, 1, W + 1, 1), (1, 1, 1, -1)):
        assert _csx.load().csx_bgs_work_len(*bad, _csx.C.byref(out)) == _csx.EINVAL
    assert _csx.load().csx_bgs_work_len(1, 1, 1, 1, None) == _csx.EINVAL
    assert {c.rows for c in EC.KERNEL_CASES} >= {1, C - 1, C, C + 1, C * F - 1, C * F, C * F + 1, C * F * F + 1}
    assert {(c.b, c.q) for c in EC.KERNEL_CASES} >= {(1, 1), (2, 3), (3, 2), (8, 8), (9, 7), (W, W), (W, 1)}
    assert {c.nv for c in EC.KERNEL_CASES} >= {1, 2, G - 1, G, G + 1}
    assert sorted(c.special for c in EC.KERNEL_CASES if c.special) == ["inf", "nan"]
    assert len(EC.KERNEL_NAMES) == len(set(EC.KERNEL_NAMES))


def restated(case, descending=False):
    V, W, H = case.data()
    basis = list(V)
    return {"gram": EO.gram(basis, W), "gram-": EO.gram(basis, W, negate=True), "update": EO.update(basis, W, H),
            "combine": EO.combine(basis, H, case.rows, case.q, descending=descending)}


def host_rule(case):
    V, W, H = case.data()
    return {"gram": _csx.bgs_host(_csx.BGS_GRAM, V, W), "gram-": _csx.bgs_host(_csx.BGS_GRAM, V, W, negate=True),
            "update": _csx.bgs_host(_csx.BGS_UPDATE, V, W, coef=H), "combine": _csx.bgs_host(_csx.BGS_COMBINE, V, coef=H)}


@pytest.mark.parametrize("name", EC.KERNEL_NAMES)
def test_host_rule_is_the_restatement(name):
    case = EC.KERNEL_BY_NAME[name]
    got, ref = host_rule(case), restated(case)
    for key in ref:
        assert same(got[key], ref[key]), key
    if case.special == "nan":                                       # the NaN column of W: its own outputs, no other
        clean = host_rule(EC.KernelCase(case.name, case.rows, case.b, case.q, case.nv, case.seed))
        keep = [c for c in range(case.q) if c != 1]
        for key in ("gram", "gram-", "update"):                     # (combine does not read W)
            assert np.isnan(got[key][..., 1]).all() and same(got[key][..., keep], clean[key][..., keep]), key
    if case.special == "inf":                                       # the Inf of V_0[:, 2]: row (0, 2) of the sums
        assert not np.isfinite(got["gram"][0, 2]).any() and np.isfinite(got["gram"][1]).all() and np.isfinite(got["gram"][0, :2]).all()


def test_combine_in_descending_order_gives_other_bytes():
    differ = [name for name in EC.KERNEL_NAMES if EC.KERNEL_BY_NAME[name].rows <= EC.CHUNK * EC.FAN + 1 and not same(
        host_rule(EC.KERNEL_BY_NAME[name])["combine"], restated(EC.KERNEL_BY_NAME[name], descending=True)["combine"])]
    print("descending (i, a) differs on", differ)
    assert "w8x8" in differ and "nv%d" % (EC.GROUP + 1) in differ and "w%dx1" % EC.MAXW in differ
    assert "w1x1" not in differ                                      # two terms: an addition commutes


def test_nv_0_and_rows_0():
    V0 = np.zeros((0, 5, 3))
    assert _csx.bgs_host(_csx.BGS_COMBINE, V0, q=2).tobytes() == np.zeros((5, 2)).tobytes()          # +0.0
    W = np.arange(10.0).reshape(5, 2)
    assert _csx.bgs_host(_csx.BGS_UPDATE, V0, W, coef=np.zeros((0, 3, 2))).tobytes() == W.tobytes()
    assert _csx.bgs_host(_csx.BGS_GRAM, np.zeros((2, 0, 3)), np.zeros((0, 2))).tobytes() == np.zeros((2, 3, 2)).tobytes()


def test_bad_arguments_of_the_host_rule():
    lib = _csx.load()
    V, W, H, out = np.zeros((2, 4, 3)), np.zeros((4, 2)), np.zeros((2, 3, 2)), np.zeros(12)

    def call(op=0, rows=4, b=3, q=2, nv=2, V=V, W=W, H=H, out=out):
        return lib.csx_bgs_host(op, rows, b, q, nv, _csx.pd(V), _csx.pd(W), 0, _csx.pd(H), _csx.pd(out))

    E = _csx.EINVAL
    for op in (0, 1, 2):
        assert call(op=op) == _csx.OK
        assert call(op=op, rows=-1) == E and call(op=op, nv=-1) == E and call(op=op, V=None) == E
        assert call(op=op, b=0) == E and call(op=op, q=0) == E and call(op=op, b=EC.MAXW + 1) == E and call(op=op, q=EC.MAXW + 1) == E
    assert call(op=3) == E and call(op=-1) == E
    assert call(op=0, W=None) == E and call(op=1, W=None) == E and call(op=2, W=None) == _csx.OK
    assert call(op=1, H=None) == E and call(op=2, H=None) == E and call(op=0, H=None) == _csx.OK
    assert call(op=0, out=None) == E and call(op=2, out=None) == E and call(op=1, out=None) == _csx.OK


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------

_RUNS = {}


def run(name, **kw):
    """the restated loop on the pencil's dense solves; the plain run of a pencil is computed once"""
    p = EC.PENCIL_BY_NAME[name]
    key = (name, tuple(sorted(kw.items())))
    if key not in _RUNS:
        args = dict(sigma=p.sigma, block=p.block, tol=TOL)
        args.update(kw)
        _RUNS[key] = EO.eig_loop(*EC.dense_callables(p), p.n, p.nev, **args)
    return _RUNS[key]


def holds(p, out, tol=TOL):
    """the conditions of the issue on a result of eigsh() for the pencil p (vectors as an array)"""
    lam, cond = p.reference()
    near = p.nearest()
    mu = near - p.sigma
    print(p.name, "blocks", out["blocks"], "solves", out["solves"], "products", out["products"], "resid", out["resid"].max(),
          "estimate", out["estimate"].max(), "omega", out["omega"].max())
    assert out["converged"].all() and not out["breakdown"] and out["blocks"] <= EC.MAX_BLOCKS and out["solves"] == out["blocks"]
    assert (out["resid"] <= tol).all()
    got = out["values"]
    assert got.shape == (p.nev,) and (np.diff(np.abs(got - p.sigma)) >= 0.0).all()                  # ascending |mu|
    # the same nev values, none missed: Bauer-Fike on the Cholesky-reduced pencil
    err = np.abs(np.sort(got) - np.sort(near))
    bound = tol * np.abs(np.sort(near) - p.sigma) * np.sqrt(cond)
    print("   error", err.max(), "bound", bound.min(), "gap to the next", np.abs(lam - p.sigma)[np.argsort(np.abs(lam - p.sigma))][p.nev] - np.abs(mu).max())
    assert (err <= bound).all()
    M, X = p.M(), np.asarray(out["vectors"])
    G = X.T @ (M @ X if M is not None else X)
    assert np.abs(G - np.eye(p.nev)).max() <= 1e-12


@pytest.mark.parametrize("name", EC.PENCIL_NAMES)
def test_the_restated_loop_finds_the_pairs_nearest_the_shift(name):
    p = EC.PENCIL_BY_NAME[name]
    out = run(name)
    holds(p, out)
    assert sorted(out) == ["blocks", "breakdown", "converged", "estimate", "omega", "products", "resid", "solves", "values", "vectors"]
    assert (out["products"] == 0) == (not p.mass)


def test_one_projection_pass_gives_other_bytes():
    name = "grid17x13-mass-3.7"
    one = run(name, single_pass=True)
    assert not same(one["vectors"], run(name)["vectors"])


def test_the_12x12_grid_has_multiple_eigenvalues():
    p = EC.PENCIL_BY_NAME["grid12x12-3.7"]
    near = np.sort(p.nearest())
    assert (np.diff(near) < 1e-12).any()                            # a block method finds both copies


def test_below_counts_the_eigenvalues_under_the_shift():
    for p in EC.PENCILS:
        w = np.linalg.eigvalsh(p.A())                               # Sylvester: the inertia of K - sigma M
        assert int((w < 0.0).sum()) == p.below()
    assert EC.PENCIL_BY_NAME["grid17x13-mass-0"].below() == 0


def test_breakdown_ends_with_exact_pairs():
    A, v0 = EC.breakdown_pencil()

    def residual(X, B):
        R = B - A @ X
        return R, np.abs(R).max(axis=0)

    out = EO.eig_loop(lambda B: np.linalg.solve(A, B), None, residual, 24, 4, block=8, v0=v0)
    assert out["breakdown"] and out["blocks"] == 1 and out["converged"].all() and (out["estimate"] == 0.0).all()
    ref = np.sort(np.linalg.eigvalsh(A[:8, :8]))[:4]
    assert np.abs(out["values"] - ref).max() <= 1e-13 * ref.max() and (out["resid"] <= 1e-14).all()
    assert not out["vectors"][8:].any()                             # the pairs live in the invariant subspace, exactly


def test_a_tolerance_below_the_attainable_ends_unconverged_without_raising():
    """at tol 2^-40 the 40 x 37 pencil stalls: the residuals stay near 4e-12 (3.8e-12 measured on the dense solves) up to the
    last block, and the loop returns what it has"""
    p = EC.PENCIL_BY_NAME["grid40x37-mass-3.7"]
    out = run(p.name, tol=2.0 ** -40)
    print("resid", out["resid"], "blocks", out["blocks"])
    assert not out["converged"].all() and not out["breakdown"] and out["blocks"] == 31
    assert out["resid"].max() < 1e-10 and (out["converged"] == (out["resid"] <= 2.0 ** -40)).all()
