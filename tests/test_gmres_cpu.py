"""gmres() and the csx_gs_* rule without a device: csx_gs_host is byte-equal to the restatement of
tests/gmres_oracle.py on every kernel case of tests/gmres_cases.py and the two kept mistakes are not; the limits are sane and
every case sits on its edge; the Givens recurrences solve the Hessenberg least-squares problem; and the systems the GPU tests
rely on do what they are there for, on the host factors and host rules of the project with the restated loop on top: the model of
refine() ends above 2^-52 (on the stale Cholesky factor it accepts no step at all) and the restated gmres() ends at or below it,
within the inner-step bounds.  NaNs compare by position, not by payload."""
import numpy as np
import pytest

import _csx
import gmres_cases as GC
import gmres_oracle as GO
import refine_cases as RC

EPS = GC.EPS


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()


def test_limits_are_sane_and_every_case_sits_on_its_edge():
    L = _csx.gmres_limits()
    assert sorted(L) == sorted(_csx.GMRES_LIMITS)
    C, F, G = L["GS_CHUNK"], L["GS_FAN"], L["GS_GROUP"]
    assert C >= 64 and F >= 2 and 1 <= G <= 16 and L["GS_TILE"] >= 1 and C % L["GS_TILE"] == 0
    assert _csx.load().csx_gmres_limits(None) == _csx.EINVAL
    # the partial sums stay below 1 / 16 of a block at the sizes the README quotes
    n, k = 5_000_000, 128
    assert _csx.gs_work_len(n, k, 17) - k * (1 + 2 * 17) <= n * k // 16
    assert _csx.gs_work_len(0, 1, 1) == 1 + 2 + 2 * G
    out = _csx.C.c_int64(0)
    for bad in ((-1, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert _csx.load().csx_gs_work_len(*bad, _csx.C.byref(out)) == _csx.EINVAL
    rows = sorted({c.rows for c in GC.KERNEL_CASES})
    assert rows == sorted({1, C - 1, C, C + 1, C * F - 1, C * F, C * F + 1, C * F * F + 1}) and GC.NOT_REACHED == ()
    assert sorted({c.k for c in GC.KERNEL_CASES}) == [1, 3, 4, 5, 63, 64, 65, 130]
    assert sorted({c.nv for c in GC.KERNEL_CASES}) == sorted({1, 2, G - 1, G, G + 1, 17})
    assert {c.mask_kind for c in GC.KERNEL_CASES} == set(GC.MASKS)
    specials = [c.special for c in GC.KERNEL_CASES if c.special is not None]
    assert len(specials) == 2 and np.isnan(specials[0]) and np.isinf(specials[1])
    assert len(GC.KERNEL_NAMES) == len(set(GC.KERNEL_NAMES))


def restated(case, descending=False):
    """what the four operations give on the case, by the restatement"""
    V, W, h, s, y, length = case.data()
    m, nv = case.mask(), case.nv
    basis = [V[i] for i in range(nv)]
    nan = np.full((case.rows, case.k), np.nan)
    return {"h": GO.project(basis, W, m, descending=descending), "h-": GO.project(basis, W, m, negate=True, descending=descending),
            "update": GO.update(basis, W, m, h, descending=descending),
            "update-": GO.update(basis, W, m, h, negate=True, descending=descending),
            "scale": GO.scale(W, s, m, V[nv]), "combine": GO.combine(basis, y, length, m, nan)}


def host_rule(case):
    V, W, h, s, y, length = case.data()
    m, nv = case.mask(), case.nv
    return {"h": _csx.gs_host(_csx.GS_PROJECT, V[:nv], W, m), "h-": _csx.gs_host(_csx.GS_PROJECT, V[:nv], W, m, negate=True),
            "update": _csx.gs_host(_csx.GS_UPDATE, V[:nv], W, m, coef=h),
            "update-": _csx.gs_host(_csx.GS_UPDATE, V[:nv], W, m, coef=h, negate=True),
            "scale": _csx.gs_host(_csx.GS_SCALE, V, W, m, coef=s, nv=nv)[nv],
            "combine": _csx.gs_host(_csx.GS_COMBINE, V[:nv], None, m, coef=y, length=length)}


def agree(got, ref):
    return all(same(got[key][t], ref[key][t]) if isinstance(ref[key], tuple) else same(got[key], ref[key])
               for key in ref for t in ((0, 1) if isinstance(ref[key], tuple) else (0,)))


@pytest.mark.parametrize("name", GC.KERNEL_NAMES)
def test_host_rule_is_the_restatement(name):
    case = GC.KERNEL_BY_NAME[name]
    got, ref = host_rule(case), restated(case)
    for key in ref:
        if isinstance(ref[key], tuple):
            assert same(got[key][0], ref[key][0]) and same(got[key][1], ref[key][1]), key
        else:
            assert same(got[key], ref[key]), key
    V, W, h, s, y, length = case.data()
    m = case.mask()
    # a masked column is left as it was; a NaN or Inf column touches no other
    dead = m == 0
    assert same(got["update"][0][:, dead], W[:, dead]) and same(got["scale"][:, dead], V[case.nv][:, dead])
    if case.special is not None:
        clean = GC.KernelCase(case.name, case.rows, case.k, case.nv, seed=case.seed)
        other = host_rule(clean)
        keep = [c for c in range(case.k) if c not in (1, 2)]
        assert same(got["h"][:, keep], other["h"][:, keep]) and same(got["update"][1][keep], other["update"][1][keep])
        assert not np.isfinite(got["h"][:, 1]).all() and not np.isfinite(got["h"][0, 2])


def test_chunk_sums_in_descending_order_give_other_bytes():
    differ = [name for name in GC.KERNEL_NAMES if GC.KERNEL_BY_NAME[name].rows <= GC.CHUNK * GC.FAN + 1
              and not agree(host_rule(GC.KERNEL_BY_NAME[name]), restated(GC.KERNEL_BY_NAME[name], descending=True))]
    print("descending leaves differ on", differ)
    assert "k3" in differ and "rows%d" % (GC.CHUNK + 1) in differ
    assert "rows1" not in differ                                     # one term: no order to get wrong


def test_bad_arguments_of_the_host_rule():
    lib = _csx.load()
    V, W, m, out = np.zeros((2, 4, 3)), np.zeros((4, 3)), _csx.i32([1, 1, 1]), np.zeros(6)
    coef, ln = np.zeros(6), _csx.i32([1, 1, 1])

    def call(op=0, rows=4, k=3, nv=2, V=V, W=W, m=m, coef=coef, ln=ln, out=out):
        return lib.csx_gs_host(op, rows, k, nv, _csx.pd(V), _csx.pd(W), _csx.pi(m), 0, _csx.pd(coef), _csx.pi(ln), _csx.pd(out))

    assert call() == _csx.OK
    assert call(op=4) == _csx.EINVAL and call(op=-1) == _csx.EINVAL
    assert call(rows=-1) == _csx.EINVAL and call(k=0) == _csx.EINVAL and call(nv=0) == _csx.EINVAL
    assert call(m=None) == _csx.EINVAL and call(V=None) == _csx.EINVAL and call(W=None) == _csx.EINVAL
    assert call(op=1, coef=None) == _csx.EINVAL and call(out=None) == _csx.EINVAL
    assert call(op=3, ln=None, out=np.zeros(12)) == _csx.EINVAL
    assert call(op=3, ln=_csx.i32([3, 0, 0]), out=np.zeros(12)) == _csx.EINVAL       # longer than the basis
    assert call(rows=0) == _csx.OK and not out.any()


def test_givens_recurrences_solve_the_hessenberg_least_squares_problem():
    rng = np.random.default_rng(20241060)
    for m in (1, 2, 5, 16):
        H = np.triu(rng.standard_normal((m + 1, m)), -1)
        beta = float(rng.uniform(0.5, 2.0))
        a = GO.Arnoldi(beta)
        for j in range(m):
            a.step(H[:j + 1, j], H[j + 1, j])
            e1 = np.zeros(j + 2)
            e1[0] = beta
            y, res, _, _ = np.linalg.lstsq(H[:j + 2, :j + 1], e1, rcond=None)
            assert np.max(np.abs(np.asarray(a.solution()) - y)) <= 1e-12 * max(1.0, np.max(np.abs(y))), (m, j)
            rnorm = np.linalg.norm(H[:j + 2, :j + 1] @ y - e1)
            assert abs(abs(a.g[-1]) - rnorm) <= 1e-12 * beta and abs(a.estimate() - rnorm / beta) <= 1e-12
    a = GO.Arnoldi(1.0)
    a.step([0.0], 0.0)                                               # both zero: the rotation is the identity, y = beta / 0
    assert (a.cs, a.sn) == ([1.0], [0.0]) and a.solution() == [np.inf]


# ---- the conditions tests/test_gpu_gmres.py relies on ------------------------------------------------------------------------------

def counted(residual, B):
    """the residual with a count of the candidates it has judged (calls with the right-hand side B)"""
    calls = [0]

    def wrapped(X, Bk):
        calls[0] += np.asarray(Bk).tobytes() == B.tobytes()
        return residual(X, Bk)
    return wrapped, calls


@pytest.mark.parametrize("name", GC.NAMES)
def test_refine_stalls_and_gmres_ends_within_its_bound(name):
    s = GC.BY_NAME[name]
    solve, residual = s.model()
    B = s.B(3)
    ref = RC.refine_loop(solve, residual, B)
    out = GO.gmres_loop(solve, residual, B)
    print(name, "bound", GC.bound(s), "refine: omega0 / eps", ref["omega0"] / EPS, "omega / eps", ref["omega"] / EPS, "steps",
          ref["steps"], "gmres: omega / eps", out["omega"] / EPS, "iters", out["iters"], "cycles", out["cycles"])
    if name == "saddle-perturb1e-10":
        # at this perturbation refinement does reach 2^-52 on the host model (tests/test_slu_cpu.py holds it to that): the
        # system is here for gmres()'s bound; the larger perturbation is the one refinement cannot mend
        assert (ref["omega"] <= EPS).all()
    else:
        assert (ref["omega"] > EPS).all()
    if s.refine_accepts_none:
        assert not ref["steps"].any() and ref["omega"].tobytes() == ref["omega0"].tobytes()
    assert (out["omega"] <= EPS).all() and (out["iters"] <= GC.bound(s)).all() and (out["iters"] >= 1).all()
    assert (out["omega"] <= out["omega0"]).all() and out["omega0"].tobytes() == ref["omega0"].tobytes()
    assert residual(out["x"], B)[1].tobytes() == out["omega"].tobytes()


def test_bounds_of_the_systems():
    assert [GC.bound(s) for s in GC.CHOL] == [4, 12, 26, 4, 12, 26, 12, 12]
    small, large = GC.SADDLE
    assert small.perturbed() == 15 == large.perturbed() and GC.bound(large) == 32      # the 15 pivots that are zero without it
    assert GC.LDL[0].perturbed() >= 1
    n, Ap, Ai, Ax, Ax2 = GC.stale_values()
    cols = np.repeat(np.arange(n), np.diff(Ap))
    assert int(np.sum((Ai == cols) & (np.abs(Ax2) < 2.0 * GC.STALE_PIVOT))) == 64       # one stale pivot per block


def test_nothing_to_do_is_the_plain_solve():
    s = GC.DIAGONAL
    solve, residual = s.model()
    B = s.B(3)
    out = GO.gmres_loop(solve, residual, B)
    assert (out["omega0"] <= EPS).all() and not out["iters"].any() and not out["cycles"].any() and out["solves"] == 1
    assert out["x"].tobytes() == solve(B).tobytes()


def test_a_single_gram_schmidt_pass_gives_other_bytes():
    s = GC.BY_NAME["chol-order0-r5-sigma50"]
    solve, residual = s.model()
    B = s.B(1)
    two, one = GO.gmres_loop(solve, residual, B), GO.gmres_loop(solve, residual, B, single_pass=True)
    assert two["x"].tobytes() != one["x"].tobytes()
    assert two["x"].tobytes() != GO.gmres_loop(solve, residual, B, descending=True)["x"].tobytes()


def test_loop_guarantees_on_the_model():
    s = GC.BY_NAME["saddle-perturb1e-06"]
    solve, residual = s.model()
    B = s.B(3)
    full = GO.gmres_loop(solve, residual, B)
    # a NaN column is never live and disturbs no other
    Bn = B.copy()
    Bn[5, 1] = np.nan
    out = GO.gmres_loop(solve, residual, Bn)
    assert np.isnan(out["omega"][1]) and out["iters"][1] == 0
    for c in (0, 2):
        assert out["x"][:, c].tobytes() == full["x"][:, c].tobytes() and out["iters"][c] == full["iters"][c]
    # maxit cuts the steps; restart = 1 still never raises omega
    cut = GO.gmres_loop(solve, residual, B, maxit=2)
    assert (cut["iters"] <= 2).all() and (cut["omega"] <= cut["omega0"]).all()
    none = GO.gmres_loop(solve, residual, B, maxit=0)
    assert none["solves"] == 1 and none["x"].tobytes() == solve(B).tobytes() and none["omega"].tobytes() == full["omega0"].tobytes()
    one = GO.gmres_loop(solve, residual, B, restart=1, maxit=6)
    assert (one["iters"] <= 6).all() and (one["omega"] <= one["omega0"]).all()


def test_a_refused_cycle_on_the_model():
    """REFUSED (saddle at perturb 1e-5): column 1 ends two accepted cycles at 1.02 eps, runs a third, and the third does not
    lower omega: it is refused, and x is what the run cut before that cycle leaves"""
    s = GC.REFUSED
    solve, residual = s.model()
    B = s.B(3)
    res, calls = counted(residual, B)
    out = GO.gmres_loop(solve, res, B)
    c = GC.REFUSED_COLUMN
    print("omega / eps", out["omega"] / EPS, "iters", out["iters"], "cycles", out["cycles"], "candidates judged", calls[0] - 1)
    assert out["omega"][c] > EPS and out["iters"][c] < GC.MAXIT and out["cycles"][c] < calls[0] - 1
    # the run that ends where the refused cycle began: maxit = the steps of the accepted cycles (a smaller maxit cuts the second
    # cycle short and ends elsewhere)
    before = None
    for cutoff in range(int(out["iters"][c]) - 1, 0, -1):
        cut = GO.gmres_loop(solve, residual, B, maxit=cutoff)
        if cut["cycles"][c] == out["cycles"][c] and cut["iters"][c] == cutoff and cut["omega"][c] == out["omega"][c]:
            before = cut
            break
    assert before is not None
    assert before["x"][:, c].tobytes() == out["x"][:, c].tobytes()
