"""csx_pattern_outer and csx_assemble_pullback without a device: the limits are sane and every case of
tests/outer_cases.py sits on its edge; csx_pattern_outer_host is byte-equal to the restatement of tests/outer_oracle.py on every
case in every mode and the two kept mistakes are not; the host rule agrees with the exact sum within the bound its depth gives;
csx_assemble_pullback_host is numpy indexing; and the exact fixtures of tests/test_gpu_solve_grad.py ARE exact: on the host
factor and solve rules of the project with the host outer rule on top, every entry of gb and gA equals the computation in
fractions.Fraction.  NaNs compare by position, not by payload."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _csx
import c_oracle as CO
import csparse_oracle as O
import ldl_cases as LC
import ldl_oracle as LO
import outer_cases as OC
import outer_oracle as OO
import slu_cases as SC
import slu_oracle as SO

W, E, EW, F, KEPT = OC.W, OC.E, OC.EW, OC.F, OC.KEPT


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()


def host(case, sym, alpha=-1.0, clean=False):
    U, V = case.data(clean)
    return _csx.pattern_outer_host(case.m, case.n, case.p, case.i, U, V, case.nrhs, alpha, sym)


def restated(case, sym, alpha=-1.0, mistake=None):
    U, V = case.data()
    return OO.pattern_outer(case.m, case.n, case.p, case.i, U, V, case.nrhs, alpha, sym, lanes=W, mistake=mistake)


def test_limits_are_sane_and_every_case_sits_on_its_edge():
    L = _csx.pattern_outer_limits()
    assert sorted(L) == sorted(_csx.PATTERN_OUTER_LIMITS)
    assert W >= 2 and W & (W - 1) == 0 and 64 % W == 0 and 8 * W == 128       # one 128-byte line of a block row
    assert E % EW == 0 and EW % 64 == 0 and E // EW == 4 and F >= 1 and (EW * W // 64) % F == 0
    assert _csx.load().csx_pattern_outer_limits(None) == _csx.EINVAL
    assert sorted({c.nrhs for c in OC.CASES if c.kind == "nrhs"}) == sorted({1, 2, 3, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1,
                                                                              130})
    assert sorted(int(c.column_lengths()[0]) for c in OC.CASES if c.kind == "column") == sorted(
        {E - 1, E, E + 1, 4 * E + 1, EW - 1, EW, EW + 1})
    assert all(c.n == 1 for c in OC.CASES if c.kind == "column")
    assert KEPT >= 1 and KEPT & (KEPT - 1) == 0
    kept = [c for c in OC.CASES if c.kind == "kept"]
    assert sorted({c.nrhs for c in kept}) == sorted({W + 1, 2 * W, 2 * W + 1, 4 * W, 4 * W + 1, KEPT * W - 1, KEPT * W, KEPT * W + 1})
    lens = set(kept[0].column_lengths().tolist())
    assert {1, F - 1, F, F + 1}.issubset(lens) and max(lens) > 4 * W * F and any(v % F for v in lens if v > F) and kept[0].square
    B = OC.BY_NAME
    assert (B["0x0"].m, B["0x0"].n) == (0, 0) and B["m0"].m == 0 and B["m0"].n > 0 and B["n0"].n == 0 and B["n0"].m > 0
    assert B["nnz0_n5"].n == 5 and B["nnz0_n5"].nnz == 0 and (B["1x1"].m, B["1x1"].n, B["1x1"].nnz) == (1, 1, 1)
    c = B["columns_of_one"]
    assert c.n == 3 * E and (c.column_lengths() == 1).all()
    c = B["every_other_empty"].column_lengths()
    assert (c[1::2] == 0).all() and (c[0::2] > 0).any()
    c = B["first_last_empty"].column_lengths()
    assert c[0] == 0 and c[-1] == 0 and (c[1:-1] > 0).all()
    assert (B["5x300"].m, B["5x300"].n) == (5, 300) and (B["300x5"].m, B["300x5"].n) == (300, 5)
    c = B["rows_0_and_last"]
    assert set(c.i.tolist()) == {0, c.m - 1}
    c = B["duplicates_unsorted"]
    mid = c.i[c.p[1]:c.p[2]].tolist()
    assert len(set(mid)) < len(mid) and mid != sorted(mid)
    for name in OC.NAMES:
        assert all(n <= 5000 for n in (B[name].m, B[name].n))
    # the symmetric storages: three share one upper triangle; one is the diagonal, one lies strictly below it
    col = {name: np.repeat(np.arange(B[name].n), B[name].column_lengths()) for name in OC.NAMES if B[name].kind == "sym"}
    up = [sorted(OC.upper_slots(B[name])) for name in OC.SYM_SHARED]
    assert up[0] == up[1] == up[2] and len(up[0]) == B["sym_upper"].nnz
    assert (B["sym_upper"].i <= col["sym_upper"]).all() and (B["sym_full"].i > col["sym_full"]).any()
    assert B["sym_full_other_below"].values is not None
    assert (B["sym_diagonal"].i == col["sym_diagonal"]).all() and (B["sym_strictly_lower"].i > col["sym_strictly_lower"]).all()
    specials = [c.special[2] for c in OC.CASES if c.special is not None]
    assert len(specials) == 2 and np.isnan(specials[0]) and np.isinf(specials[1])
    assert [c.special[0] for c in OC.CASES if c.special is not None] == ["U", "V"]
    assert len(OC.NAMES) == len(set(OC.NAMES))


@pytest.mark.parametrize("name", OC.NAMES)
def test_host_rule_is_the_restatement(name):
    case = OC.BY_NAME[name]
    for sym in OC.modes(case):
        for alpha in (-1.0, 0.75):
            got = host(case, sym, alpha)
            assert got.shape == (case.nnz,) and same(got, restated(case, sym, alpha)), (name, sym, alpha)
    if case.special is not None:
        for sym in OC.modes(case):
            got, clean, hit = host(case, sym), host(case, sym, clean=True), case.touched(sym)
            assert hit.any() and not np.isfinite(got[hit]).any()
            assert got[~hit].tobytes() == clean[~hit].tobytes()           # ... and only into the entries whose rows hold them


def test_alpha_minus_one_is_the_exact_negation_and_one_column_is_one_product():
    case = OC.BY_NAME["nrhs%d" % (2 * W + 1)]
    assert same(host(case, False, -1.0), -host(case, False, 1.0))
    case = OC.BY_NAME["nrhs1"]
    U, V = case.data()
    col = np.repeat(np.arange(case.n), case.column_lengths())
    assert same(host(case, False, 1.0), U[case.i, 0] * V[col, 0])


def test_the_kept_mistakes_differ():
    wide = [c for c in OC.CASES if c.nrhs > W and c.special is None]
    assert any(not same(restated(c, False), restated(c, False, mistake="left_to_right")) for c in wide)
    case = OC.BY_NAME["sym_diagonal"]
    assert not same(restated(case, True), restated(case, True, mistake="diagonal_twice"))
    for name in ("sym_upper", "sym_strictly_lower"):          # ... and only there
        case = OC.BY_NAME[name]
        col = np.repeat(np.arange(case.n), case.column_lengths())
        off = case.i != col
        a, b = restated(case, True), restated(case, True, mistake="diagonal_twice")
        assert a[off].tobytes() == b[off].tobytes()


def test_strictly_lower_entries_are_plus_zero():
    for name in ("sym_strictly_lower", "sym_full"):
        case = OC.BY_NAME[name]
        col = np.repeat(np.arange(case.n), case.column_lengths())
        got = host(case, True)
        low = case.i > col
        assert low.any() and got[low].tobytes() == np.zeros(int(low.sum())).tobytes()


@pytest.mark.parametrize("name", [c.name for c in OC.CASES if c.special is None and c.nnz and c.nnz <= 400])
def test_host_rule_is_within_the_bound_of_its_depth(name):
    """|rule - exact| <= (ceil(nrhs / W') + log2 W' + 2) 2^-53 sum |terms| per entry, twice that in sym mode (W' the rule's
    width for this nrhs): a partial is a chain of ceil(nrhs / W') roundings (twice as many with the mirrored products), the
    butterfly adds log2 W', the products and alpha one each"""
    case = OC.BY_NAME[name]
    U, V = case.data()
    k, alpha = case.nrhs, 0.75
    w = OO.width(k, W)
    col = np.repeat(np.arange(case.n), case.column_lengths())
    for sym in OC.modes(case):
        got = host(case, sym, alpha)
        for q in range(case.nnz):
            i, j = int(case.i[q]), int(col[q])
            if sym and i > j:
                continue
            terms = [Fraction(float(U[i, c])) * Fraction(float(V[j, c])) for c in range(k)]
            if sym and i < j:
                terms += [Fraction(float(U[j, c])) * Fraction(float(V[i, c])) for c in range(k)]
            exact = Fraction(alpha) * sum(terms)
            size = abs(Fraction(alpha)) * sum(abs(t) for t in terms)
            bound = (-(-k // w) + int(math.log2(w)) + 2) * Fraction(2) ** -53 * size * (2 if sym else 1)
            assert abs(Fraction(float(got[q])) - exact) <= bound, (name, sym, q)


def test_host_rule_refuses_bad_arguments():
    lib = _csx.load()
    p, i = _csx.i32([0, 1, 2]), _csx.i32([0, 1])
    U = V = np.ones(4)
    out = np.full(2, 7.0)

    def call(m=2, n=2, p=p, i=i, nrhs=2, mode=0, U=U, V=V, out=out):
        return lib.csx_pattern_outer_host(m, n, _csx.pi(p), _csx.pi(i), nrhs, mode, 1.0, _csx.pd(U), _csx.pd(V), _csx.pd(out))

    assert call() == _csx.OK and (out == 2.0).all()
    out[:] = 7.0
    bad = [dict(nrhs=0), dict(mode=2), dict(mode=-1), dict(m=3, mode=1, i=_csx.i32([0, 2])), dict(i=_csx.i32([0, 2])),
           dict(i=_csx.i32([-1, 0])), dict(p=_csx.i32([0, 2, 1])), dict(p=_csx.i32([1, 1, 2])), dict(U=None), dict(out=None),
           dict(m=-1)]
    for kw in bad:
        assert call(**kw) == _csx.EINVAL, kw
    assert (out == 7.0).all()


@pytest.mark.parametrize("plan", OC.PLANS, ids=[p.name for p in OC.PLANS])
def test_pullback_host_is_numpy_indexing(plan):
    got = _csx.assemble_pullback_host(plan.sp, plan.src, plan.g)
    slot = np.empty(plan.nz, np.int64)
    slot[plan.src] = np.repeat(np.arange(plan.nnz), np.diff(plan.sp))
    assert got.tobytes() == plan.g[slot].tobytes() and got.tobytes() == OO.pullback(plan.sp, plan.src, plan.g).tobytes()
    if plan.name == "dup70":
        assert np.diff(plan.sp).max() >= 70
    if plan.name == "no_duplicates":
        assert plan.nz == plan.nnz > 0
    if plan.name == "nz0":
        assert plan.nz == 0 and plan.nnz == 0
    # every triplet of a slot is the slot's own triplet: its (row, column) are the slot's
    lib = _csx.load()
    assert lib.csx_assemble_pullback_host(plan.nnz, plan.nz + 1, _csx.pi(plan.sp), _csx.pi(plan.src), _csx.pd(plan.g),
                                          _csx.pd(np.zeros(plan.nz + 1))) == _csx.EINVAL


# ---- the exact fixtures ARE exact ------------------------------------------------------------------------------------------------

def _columns(solve_one, B):
    return np.column_stack([solve_one(np.ascontiguousarray(B[:, c])) for c in range(B.shape[1])])


def _check_exact(fx, X, lam, trans):
    """the host outer rule on the host solves against the Fractions"""
    Xr, lr, gr = fx.rational(trans)
    assert np.array_equal(X, OC.as_floats(Xr)) and np.array_equal(lam, OC.as_floats(lr))
    U, V = (X, lam) if trans else (lam, X)
    gA = _csx.pattern_outer_host(fx.n, fx.n, fx.p, fx.i, U, V, OC.EXACT_K, -1.0, fx.sym)
    assert np.array_equal(gA, OC.as_floats(gr))
    assert np.abs(gA).max() > 0 and np.abs(lam).max() > 0


@pytest.mark.parametrize("trans", (False, True))
def test_exact_fixture_lu_host(trans):
    fx = OC.EXACT["lower"]
    n = fx.n
    N = O.cs_lu(fx.matrix(O), O.cs_sqr(0, fx.matrix(O), False), 1.0)
    assert N is not None and list(N.pinv) == list(range(n))                # the pivots are the diagonal entries
    Lp, Li, Lx = np.asarray(N.L.p, np.int32), np.asarray(N.L.i[:N.L.p[n]], np.int32), np.asarray(N.L.x[:N.L.p[n]])
    Up, Ui, Ux = np.asarray(N.U.p, np.int32), np.asarray(N.U.i[:N.U.p[n]], np.int32), np.asarray(N.U.x[:N.U.p[n]])

    def plain(b):
        return CO.usolve(n, Up, Ui, Ux, CO.lsolve(n, Lp, Li, Lx, b))

    def transposed(b):
        return CO.ltsolve(n, Lp, Li, Lx, CO.utsolve(n, Up, Ui, Ux, b))

    X = _columns(transposed if trans else plain, fx.B)
    lam = _columns(plain if trans else transposed, fx.GX)
    _check_exact(fx, X, lam, trans)


@pytest.mark.parametrize("trans", (False, True))
def test_exact_fixture_static_lu_host(trans):
    fx = OC.EXACT["lower"]
    case = SC.Case("exact-lower", fx.n, fx.p, fx.i, fx.x)
    st, Lx, Ux, info = SO.host(case, case.x, 0.0)
    assert st == 0 and info[2] == 0 and info[3] == -1
    Lp, Li, _ = SO.pattern_of(case)
    n = fx.n

    def plain(b):
        return SO.solve(case, Lx, Ux, b)

    def transposed(b):                    # A = L Ut' in natural order: A'^-1 b = L'^-1 Ut^-1 b
        return CO.ltsolve(n, Lp, Li, Lx, CO.lsolve(n, Lp, Li, Ux, b))

    X = _columns(transposed if trans else plain, fx.B)
    lam = _columns(plain if trans else transposed, fx.GX)
    _check_exact(fx, X, lam, trans)


def test_exact_fixture_cholesky_host():
    fx = OC.EXACT["chol"]
    n = fx.n
    A = fx.matrix(O)
    S = O.cs_schol(0, A)
    N = O.cs_chol(A, S)
    assert N is not None
    Lp, Li, Lx = np.asarray(N.L.p, np.int32), np.asarray(N.L.i[:N.L.p[n]], np.int32), np.asarray(N.L.x[:N.L.p[n]])

    def solve(b):
        return CO.ltsolve(n, Lp, Li, Lx, CO.lsolve(n, Lp, Li, Lx, b))

    _check_exact(fx, _columns(solve, fx.B), _columns(solve, fx.GX), False)


def test_exact_fixture_ldl_host():
    fx = OC.EXACT["ldl"]
    n = fx.n
    case = LC.Case("exact-ldl", n, fx.p, fx.i, fx.x)
    st, Lx, d, info = LO.host(case, case.x, 0.0)
    assert st == 0 and info[1] > 0 and info[2] == 0 and info[3] == -1      # indefinite, nothing perturbed, no breakdown
    Lp, Li, _ = LO.pattern_of(case)

    def solve(b):
        return CO.ltsolve(n, Lp, Li, Lx, CO.lsolve(n, Lp, Li, Lx, b) / d)

    _check_exact(fx, _columns(solve, fx.B), _columns(solve, fx.GX), False)
