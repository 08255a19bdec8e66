"""sparseinv_ldl / sparseinv_lu and the inverse() / inverse_at() / inverse_entries() / inverse_diag() of ldlsol_factor and
slusol_factor on the device: every value byte-equal to the restatement (tests/sparseinv_ldlu_oracle.py) run on
exactly the factor the device holds, on one case per side of every cut of the launch selection
(tests/sparseinv_ldlu_cases.py); against the dense inverse only on the cases tests/test_sparseinv_ldlu_cpu.py names (those where
the restatement itself meets the bound), with the error printed on the others."""
import functools

import numpy as np
import pytest

import ldl_cases as LC
import slu_cases as SC
import sparseinv_ldlu_cases as CASES
import sparseinv_ldlu_oracle as SI
import tol as TOL
from test_gpu_parity import cs  # noqa: F401
from test_sparseinv_ldlu_cpu import ACCURACY_LDL, ACCURACY_SLU, GROWTH_LDL, GROWTH_SLU

pytestmark = pytest.mark.gpu


def _dev_cs(cs, n, p, i, x):
    import _csx
    p, i, x = np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64)
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(n, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), h), "csx_csc_upload")
    return cs._from_device(h, lambda nnz: max(nnz, 1))


def _arrays(M):
    import _csx
    m, n, nnz, hv = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return p, i[:nnz], x[:nnz]


@functools.lru_cache(maxsize=None)
def _want(name):
    """the restatement's bytes for a constructed case, computed once: (Z.x of LDL', ZL.x, ZUt.x of LU)"""
    c = CASES.BY_NAME[name]
    z = SI.ldl_x_np(c.n, c.p, c.i, c.lx, c.d)
    zl, zu = SI.lu_x_np(c.n, c.p, c.i, c.lx, c.ux)
    return z.tobytes(), zl.tobytes(), zu.tobytes()


def _check_info(cs, c, kind, walk=True):
    info = cs.sparseinv_info()
    nd, widest, _ = CASES.model(c, walk)
    assert info["kind"] == kind and info["n"] == c.n
    assert (info["depths"], info["widest"], info["terms"]) == (nd, widest, c.terms()), info


@pytest.mark.parametrize("name", CASES.NAMES)
def test_ldl_bytes_of_the_loop_at_every_cut(cs, name):
    import _csx
    c = CASES.BY_NAME[name]
    L = _dev_cs(cs, c.n, c.p, c.i, c.lx)
    d = cs.dvec(c.d)
    want = _want(name)[0]
    for walk in (1, 0) if name in CASES.WALK_OFF else (1,):
        with _csx.option("sparseinv.walk", walk):
            for _ in range(2):
                Z = cs.sparseinv_ldl(L, d)
                _check_info(cs, c, "ldl", bool(walk))
                zp, zi, zx = _arrays(Z)
                assert np.array_equal(zp, c.p) and np.array_equal(zi, c.i)
                assert zx.tobytes() == want, (name, walk)
    assert _arrays(L)[2].tobytes() == c.lx.tobytes() and d.numpy().tobytes() == c.d.tobytes()     # nothing is changed


@pytest.mark.parametrize("name", CASES.NAMES)
def test_lu_bytes_of_the_loop_at_every_cut(cs, name):
    import _csx
    c = CASES.BY_NAME[name]
    L, U = _dev_cs(cs, c.n, c.p, c.i, c.lx), _dev_cs(cs, c.n, c.p, c.i, c.ux)
    _, wl, wu = _want(name)
    for walk in (1, 0) if name in CASES.WALK_OFF else (1,):
        with _csx.option("sparseinv.walk", walk):
            for _ in range(2):
                ZL, ZU = cs.sparseinv_lu(L, U)
                _check_info(cs, c, "lu", bool(walk))
                for Z, want in ((ZL, wl), (ZU, wu)):
                    zp, zi, zx = _arrays(Z)
                    assert np.array_equal(zp, c.p) and np.array_equal(zi, c.i)
                    assert zx.tobytes() == want, (name, walk)
    assert _arrays(L)[2].tobytes() == c.lx.tobytes() and _arrays(U)[2].tobytes() == c.ux.tobytes()


def test_chol_call_still_reports_its_kind(cs):
    c = CASES.BY_NAME["cliques2x9"]
    x = np.abs(c.lx) + 1.0
    cs.sparseinv(_dev_cs(cs, c.n, c.p, c.i, x))
    assert cs.sparseinv_info()["kind"] == "chol"


# ---- through the solvers ------------------------------------------------------------------------------------------------

def _entries(case):
    return case.i.astype(np.int64), case.cols.astype(np.int64)


def _trace(case, z, symmetric):
    """sum_q w_q A_q z_q over the stored entries the factorisation sees (no duplicates): trace(A inv(A)) = n"""
    r, c = _entries(case)
    if symmetric:
        use = r <= c
        w = np.where(r == c, 1.0, 2.0)[use]
        return float(np.sum(w * case.x[use] * z[use])), float(np.sum(np.abs(w * case.x[use] * z[use])))
    return float(np.sum(case.x * z)), float(np.sum(np.abs(case.x * z)))


def _trace_tol(accurate, bound, nnz, growth):
    """relative to the sum of the magnitudes of the nnz terms: one rounding a term of the sum itself (nnz eps), and the error
    of the entries -- the bound they are held to where they are held to one, else a rounding for every term scaled by the
    factor's growth max |l| (what the recurrence inherits from a static-pivot factor)"""
    return bound + nnz * TOL.EPS if accurate else nnz * TOL.EPS * max(1.0, growth)


def _ldl_factor(cs, case, which="A"):
    F = cs.ldlsol_factor(case.matrix(cs, case.values(which)), case.order, case.perturb)
    assert F is not None
    return F


def _ldl_restated(F, case):
    """the restatement on the factor the device holds: (pinv, p, i, Z.x)"""
    p, i, x = _arrays(F.factors.L)
    d = F.factors.D.numpy().reshape(-1)
    pinv = F.symbolic.pinv
    return (None if pinv is None else np.asarray(pinv, np.int64)), p, i, SI.ldl_x_np(case.n, p, i, x, d)


@pytest.mark.parametrize("name", ACCURACY_LDL + GROWTH_LDL)
def test_ldlsol_factor_inverse_entries(cs, name):
    case = LC.BY_NAME[name]
    n = case.n
    F = _ldl_factor(cs, case)
    pinv, p, i, z = _ldl_restated(F, case)
    zp, zi, zx = _arrays(F.inverse())
    assert cs.sparseinv_info()["kind"] == "ldl"
    assert np.array_equal(zp, p) and np.array_equal(zi, i) and zx.tobytes() == z.tobytes()
    r, c = _entries(case)
    ent = F.inverse_entries()
    want, missing = SI.gather(n, p, i, z, None, pinv, pinv, r, c)
    assert missing == 0 and ent.tobytes() == want.tobytes()
    k = np.arange(n)
    dg = F.inverse_diag()
    assert dg.tobytes() == SI.gather(n, p, i, z, None, pinv, pinv, k, k)[0].tobytes()
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(r), 40)
    at = F.inverse_at(c[pick], r[pick])                            # the mirrored pairs: the same slots
    assert at.tobytes() == ent[pick].tobytes()
    A = case.dense()
    ref = np.linalg.inv(A)
    bound = TOL.cross_bound(np.linalg.cond(A, 1))
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    err = max(TOL.componentwise(ent, ref[lo, hi]), TOL.componentwise(dg, np.diag(ref)))
    print(name, "entries and diagonal against the dense inverse, componentwise", err, "bound", bound, "max |l|", F.info()["max_abs_l"])
    if name in ACCURACY_LDL:
        assert err <= bound
    if name != "dups":
        tr, mag = _trace(case, ent, True)
        print(name, "sum_q A_q inv(A)_q - n =", tr - n, "sum of magnitudes", mag)
        assert abs(tr - n) <= _trace_tol(name in ACCURACY_LDL, bound, len(r), F.info()["max_abs_l"]) * mag
    off = np.argwhere(SI.dense_lower_upper(n, p, i, np.ones(len(i)), None) == 0)
    if len(off):
        perm = np.arange(n) if pinv is None else np.argsort(pinv)
        with pytest.raises(ValueError) as e:
            F.inverse_at([perm[off[0][0]], 0], [perm[off[0][1]], 0])
        assert "1 of 2 pairs" in str(e.value)
    with pytest.raises(ValueError):
        F.inverse_at([n], [0])
    assert F.inverse_diag().tobytes() == dg.tobytes()


def _slu_factor(cs, case, which="A"):
    F = cs.slusol_factor(case.matrix(cs, case.values(which)), case.order, case.perturb, case.match, case.match_seed)
    assert F is not None
    return F


def _slu_maps(F, n):
    """(rmap, cmap) of inv(A)(x, y) = Z(rmap[x], cmap[y]): pinv and pinv o prow^-1"""
    pinv = np.arange(n) if F.factors.pinv is None else np.asarray(F.factors.pinv, np.int64)
    if F.factors.prow is None:
        return pinv, pinv
    prinv = np.argsort(np.asarray(F.factors.prow, np.int64))
    return pinv, pinv[prinv]


def _slu_restated(F, case):
    p, i, lx = _arrays(F.factors.L)
    ux = _arrays(F.factors.U)[2]
    zl, zu = SI.lu_x_np(case.n, p, i, lx, ux)
    return p, i, zl, zu


@pytest.mark.parametrize("name", ACCURACY_SLU + GROWTH_SLU)
def test_slusol_factor_inverse_entries(cs, name):
    case = SC.BY_NAME[name]
    n = case.n
    F = _slu_factor(cs, case)
    p, i, zl, zu = _slu_restated(F, case)
    rmap, cmap = _slu_maps(F, n)
    ZL, ZU = F.inverse()
    assert cs.sparseinv_info()["kind"] == "lu"
    for Z, want in ((ZL, zl), (ZU, zu)):
        zp, zi, zx = _arrays(Z)
        assert np.array_equal(zp, p) and np.array_equal(zi, i) and zx.tobytes() == want.tobytes()
    r, c = _entries(case)
    ent = F.inverse_entries()                                      # entry (r, c) of A -> inv(A)(c, r)
    want, missing = SI.gather(n, p, i, zl, zu, rmap, cmap, c, r)
    assert missing == 0 and ent.tobytes() == want.tobytes()
    rng = np.random.default_rng(4)
    pick = rng.integers(0, len(r), 40)
    assert F.inverse_at(c[pick], r[pick]).tobytes() == ent[pick].tobytes()
    A = case.dense()
    ref = np.linalg.inv(A)
    bound = TOL.cross_bound(np.linalg.cond(A, 1))
    err = TOL.componentwise(ent, ref[c, r])
    print(name, "entries against the dense inverse, componentwise", err, "bound", bound, "max |l|", F.info()["max_abs_l"])
    if name in ACCURACY_SLU:
        assert err <= bound
    tr, mag = _trace(case, ent, False)
    print(name, "sum_q A_q inv(A)_q - n =", tr - n, "sum of magnitudes", mag)
    assert abs(tr - n) <= _trace_tol(name in ACCURACY_SLU, bound, len(r), F.info()["max_abs_l"]) * mag
    k = np.arange(n)
    want, missing = SI.gather(n, p, i, zl, zu, rmap, cmap, k, k)
    if missing:                                                    # a matching in force: most diagonals are not on the pattern
        with pytest.raises(ValueError) as e:
            F.inverse_diag()
        assert "%d of %d pairs" % (missing, n) in str(e.value)
    else:
        dg = F.inverse_diag()
        assert dg.tobytes() == want.tobytes()
        derr = TOL.componentwise(dg, np.diag(ref))
        print(name, "diagonal against the dense inverse, componentwise", derr, "bound", bound)
        if name in ACCURACY_SLU:
            assert derr <= bound
    assert (missing > 0) == name.startswith("west")
    with pytest.raises(ValueError):
        F.inverse_at([0], [-1])


@pytest.mark.parametrize("name", ["kkt-sqd", "grid24-shift"])
def test_ldlsol_answers_follow_refactor_and_survive_a_breakdown(cs, name):
    case = LC.BY_NAME[name]
    F = _ldl_factor(cs, case)
    e0 = F.inverse_entries()
    assert F.refactor(case.A2[0]) is True
    G = _ldl_factor(cs, case, 0)
    e1, z1, d1 = F.inverse_entries(), _arrays(F.inverse())[2], F.inverse_diag()
    assert e1.tobytes() != e0.tobytes()
    assert e1.tobytes() == G.inverse_entries().tobytes() and z1.tobytes() == _arrays(G.inverse())[2].tobytes()
    assert d1.tobytes() == G.inverse_diag().tobytes()
    assert z1.tobytes() == _ldl_restated(F, case)[3].tobytes()
    pinv = F.symbolic.pinv
    j0 = 0 if pinv is None else list(pinv).index(0)
    assert F.refactor(case.breaking(j0)) is False
    assert F.inverse_entries().tobytes() == e1.tobytes() and _arrays(F.inverse())[2].tobytes() == z1.tobytes()
    assert F.inverse_diag().tobytes() == d1.tobytes()


@pytest.mark.parametrize("name", ["grid24", "west-nd"])
def test_slusol_answers_follow_refactor_and_survive_a_breakdown(cs, name):
    case = SC.BY_NAME[name]
    F = _slu_factor(cs, case)
    e0 = F.inverse_entries()
    assert F.refactor(case.A2[0]) is True
    G = _slu_factor(cs, case, 0)
    e1 = F.inverse_entries()
    z1 = [_arrays(Z)[2] for Z in F.inverse()]
    assert e1.tobytes() != e0.tobytes() and e1.tobytes() == G.inverse_entries().tobytes()
    assert [z.tobytes() for z in z1] == [_arrays(Z)[2].tobytes() for Z in G.inverse()]
    _, _, zl, zu = _slu_restated(F, case)
    assert z1[0].tobytes() == zl.tobytes() and z1[1].tobytes() == zu.tobytes()
    pinv, prow = F.factors.pinv, F.factors.prow
    j0 = 0 if pinv is None else list(pinv).index(0)
    i0 = j0 if prow is None else prow[j0]
    assert F.refactor(case.breaking(i0, j0)) is False
    assert F.inverse_entries().tobytes() == e1.tobytes()
    assert [_arrays(Z)[2].tobytes() for Z in F.inverse()] == [z.tobytes() for z in z1]


def test_bad_input_raises_and_the_next_call_is_right(cs):
    c = CASES.BY_NAME["arrow24x5"]
    n, p, i = c.n, c.p, c.i
    wz, wl, wu = _want(c.name)
    L = _dev_cs(cs, n, p, i, c.lx)

    def good():
        assert _arrays(cs.sparseinv_ldl(L, c.d))[2].tobytes() == wz
        ZL, ZU = cs.sparseinv_lu(L, _dev_cs(cs, n, p, i, c.ux))
        assert _arrays(ZL)[2].tobytes() == wl and _arrays(ZU)[2].tobytes() == wu

    def bad_ldl(Lb, d, word):
        with pytest.raises(ValueError) as e:
            cs.sparseinv_ldl(Lb, d)
        assert "csx_ldl_inverse" in str(e.value) and word in str(e.value), str(e.value)
        good()

    def bad_lu(Lb, Ub, word):
        with pytest.raises(ValueError) as e:
            cs.sparseinv_lu(Lb, Ub)
        assert "csx_slu_inverse" in str(e.value) and word in str(e.value), str(e.value)
        good()

    good()
    for v in (0.0, float("nan"), float("inf")):                    # a pivot that is zero or not finite
        d = c.d.copy()
        d[17] = v
        bad_ldl(L, d, "entry of d")
        ux = c.ux.copy()
        ux[p[17]] = v
        bad_lu(L, _dev_cs(cs, n, p, i, ux), "pivot")
    bad_ldl(L, c.d[:n - 1], "entries")                             # a short d
    j = 3                                                          # column 3 of the first tree: rows 3, 4, 23
    ib = i.copy()                                                  # Ut's i differs from L's in one entry
    ib[p[j] + 1] = i[p[j] + 1] + 1
    bad_lu(L, _dev_cs(cs, n, p, ib, c.ux), "pattern of L")
    pb = p.copy()                                                  # ... its p in one entry (the same nnz)
    pb[j + 1] -= 1
    bad_lu(L, _dev_cs(cs, n, pb, i, c.ux), "pattern of L")
    one = CASES.BY_NAME["one"]                                     # another order
    bad_lu(L, _dev_cs(cs, 1, one.p, one.i, one.ux), "not one pattern")
    # an entry dropped: rows 4 < 23 of column 3 are a pair that column 4 no longer stores
    q = int(p[4] + np.nonzero(i[p[4]:p[5]] == 23)[0][0])
    pd_ = p.copy()
    pd_[5:] -= 1
    Ld = _dev_cs(cs, n, pd_, np.delete(i, q), np.delete(c.lx, q))
    bad_ldl(Ld, c.d, "not that of a Cholesky factor")
    bad_lu(Ld, _dev_cs(cs, n, pd_, np.delete(i, q), np.delete(c.ux, q)), "not that of a Cholesky factor")
    bad_ldl(Ld, c.d, "not that of a Cholesky factor")              # (its schedule is cached by now: the same answer)
    ib = i.copy()                                                  # rows out of order
    ib[p[j] + 1], ib[p[j] + 2] = i[p[j] + 2], i[p[j] + 1]
    bad_ldl(_dev_cs(cs, n, p, ib, c.lx), c.d, "ascending")
    with pytest.raises(ValueError):
        cs.sparseinv_ldl(None, c.d)
    with pytest.raises(ValueError):
        cs.sparseinv_lu(L, None)
    good()
