"""ldlsol_factor on the device on the cases of tests/ldl_cases.py: L.p, L.i, L.x and d byte-equal to csx_ldl_host
(which tests/test_ldl_cpu.py holds to the Python restatement) for every case, order and value set; which kernel ran; refactor
against a fresh factor, a breaking refactor that changes nothing, and a refactor after it; perturbed pivots; solves of lists
and blocks; csx_block_div_rows against numpy; refine(), inertia(), logdet(), backward_error(A=), condest(); the CSX_EINVAL cases
of the C ABI.  The conditions relied on (omega of the unrefined solves, growth, the gap at sigma) are asserted by the CPU test.

Observed on an MI355X: kkt-sqd unrefined, list solves and blocks of every width under exact=None and exact=True: 3.07 - 3.59 eps
(the rounding-equal order of a block coincides with the exact one on these factors: no small components for the matrix cores);
refine() on the shifted grid from 432 - 1 462 eps to <= 0.91 eps in one step, on the perturbed case from 1.4e9 - 6.2e9 eps to
0.99 eps in two; condest() of the shifted grid 1645.76 against the dense cond_1 1645.76; the block of 130 independent random
columns (byte-equal to its list solves, not bounded): 2.3 - 5.7 eps at the committed order, 2.8 - 6.2 eps in natural order."""
import numpy as np
import pytest

import ldl_cases as LC
import ldl_oracle as LO
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BLOCKS = (1, 3, 64, 65, 130)


def _download(cs, M):
    import _csx
    m, n, nnz, hv = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return p, i[:nnz], x[:nnz]


def _factor(cs, case, which="A", perturb=None, exact=None, pin=False):
    A = case.matrix(cs, case.values(which))
    if pin:
        cs.cs_pin(A)
    return cs.ldlsol_factor(A, case.order, case.perturb if perturb is None else perturb, exact)


def _is_reference(cs, F, case, which):
    Lp, Li, _ = LO.pattern_of(case)
    Lx, d, info = LO.reference(case, which)
    p, i, x = _download(cs, F.factors.L)
    assert p.tolist() == Lp and i.tolist() == Li
    assert x.tobytes() == Lx.tobytes(), which
    assert F.factors.D.numpy().reshape(-1).tobytes() == d.tobytes(), which
    got = F.info()
    assert (got["pos"], got["neg"], got["perturbed"], got["breakdown"]) == info, which
    assert F.inertia() == info[:2]
    off = np.ones(len(Lx), bool)
    off[np.asarray(Lp[:-1])] = False
    assert got["min_abs_d"] == np.min(np.abs(d)) and got["max_abs_d"] == np.max(np.abs(d))
    assert got["max_abs_l"] == (np.max(np.abs(Lx[off])) if off.any() else 0.0)


@pytest.mark.parametrize("name", LC.NAMES)
def test_factor_and_refactor_are_the_host_rule(cs, name):
    case = LC.BY_NAME[name]
    pinv = LO.pinv_of(case)
    for which in LC.VALUE_SETS:
        F = _factor(cs, case, which)
        assert F is not None, which
        assert F.symbolic.pinv == pinv
        _is_reference(cs, F, case, which)
    # refactor: a matrix, then values; byte-equal to the fresh factors above (both are the host rule's bytes)
    F = _factor(cs, case, "A")
    b = LC.rhs(case, 1)[0].tolist()
    B = np.ascontiguousarray(LC.rhs(case, 3).T)
    x0, X0 = list(b), cs.dvec(B)
    assert F.solve(x0) is True and F.solve(X0) is True              # the triangular plans of A's factor are cached now
    assert F.refactor(case.matrix(cs, case.A2[0])) is True
    _is_reference(cs, F, case, 0)
    assert F.operator_info()["source"] == "refactored"
    # ... and must not outlive it: the next solves are a fresh factor's, byte for byte
    fresh = _factor(cs, case, 0)
    xa, xb, Xa, Xb = list(b), list(b), cs.dvec(B), cs.dvec(B)
    assert F.solve(xa) is True and fresh.solve(xb) is True and F.solve(Xa) is True and fresh.solve(Xb) is True
    assert np.asarray(xa).tobytes() == np.asarray(xb).tobytes() and Xa.numpy().tobytes() == Xb.numpy().tobytes()
    if case.n > 1:
        assert np.asarray(xa).tobytes() != np.asarray(x0).tobytes()
    assert F.refactor(case.A2[1]) is True
    _is_reference(cs, F, case, 1)
    x1 = list(b)
    assert F.solve(x1) is True
    # a breaking refactor: False, and L.x, d and the next solve's bytes are what they were
    bad = case.breaking(LO.first_column(case))
    assert F.refactor(bad) is False
    assert F.info()["breakdown"] == 0
    p, i, x = _download(cs, F.factors.L)
    assert x.tobytes() == LO.reference(case, 1)[0].tobytes()
    assert F.factors.D.numpy().reshape(-1).tobytes() == LO.reference(case, 1)[1].tobytes()
    assert F.inertia() == LO.reference(case, 1)[2][:2]
    x2 = list(b)
    assert F.solve(x2) is True and np.asarray(x2).tobytes() == np.asarray(x1).tobytes()
    # ... and the factor still takes new values
    assert F.refactor(cs.dvec(case.A2[0])) is True
    _is_reference(cs, F, case, 0)
    # a fresh factor of the breaking values: None
    A = case.matrix(cs, bad)
    assert cs.ldlsol_factor(A, case.order, case.perturb) is None


def test_which_kernel_ran(cs):
    import _csx
    i = _factor(cs, LC.BY_NAME["chain"]).info()
    assert (i["levels"], i["launches"], i["run_launches"], i["level_launches"]) == (257, 1, 1, 0)      # the run walker alone
    i = _factor(cs, LC.BY_NAME["leaves"]).info()
    assert (i["levels"], i["launches"], i["run_launches"], i["level_launches"]) == (2, 2, 0, 2)        # one wave per column
    for name, counts in (("chains4", (3, 1, 1, 0)), ("chains5", (3, 3, 0, 3))):     # the width edge: 4 columns a level, then 5
        F = _factor(cs, LC.BY_NAME[name])
        i = F.info()
        assert (i["levels"], i["launches"], i["run_launches"], i["level_launches"]) == counts, name
        _is_reference(cs, F, LC.BY_NAME[name], "A")
    for name in ("grid24-shift", "dups"):
        i = _factor(cs, LC.BY_NAME[name]).info()
        assert i["level_launches"] >= 1 and i["run_launches"] >= 1 and i["launches"] < i["levels"]     # wide levels, narrow runs
        assert i["long_columns"] == 0
    i = _factor(cs, LC.BY_NAME["long-column"]).info()
    assert i["window"] == _csx.ldl_window() == LC.WINDOW and i["n"] == i["window"] + 1
    assert i["long_columns"] == 1                          # counted by the kernel: column 0 alone took the in-place path
    F = _factor(cs, LC.BY_NAME["long-column-updated"])
    assert F.info()["long_columns"] == 2                   # ... and here column 1 too, which takes an update
    assert F.refactor(LC.BY_NAME["long-column-updated"].A2[0]) is True and F.info()["long_columns"] == 2     # per run, not summed
    assert i["kernel_us"] > 0 and i["lnz"] == LO.pattern_of(LC.BY_NAME["long-column"])[0][-1]


def test_a_zero_pivot_is_a_breakdown_unless_perturbed(cs):
    case = LC.BY_NAME["kkt-zero"]
    assert _factor(cs, case, perturb=0.0) is None
    F = _factor(cs, case)
    info = LO.reference(case, "A")[2]
    assert info[2] >= 1 and F.info()["perturbed"] == info[2] and F.inertia() == (LC.KKT_NH, LC.KKT_NC)


# printed with every figure, so that a run with -s shows them
SOLVE_NOTE = "kkt-sqd unrefined, omega / eps per block width"


@pytest.mark.parametrize("name", ["kkt-sqd", "kkt-sqd-natural"])
def test_solves_of_lists_and_blocks(cs, name):
    case = LC.BY_NAME[name]
    n = case.n
    F, FX = _factor(cs, case, pin=True), _factor(cs, case, exact=True, pin=True)
    cols = LC.rhs(case, max(BLOCKS))
    lists = []
    for c in range(max(BLOCKS)):
        x = cols[c].tolist()
        assert F.solve(x) is True
        lists.append(np.asarray(x))
        if c < LC.BASE:
            w = F.backward_error(x, cols[c].tolist())
            print(SOLVE_NOTE, name, "list", c, w / EPS)
            assert isinstance(w, float) and w <= 4 * EPS
    for k in BLOCKS:
        B = np.ascontiguousarray(cols[:k].T)
        dX = cs.dvec(B)
        assert FX.solve(dX) is True
        X = dX.numpy().reshape(n, k)
        for c in range(k):
            assert X[:, c].tobytes() == lists[c].tobytes(), (k, c)
        w = FX.backward_error(dX, cs.dvec(B))
        print(SOLVE_NOTE, name, "exact block", k, w.max() / EPS)
        assert w.shape == (k,) and (w <= 4 * EPS).all()
        dX = cs.dvec(B)
        assert F.solve(dX) is True
        w = F.backward_error(dX, cs.dvec(B))
        print(SOLVE_NOTE, name, "block", k, w.max() / EPS)
        assert (w <= 4 * EPS).all()
    # 130 independent columns, so that the wide path sees varied data: byte-equal to the list solves, no bound on omega
    R = LC.random_block(case, max(BLOCKS))
    dX = cs.dvec(R)
    assert FX.solve(dX) is True
    X = dX.numpy().reshape(n, max(BLOCKS))
    w = FX.backward_error(dX, cs.dvec(R))
    print(SOLVE_NOTE, name, "independent columns", w.min() / EPS, w.max() / EPS)
    for c in range(max(BLOCKS)):
        x = R[:, c].tolist()
        assert FX.solve(x) is True and X[:, c].tobytes() == np.asarray(x).tobytes(), c


@pytest.mark.parametrize("k,offset", [(1, 0), (3, 0), (4, 0), (64, 0), (65, 0), (4, 1), (6, 3), (2, 1)])
def test_block_div_rows_is_numpys_division(cs, k, offset):
    """odd and even widths; offset: the block starts that many doubles into an allocation (odd: not 16-byte aligned)"""
    import _csx
    rows = 1037
    rng = np.random.default_rng(100 + k + offset)
    X, d = rng.uniform(-1.0, 1.0, (rows, k)), rng.uniform(0.5, 2.0, rows) * np.where(rng.uniform(size=rows) < 0.5, -1.0, 1.0)
    whole = np.concatenate([np.full(offset, 7.0), X.reshape(-1), np.full(3, 9.0)])
    dw, dd = cs.dvec(whole), cs.dvec(d)
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_vec_wrap(_csx.C.c_void_p(dw.device_ptr() + 8 * offset), rows * k, h), "csx_vec_wrap")
    try:
        _csx.check(_csx.lib().csx_block_div_rows(h, dd.handle, rows, k), "csx_block_div_rows")
    finally:
        _csx.free(h)
    expect = np.concatenate([np.full(offset, 7.0), (X / d[:, None]).reshape(-1), np.full(3, 9.0)])
    assert dw.numpy().reshape(-1).tobytes() == expect.tobytes()


@pytest.mark.parametrize("name", ["grid24-shift", "grid24-shift-natural", "kkt-zero"])
def test_refine(cs, name):
    case = LC.BY_NAME[name]
    n = case.n
    for exact in (None, True):
        F = _factor(cs, case, exact=exact, pin=True)
        for k in (1, 3, 65):
            B = np.ascontiguousarray(LC.rhs(case, k).T)
            dX = cs.dvec(B)
            out = F.refine(dX)
            print(name, exact, k, "omega0 / eps", out["omega0"].max() / EPS, "omega / eps", out["omega"].max() / EPS,
                  "steps", out["steps"].max())
            assert (out["omega"] <= 4 * EPS).all() and (out["omega"] <= out["omega0"]).all()
            assert F.backward_error(dX, cs.dvec(B)).tobytes() == out["omega"].tobytes()
        b = LC.rhs(case, 1)[0].tolist()
        x = list(b)
        one = F.refine(x)
        assert one["omega"][0] <= 4 * EPS and one["omega"][0] <= one["omega0"][0] and F.backward_error(x, b) == one["omega"][0]


@pytest.mark.parametrize("name", LC.SMALL)
def test_inertia_and_logdet_against_the_dense_matrix(cs, name):
    case = LC.BY_NAME[name]
    F = _factor(cs, case)
    S = case.dense()
    w = np.linalg.eigvalsh(S)
    assert F.inertia() == (int(np.sum(w > 0)), int(np.sum(w < 0)))
    if case.perturb == 0.0:                      # (a perturbed factor is the factor of a nearby matrix)
        sign, logabs = np.linalg.slogdet(S)
        s, l = F.logdet()
        assert s == sign and abs(l - logabs) <= 1e-10 * abs(logabs)


def test_backward_error_against_another_matrix_and_condest(cs):
    case = LC.BY_NAME["grid24-shift"]
    F = _factor(cs, case, pin=True)
    b = LC.rhs(case, 1)[0].tolist()
    x = list(b)
    assert F.solve(x) is True
    A2 = cs.cs_pin(case.matrix(cs, case.A2[0]))
    w = F.backward_error(x, b, A=A2)
    assert np.isfinite(w) and w >= 0.0 and F.operator_info()["source"] == "given"
    out = F.refine(list(b), A=A2)
    assert np.isfinite(out["omega"]).all() and (out["omega"] <= out["omega0"]).all()
    c = F.condest()
    dense = np.linalg.cond(case.dense(), 1)
    print("condest", c, "cond_1", dense)
    assert np.isfinite(c) and 1.0 <= c <= dense * (1 + 1e-8)
    assert np.isfinite(F.condest(A=A2)) and F.condest(A=A2) >= 1.0


def test_bad_arguments(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    case = LC.BY_NAME["grid24-shift-natural"]
    A = cs.cs_pin(case.matrix(cs))
    S = cs.cs_schol(0, A)
    parent, cp = _csx.i32(S.parent), _csx.i32(S.cp)

    def factor(h, parent=parent, cp=cp, tau=0.0):
        out, ok = _csx.new_handle(), C.c_int(0)
        st = lib.csx_ldl_factor(h, _csx.pi(parent), _csx.pi(cp), None, tau, out, ok)
        if st == _csx.OK:
            assert ok.value == 1
            _csx.free(out)
        return st

    assert factor(A._dev.handle) == _csx.OK
    assert factor(A._dev.handle, tau=-1.0) == _csx.EINVAL and factor(A._dev.handle, tau=float("nan")) == _csx.EINVAL
    P = cs.cs_spalloc(case.n, case.n, len(case.i), False, False)          # pattern only
    P.p, P.i, P.x = case.p.tolist(), case.i.tolist(), None
    assert factor(cs.cs_pin(P)._dev.handle) == _csx.EINVAL
    R = cs.cs_spalloc(case.n + 1, case.n, len(case.i), True, False)        # not square
    R.p, R.i, R.x = case.p.tolist(), case.i.tolist(), case.x.tolist()
    assert factor(cs.cs_pin(R)._dev.handle) == _csx.EINVAL
    wrong = cp.copy()                                                      # an S that is not A's: the counts, then the tree
    wrong[1:] += 1
    assert factor(A._dev.handle, cp=wrong) == _csx.EINVAL
    assert factor(A._dev.handle, parent=np.full(case.n, -1, np.int32)) == _csx.EINVAL
    # refactor: another pattern with the same shape and entry count, a short vector, no matrix
    F = cs.ldlsol_factor(A, 0)
    i2 = case.i.copy()
    first_off = int(np.flatnonzero(case.i != case.cols)[0])
    i2[first_off] = 0 if i2[first_off] != 0 else 1
    B = cs.cs_spalloc(case.n, case.n, len(case.i), True, False)
    B.p, B.i, B.x = case.p.tolist(), i2.tolist(), case.x.tolist()
    before = _download(cs, F.factors.L)[2].tobytes()
    with pytest.raises(ValueError):
        F.refactor(B)
    with pytest.raises(ValueError):
        F.refactor(case.x[:-1])
    assert _download(cs, F.factors.L)[2].tobytes() == before
    # csx_block_div_rows: short vectors, no columns
    X, d = cs.dvec(np.ones(12)), cs.dvec(np.ones(3))
    assert lib.csx_block_div_rows(X.handle, d.handle, 3, 4) == _csx.OK
    assert lib.csx_block_div_rows(X.handle, d.handle, 4, 3) == _csx.EINVAL      # d is short
    assert lib.csx_block_div_rows(X.handle, d.handle, 3, 5) == _csx.EINVAL      # X is short
    assert lib.csx_block_div_rows(X.handle, d.handle, 3, 0) == _csx.EINVAL
    # the Python face
    T = cs.cs_spalloc(3, 3, 1, True, True)
    assert cs.ldlsol_factor(T) is None and cs.ldlsol_factor(R) is None
    with pytest.raises(ValueError):
        cs.ldlsol_factor(A, 0, perturb=-1.0)
