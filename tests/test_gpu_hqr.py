"""hqrsol_factor on the device on the cases of tests/hqr_cases.py: V.p, V.i, V.x, R.p, R.i, R.x, beta and the
statistics byte-equal to csx_hqr_host (which tests/test_hqr_cpu.py holds to the Python restatement) on the solver's own
analysis, for every case, order and value set; which kernel ran and how often; refactor against a fresh factor, a breaking
refactor that changes nothing, and a refactor after it; solves of lists and blocks for m > n, m = n, m < n and the transposed
system; refine(), condest(), logabsdet(); the errors.  The conditions relied on (omega after refinement for the committed
right-hand sides) are asserted by the CPU test."""
import numpy as np
import pytest

import hqr_cases as HC
import hqr_oracle as HO
import trans_oracle as T
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BLOCKS = (1, 3, 64, 65, 130)
WITHIN = 3


def _download(M):
    import _csx
    m, n, nnz, hv = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return p, i[:nnz], x[:nnz]


def _factor(cs, case, which="A", pin=False):
    A = case.matrix(cs, case.values(which))
    if pin:
        cs.cs_pin(A)
    return cs.hqrsol_factor(A, case.order)


def _analysis(case, F):
    """the solver's own analysis in the shape of hqr_cases.Analysis: the factored matrix is this file's, the column order and
    the rest are the product's"""
    S, mine = HC.Analysis(), case.analysis
    S.m, S.n, S.p, S.i, S.perm = mine.m, mine.n, mine.p, mine.i, mine.perm
    sym = F.symbolic
    S.q = None if sym.q is None else np.asarray(sym.q, np.int32)
    S.parent, S.pinv, S.leftmost = np.asarray(sym.parent, np.int32), np.asarray(sym.pinv[:S.m], np.int32), np.asarray(sym.leftmost, np.int32)
    S.m2, S.vnz, S.rnz = sym.m2, sym.lnz, sym.unz
    return S


def _host(case, F, x):
    out = HO.host(case, x, S=_analysis(case, F))
    assert out[0] == 0
    return out[1:]


def _is_reference(F, case, x):
    Vp, Vi, Vx, Rp, Ri, Rx, beta = ref = _host(case, F, x)
    p, i, v = _download(F.factors.L)
    assert p.tolist() == Vp.tolist() and i.tolist() == Vi.tolist() and v.tobytes() == Vx.tobytes()
    p, i, v = _download(F.factors.U)
    assert p.tolist() == Rp.tolist() and i.tolist() == Ri.tolist() and v.tobytes() == Rx.tobytes()
    assert np.asarray(F.factors.B, np.float64).tobytes() == beta.tobytes()
    d = np.abs(Rx[Rp[1:] - 1])
    got = F.info()
    assert got["breakdown"] == -1 and got["zero_diagonals"] == int(np.sum(d == 0.0))
    assert got["min_abs_r"] == d.min() and got["max_abs_r"] == d.max()
    assert (got["m"], got["n"], got["m2"], got["vnz"], got["rnz"]) == (len(F.symbolic.leftmost), len(Vp) - 1, F.symbolic.m2, Vp[-1], Rp[-1])
    return ref


def _solve_both(F, case, b, B):
    """a list solve and a block solve of every system the factor takes"""
    out = []
    if not case.solvable:                                   # a zero on R's diagonal: the factor is asserted, no solve is
        return out
    square = case.m == case.n
    for trans in ((False, True) if square else (False,)):
        x = list(b[True] if trans else b[False])
        assert F.solve(x, trans=trans) is True
        out.append(np.asarray(x).tobytes())
        out.append(F.solve(cs_mod.dvec(B[trans]), trans=trans).numpy().tobytes())
    return out


cs_mod = None


@pytest.mark.parametrize("name", HC.NAMES)
def test_factor_and_refactor_are_the_host_rule(cs, name):
    global cs_mod
    cs_mod = cs
    case = HC.BY_NAME[name]
    for which in HC.VALUE_SETS:
        F = _factor(cs, case, which)
        assert F is not None, which
        _is_reference(F, case, case.values(which))
    if name == "empty-row":
        assert F.symbolic.m2 > case.m
    assert F.info()["transposed"] is (case.m < case.n)
    # refactor: a matrix, then values, then a dvec; byte-equal to the fresh factors above (both are the host rule's bytes)
    F = _factor(cs, case, "A")
    rows_in = case.m                                        # equations of A x = b (least squares / minimum norm alike)
    b = {False: HC.rhs(case, 1, rows_in)[0].tolist(), True: HC.rhs(case, 1, case.n)[0].tolist()}
    B = {False: np.ascontiguousarray(HC.rhs(case, 3, rows_in).T), True: np.ascontiguousarray(HC.rhs(case, 3, case.n).T)}
    s0 = _solve_both(F, case, b, B)                          # every triangular plan is cached now
    assert F.refactor(case.matrix(cs, case.A2[0])) is True
    _is_reference(F, case, case.A2[0])
    # ... and must not outlive it: the next solves are a fresh factor's, byte for byte
    sa, sb = _solve_both(F, case, b, B), _solve_both(_factor(cs, case, 0), case, b, B)
    assert sa == sb
    if case.solvable and len(case.i) > 1:
        assert all(x != y for x, y in zip(sa, s0))
    assert F.refactor(case.A2[1]) is True
    _is_reference(F, case, case.A2[1])
    s1 = _solve_both(F, case, b, B)
    # a breaking refactor: False, and V.x, R.x, beta and the next solve's bytes are what they were
    S = _analysis(case, F)
    bad = case.breaking(0 if S.q is None else int(S.q[0]))
    assert F.refactor(bad) is False
    assert F.info()["breakdown"] == 0
    _, _, Vx, _, _, Rx, beta = _host(case, F, case.A2[1])
    assert _download(F.factors.L)[2].tobytes() == Vx.tobytes() and _download(F.factors.U)[2].tobytes() == Rx.tobytes()
    assert np.asarray(F.factors.B, np.float64).tobytes() == beta.tobytes()
    assert _solve_both(F, case, b, B) == s1
    # ... and the factor still takes new values
    assert F.refactor(cs.dvec(case.A2[0])) is True
    _is_reference(F, case, case.A2[0])
    # a fresh factor of the breaking values: None
    assert cs.hqrsol_factor(case.matrix(cs, bad), case.order) is None


def test_which_kernel_ran(cs):
    import _csx

    def counts(name):
        i = _factor(cs, HC.BY_NAME[name]).info()
        return i["levels"], i["launches"], i["run_launches"], i["level_launches"]

    assert HC.RUN_LEVELS == 256
    assert counts("bidiagonal") == (257, 2, 2, 0)          # the run walker alone: a launch takes RUN_LEVELS levels
    assert counts("blocks") == (2, 2, 0, 2)                # one wave per column: one wide level a launch
    assert counts("chains4") == (3, 1, 1, 0)               # the width edge: 4 columns a level go to the walker ...
    assert counts("chains5") == (3, 3, 0, 3)               # ... 5 to a wave per column
    for name in ("chains4", "chains5"):
        _is_reference(_factor(cs, HC.BY_NAME[name]), HC.BY_NAME[name], HC.BY_NAME[name].x)
    for name in ("grid24-shift", "stacked"):
        i = _factor(cs, HC.BY_NAME[name]).info()
        print(name, i)
        assert i["run_launches"] >= 1 and i["launches"] < i["levels"]      # narrow runs: fewer launches than levels
    i = _factor(cs, HC.BY_NAME["long-column"]).info()
    assert (i["window"], i["run_levels"]) == _csx.hqr_window() == (HC.WINDOW, HC.RUN_LEVELS) and i["m"] == i["window"] + 1
    assert i["long_columns"] == 1 and i["kernel_us"] > 0   # counted by the kernel: column 0 alone took the in-place path
    F = _factor(cs, HC.BY_NAME["long-column-updated"])
    assert F.info()["long_columns"] == 2                   # ... and here column 1 too, which takes a reflection
    assert F.refactor(HC.BY_NAME["long-column-updated"].A2[0]) is True and F.info()["long_columns"] == 2     # per run, not summed


def _list_chain(cs, F, case, b, second):
    """the solve by the existing list-level calls on the downloaded factors"""
    S = F.symbolic
    N = F.factors
    V, R = cs.cs_spalloc(1, 1, 1, True, False), cs.cs_spalloc(1, 1, 1, True, False)
    for M, src in ((V, N.L), (R, N.U)):
        p, i, x = _download(src)
        M.m, M.n = src.m, src.n
        M.p, M.i, M.x = p.tolist(), i.tolist() or [0], x.tolist() or [0.0]
    H = cs.csn()
    H.L, H.B = V, list(N.B)
    m, n = len(S.leftmost), V.n
    x = cs.xalloc(S.m2)
    if not second:
        cs.cs_ipvec(S.pinv, list(b), x, m)
        cs._apply_q(H, x, True)
        cs.cs_usolve(R, x)
        out = cs.xalloc(n)
        cs.cs_ipvec(S.q, x, out, n)
    else:
        cs.cs_pvec(S.q, list(b), x, n)
        cs.cs_utsolve(R, x)
        cs._apply_q(H, x, False)
        out = cs.xalloc(m)
        cs.cs_pvec(S.pinv, x, out, m)
    return np.asarray(out)


@pytest.mark.parametrize("name,trans", [("ash219", False), ("stacked", False), ("lp_afiro", False), ("grid24-shift", False),
                                        ("grid24-shift", True), ("west-nd", False), ("west-nd", True)])
def test_solves_of_lists_and_blocks(cs, name, trans):
    case = HC.BY_NAME[name]
    F = _factor(cs, case, pin=True)
    second = trans or case.m < case.n
    rows_in, rows_out = (case.n, case.m) if trans else (case.m, case.n)
    cols = HC.rhs(case, max(BLOCKS), rows_in)
    lists = []
    for c in range(max(BLOCKS)):
        x = cols[c].tolist() + [0.0] * max(rows_out - rows_in, 0)
        assert F.solve(x, trans=trans) is True
        lists.append(np.asarray(x[:rows_out]))
    for c in range(HC.BASE):
        assert lists[c].tobytes() == _list_chain(cs, F, case, cols[c], second).tobytes(), c
    for k in BLOCKS:
        X = F.solve(cs.dvec(np.ascontiguousarray(cols[:k].T)), trans=trans).numpy().reshape(rows_out, k)
        for c in range(k):
            assert X[:, c].tobytes() == lists[c].tobytes(), (k, c)
    # what was solved
    A = case.dense()
    op = A.T if trans else A
    for c in range(HC.BASE):
        r = cols[c] - op @ lists[c]
        if op.shape[0] > op.shape[1]:
            assert np.max(np.abs(op.T @ r)) <= 1e-10 * np.abs(op).max() * np.abs(cols[c]).max() * op.shape[0]
        else:
            assert np.max(np.abs(r)) <= 1e-9 * np.abs(cols[c]).max()


@pytest.mark.parametrize("name", ["west", "west-nd", "grid24-shift", "grid24-shift-natural"])
def test_refine(cs, name):
    case = HC.BY_NAME[name]
    F = _factor(cs, case, pin=True)
    for trans in (False, True):
        for k in (1, 3, 65):
            B = np.ascontiguousarray(HC.rhs(case, k).T)
            dX = cs.dvec(B)
            out = F.refine(dX, maxit=WITHIN, trans=trans)
            print(name, trans, k, "omega0 / eps", out["omega0"].max() / EPS, "omega / eps", out["omega"].max() / EPS, "steps",
                  out["steps"].max())
            assert (out["omega"] <= EPS).all() and (out["omega"] <= out["omega0"]).all() and out["steps"].max() <= WITHIN
            assert F.backward_error(dX, cs.dvec(B), trans=trans).tobytes() == out["omega"].tobytes()
        b = HC.rhs(case, 1)[0].tolist()
        x = list(b)
        one = F.refine(x, maxit=WITHIN, trans=trans)
        assert one["omega"][0] <= EPS and one["omega"][0] <= one["omega0"][0] and F.backward_error(x, b, trans=trans) == one["omega"][0]


def test_condest_and_logabsdet(cs):
    case = HC.BY_NAME["west"]
    F = _factor(cs, case)
    D = case.dense()
    want = np.abs(D).sum(axis=0).max() * np.abs(np.linalg.inv(D)).sum(axis=0).max()      # cond_1 itself
    e1, e2 = F.condest(), F.condest()
    print("west condest", e1, "cond_1", want, "dlacn2 on the dense matrix", T.condest_dense(D))
    assert e1 == e2 and want / 3.0 <= e1 <= want * (1.0 + 1e-8)      # Hager-Higham: a lower bound, within 3 in practice
    for name in HC.SQUARE:
        c = HC.BY_NAME[name]
        logabs = np.linalg.slogdet(c.dense())[1]
        assert abs(_factor(cs, c).logabsdet() - logabs) <= 1e-10 * max(abs(logabs), 1.0), name
    assert _factor(cs, HC.BY_NAME["diagonal"]).logabsdet() == -np.inf


def test_errors(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    for name in ("ash219", "lp_afiro"):
        F = _factor(cs, HC.BY_NAME[name])
        b = HC.rhs(HC.BY_NAME[name], 1)[0].tolist()
        with pytest.raises(ValueError):
            F.refine(list(b))
        with pytest.raises(ValueError):
            F.backward_error(list(b), list(b))
        with pytest.raises(ValueError):
            F.condest()
        with pytest.raises(ValueError):
            F.solve(list(b), trans=True)
    case = HC.BY_NAME["grid24-shift"]
    A = cs.cs_pin(case.matrix(cs))
    F = cs.hqrsol_factor(A, case.order)
    S = _analysis(case, F)

    def factor(h, q=S.q, parent=S.parent, pinv=S.pinv, leftmost=S.leftmost, m2=S.m2):
        out, ok = _csx.new_handle(), C.c_int(0)
        st = lib.csx_hqr_factor(h, _csx.pi(q), _csx.pi(parent), _csx.pi(pinv), _csx.pi(leftmost), m2, out, ok)
        if st == _csx.OK:
            assert ok.value == 1
            _csx.free(out)
        return st

    assert factor(A._dev.handle) == _csx.OK
    P = cs.cs_spalloc(case.m, case.n, len(case.i), False, False)          # pattern only
    P.p, P.i, P.x = case.p.tolist(), case.i.tolist(), None
    assert factor(cs.cs_pin(P)._dev.handle) == _csx.EINVAL
    wide = HC.BY_NAME["lp_afiro"]                                          # m < n
    W = cs.cs_pin(wide.matrix(cs))
    assert factor(W._dev.handle) == _csx.EINVAL
    assert factor(A._dev.handle, parent=np.full(case.n, -1, np.int32)) == _csx.EINVAL      # symbolic arrays that are not A's
    assert factor(A._dev.handle, q=None) == _csx.EINVAL
    twice = S.pinv.copy()
    twice[1] = twice[0]
    assert factor(A._dev.handle, pinv=twice) == _csx.EINVAL
    assert factor(A._dev.handle, leftmost=np.zeros(case.m, np.int32)) == _csx.EINVAL
    assert factor(A._dev.handle, m2=case.m - 1) == _csx.EINVAL
    # refactor: another pattern with the same shape and entry count, a short vector
    i2 = case.i.copy()
    first_off = int(np.flatnonzero(case.i != case.cols)[0])
    i2[first_off] = 0 if i2[first_off] != 0 else 1
    B = cs.cs_spalloc(case.m, case.n, len(case.i), True, False)
    B.p, B.i, B.x = case.p.tolist(), i2.tolist(), case.x.tolist()
    before = _download(F.factors.L)[2].tobytes(), _download(F.factors.U)[2].tobytes()
    with pytest.raises(ValueError):
        F.refactor(B)
    with pytest.raises(ValueError):
        F.refactor(case.x[:-1])
    assert (_download(F.factors.L)[2].tobytes(), _download(F.factors.U)[2].tobytes()) == before
    ok = C.c_int(0)
    assert lib.csx_hqr_refactor(A._dev.handle, A._dev.handle, ok) == _csx.EINVAL         # not a factor
    # the Python face
    Tr = cs.cs_spalloc(3, 3, 1, True, True)
    assert cs.hqrsol_factor(Tr) is None and cs.hqrsol_factor(A, 7) is None
    with pytest.raises(TypeError):
        cs.hqrsol_factor(P)
