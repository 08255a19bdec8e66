"""slusol_factor on the device on the cases of tests/slu_cases.py: L.p, L.i, L.x, Ut.x and the statistics
byte-equal to csx_slu_host (which tests/test_slu_cpu.py holds to the Python restatement) for every case, order and value set;
which kernel ran and how often; refactor against a fresh factor, a breaking refactor that changes nothing, and a refactor after it;
perturbed pivots; solves of lists and blocks, forward and transposed; refine(), condest(), logdet(); the `match` argument; the
CSX_EINVAL cases of the C ABI.  The conditions relied on (omega before and after refinement for the committed seeds) are
asserted by the CPU test."""
import numpy as np
import pytest

import slu_cases as SC
import slu_oracle as SO
import trans_oracle as T
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
BLOCKS = (1, 3, 64, 65, 130)


def _download(M):
    import _csx
    m, n, nnz, hv = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return p, i[:nnz], x[:nnz]


def _factor(cs, case, which="A", perturb=None, exact=None, pin=False):
    A = case.matrix(cs, case.values(which))
    if pin:
        cs.cs_pin(A)
    return cs.slusol_factor(A, case.order, case.perturb if perturb is None else perturb, case.match, case.match_seed, exact)


def _is_reference(F, case, which):
    Lp, Li, _ = SO.pattern_of(case)
    Lx, Ux, info = SO.reference(case, which)
    for M, ref in ((F.factors.L, Lx), (F.factors.U, Ux)):
        p, i, x = _download(M)
        assert p.tolist() == Lp and i.tolist() == Li
        assert x.tobytes() == ref.tobytes(), which
    got = F.info()
    assert (got["pos"], got["neg"], got["perturbed"], got["breakdown"]) == info, which
    d = Ux[np.asarray(Lp[:-1])]
    off = np.ones(len(Lx), bool)
    off[np.asarray(Lp[:-1])] = False
    assert got["min_abs_d"] == np.min(np.abs(d)) and got["max_abs_d"] == np.max(np.abs(d))
    assert got["max_abs_l"] == (np.max(np.abs(Lx[off])) if off.any() else 0.0)
    assert got["max_abs_u"] == (np.max(np.abs(Ux[off])) if off.any() else 0.0)


@pytest.mark.parametrize("name", SC.NAMES)
def test_factor_and_refactor_are_the_host_rule(cs, name):
    case = SC.BY_NAME[name]
    for which in SC.VALUE_SETS:
        F = _factor(cs, case, which)
        assert F is not None, which
        assert F.factors.pinv == SO.pinv_of(case)
        assert F.factors.prow == (None if case.prow is None else case.prow.tolist())      # the device's matching is the committed one
        _is_reference(F, case, which)
    # refactor: a matrix, then values; byte-equal to the fresh factors above (both are the host rule's bytes)
    F = _factor(cs, case, "A")
    b = SC.rhs(case, 1)[0].tolist()
    B = np.ascontiguousarray(SC.rhs(case, 3).T)
    x0, X0, t0 = list(b), cs.dvec(B), list(b)
    assert F.solve(x0) is True and F.solve(X0) is True and F.solve(t0, trans=True) is True     # every triangular plan is cached now
    assert F.refactor(case.matrix(cs, case.A2[0])) is True
    _is_reference(F, case, 0)
    # ... and must not outlive it: the next solves are a fresh factor's, byte for byte
    fresh = _factor(cs, case, 0)
    xa, xb, Xa, Xb, ta, tb = list(b), list(b), cs.dvec(B), cs.dvec(B), list(b), list(b)
    assert F.solve(xa) is True and fresh.solve(xb) is True and F.solve(Xa) is True and fresh.solve(Xb) is True
    assert F.solve(ta, trans=True) is True and fresh.solve(tb, trans=True) is True
    assert np.asarray(xa).tobytes() == np.asarray(xb).tobytes() and Xa.numpy().tobytes() == Xb.numpy().tobytes()
    assert np.asarray(ta).tobytes() == np.asarray(tb).tobytes()
    if case.n > 1:
        assert np.asarray(xa).tobytes() != np.asarray(x0).tobytes() and np.asarray(ta).tobytes() != np.asarray(t0).tobytes()
    assert F.refactor(case.A2[1]) is True
    _is_reference(F, case, 1)
    x1 = list(b)
    assert F.solve(x1) is True
    # a breaking refactor: False, and L.x, Ut.x and the next solve's bytes are what they were
    bad = case.breaking(*SO.first_pivot(case))
    assert F.refactor(bad) is False
    assert F.info()["breakdown"] == 0
    assert _download(F.factors.L)[2].tobytes() == SO.reference(case, 1)[0].tobytes()
    assert _download(F.factors.U)[2].tobytes() == SO.reference(case, 1)[1].tobytes()
    assert (F.info()["pos"], F.info()["neg"]) == SO.reference(case, 1)[2][:2]
    x2 = list(b)
    assert F.solve(x2) is True and np.asarray(x2).tobytes() == np.asarray(x1).tobytes()
    # ... and the factor still takes new values
    assert F.refactor(cs.dvec(case.A2[0])) is True
    _is_reference(F, case, 0)
    # a fresh factor of the breaking values: None
    assert cs.slusol_factor(case.matrix(cs, bad), case.order, case.perturb, case.match, case.match_seed) is None


def test_which_kernel_ran(cs):
    import _csx

    def counts(name):
        i = _factor(cs, SC.BY_NAME[name]).info()
        return i["levels"], i["launches"], i["run_launches"], i["level_launches"]

    assert SC.RUN_LEVELS == 256
    assert counts("chain256") == (256, 1, 1, 0)            # the run walker alone: one launch takes RUN_LEVELS levels
    assert counts("chain257") == (257, 2, 2, 0)            # ... a longer run is several
    assert counts("blocks") == (2, 2, 0, 2)                # one wave per column: one wide level a launch
    assert counts("chains4") == (3, 1, 1, 0)               # the width edge: 4 columns a level go to the walker ...
    assert counts("chains5") == (3, 3, 0, 3)               # ... 5 to a wave per column
    for name in ("chains4", "chains5"):
        _is_reference(_factor(cs, SC.BY_NAME[name]), SC.BY_NAME[name], "A")
    for name in ("grid24-shift", "dups", "one-sided"):
        i = _factor(cs, SC.BY_NAME[name]).info()
        assert i["level_launches"] >= 1 and i["run_launches"] >= 1 and i["launches"] < i["levels"]     # wide levels, narrow runs
        assert i["long_columns"] == 0
    i = _factor(cs, SC.BY_NAME["long-column"]).info()
    assert (i["window"], i["run_levels"]) == _csx.slu_window() == (SC.WINDOW, SC.RUN_LEVELS) and i["n"] == i["window"] + 1
    assert i["long_columns"] == 1                          # counted by the kernel: column 0 alone took the in-place path
    assert i["kernel_us"] > 0 and i["lnz"] == SO.pattern_of(SC.BY_NAME["long-column"])[0][-1]
    F = _factor(cs, SC.BY_NAME["long-column-updated"])
    assert F.info()["long_columns"] == 2                   # ... and here column 1 too, which takes an update
    assert F.refactor(SC.BY_NAME["long-column-updated"].A2[0]) is True and F.info()["long_columns"] == 2     # per run, not summed


def test_a_zero_pivot_is_a_breakdown_unless_perturbed(cs):
    case = SC.BY_NAME["saddle"]
    assert _factor(cs, case, perturb=0.0) is None
    F = _factor(cs, case)
    info = SO.reference(case, "A")[2]
    assert 9 <= info[2] <= 17 and F.info()["perturbed"] == info[2]


@pytest.mark.parametrize("name", ["grid24", "west-nd", "saddle-natural"])
def test_solves_of_lists_and_blocks(cs, name):
    """the exact order of a block is the list solves' column by column, forward and transposed, at every width; solves in the
    rounding-equal order of a block solve the system as well as the list solves do"""
    case = SC.BY_NAME[name]
    n = case.n
    F, FX = _factor(cs, case, pin=True), _factor(cs, case, exact=True, pin=True)
    cols = SC.rhs(case, max(BLOCKS))
    R = SC.random_block(case, max(BLOCKS))
    for trans in (False, True):
        lists = []
        for c in range(max(BLOCKS)):
            x = cols[c].tolist()
            assert F.solve(x, trans=trans) is True
            lists.append(np.asarray(x))
        w_list = max(F.backward_error(lists[c].tolist(), cols[c].tolist(), trans=trans) for c in range(SC.BASE))
        for k in BLOCKS:
            B = np.ascontiguousarray(cols[:k].T)
            dX = cs.dvec(B)
            assert FX.solve(dX, trans=trans) is True
            X = dX.numpy().reshape(n, k)
            for c in range(k):
                assert X[:, c].tobytes() == lists[c].tobytes(), (trans, k, c)
            dX = cs.dvec(B)
            assert F.solve(dX, trans=trans) is True
            w = F.backward_error(dX, cs.dvec(B), trans=trans)
            print(name, "trans", trans, "block", k, "omega / eps", w.max() / EPS, "lists", w_list / EPS)
            assert w.shape == (k,) and (w <= 4.0 * w_list + 4 * EPS).all()
        # 130 independent columns, so that the wide path sees varied data: byte-equal to the list solves
        dX = cs.dvec(R)
        assert FX.solve(dX, trans=trans) is True
        X = dX.numpy().reshape(n, max(BLOCKS))
        for c in range(max(BLOCKS)):
            x = R[:, c].tolist()
            assert FX.solve(x, trans=trans) is True and X[:, c].tobytes() == np.asarray(x).tobytes(), (trans, c)


# (name, omega0 of every column at least, steps within which omega <= eps): what tests/test_slu_cpu.py established
REFINE = [("grid24-shift", 16.0, 3), ("grid24-shift-natural", 16.0, 3), ("one-sided", 16.0, 3), ("west", 0.0, 3), ("west-nd", 0.0, 3),
          ("fs183", 0.0, 3), ("saddle-natural", 0.0, 3), ("saddle", 0.0, 4)]


@pytest.mark.parametrize("name,least,steps", REFINE)
def test_refine(cs, name, least, steps):
    case = SC.BY_NAME[name]
    for exact in (None, True):
        F = _factor(cs, case, exact=exact, pin=True)
        for k in (1, 3, 65):
            B = np.ascontiguousarray(SC.rhs(case, k).T)
            dX = cs.dvec(B)
            out = F.refine(dX, maxit=steps)
            print(name, exact, k, "omega0 / eps", out["omega0"].min() / EPS, out["omega0"].max() / EPS, "omega / eps",
                  out["omega"].max() / EPS, "steps", out["steps"].max())
            assert (out["omega0"] >= least * EPS).all()
            assert (out["omega"] <= EPS).all() and (out["omega"] <= out["omega0"]).all() and out["steps"].max() <= steps
            assert F.backward_error(dX, cs.dvec(B)).tobytes() == out["omega"].tobytes()
        b = SC.rhs(case, 1)[0].tolist()
        x = list(b)
        one = F.refine(x, maxit=steps)
        assert one["omega"][0] <= EPS and one["omega"][0] <= one["omega0"][0] and F.backward_error(x, b) == one["omega"][0]
    # the transposed system on the same factor
    tr = F.refine(cs.dvec(np.ascontiguousarray(SC.rhs(case, 3).T)), trans=True)
    print(name, "transposed omega0 / eps", tr["omega0"].max() / EPS, "omega / eps", tr["omega"].max() / EPS)
    assert (tr["omega"] <= tr["omega0"]).all() and np.isfinite(tr["omega"]).all()


@pytest.mark.parametrize("name", ["one", "grid24", "west", "west-nd"])
def test_condest(cs, name):
    case = SC.BY_NAME[name]
    F = _factor(cs, case)
    want = T.condest_dense(case.dense())
    e1, e2 = F.condest(), F.condest()
    print(name, "condest", e1, "dense", want)
    assert e1 == e2 and abs(e1 - want) <= 1e-10 * want


@pytest.mark.parametrize("name", [n for n in SC.NAMES if SC.BY_NAME[n].perturb == 0.0])
def test_logdet_against_the_dense_matrix(cs, name):
    case = SC.BY_NAME[name]
    sign, logabs = np.linalg.slogdet(case.dense())
    s, l = _factor(cs, case).logdet()
    assert s == sign and abs(l - logabs) <= 1e-10 * max(abs(logabs), 1.0)


def test_the_match_argument(cs):
    west, grid = SC.BY_NAME["west"], SC.BY_NAME["grid24-shift-natural"]
    prow = cs.maxtrans_array(west.matrix(cs), west.match_seed)[west.n:].tolist()
    assert prow == west.prow.tolist()
    # None: only when a diagonal entry is not stored
    F = cs.slusol_factor(west.matrix(cs), 0, 0.0, None, west.match_seed)
    assert F.info()["matched"] is True and F.factors.prow == prow
    F = cs.slusol_factor(grid.matrix(cs), 0)
    assert F.info()["matched"] is False and F.factors.prow is None
    # True: always -- on a full diagonal any maximum matching is taken; the factor still solves the system
    F = cs.slusol_factor(grid.matrix(cs), 0, 0.0, True, 5)
    assert F.info()["matched"] is True and sorted(F.factors.prow) == list(range(grid.n))
    b = SC.rhs(grid, 1)[0].tolist()
    x = list(b)
    out = F.refine(x)
    assert out["omega"][0] <= out["omega0"][0] and np.isfinite(out["omega"][0])
    # False: never -- west0067 has 65 zero diagonal entries: the first pivot is zero
    assert cs.slusol_factor(west.matrix(cs), 0, 0.0, False) is None
    # structurally singular: two columns with one row between them
    S = cs.cs_spalloc(3, 3, 4, True, False)
    S.p, S.i, S.x = [0, 1, 2, 4], [0, 0, 1, 2], [1.0, 2.0, 3.0, 4.0]
    assert cs.slusol_factor(S) is None and cs.slusol_factor(S, match=True) is None


def test_bad_arguments(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    case = SC.BY_NAME["grid24-shift-natural"]
    n = case.n
    A = cs.cs_pin(case.matrix(cs))
    _, _, parent = SO.pattern_of(case)
    parent, cp = _csx.i32(parent), _csx.i32(SO.pattern_of(case)[0])

    def factor(h, parent=parent, cp=cp, prow=None, pinv=None, tau=0.0):
        out, ok = _csx.new_handle(), C.c_int(0)
        st = lib.csx_slu_factor(h, _csx.pi(parent), _csx.pi(cp), _csx.pi(prow), _csx.pi(pinv), tau, out, ok)
        if st == _csx.OK:
            assert ok.value == 1
            _csx.free(out)
        return st

    assert factor(A._dev.handle) == _csx.OK
    assert factor(A._dev.handle, tau=-1.0) == _csx.EINVAL and factor(A._dev.handle, tau=float("nan")) == _csx.EINVAL
    P = cs.cs_spalloc(n, n, len(case.i), False, False)                     # pattern only
    P.p, P.i, P.x = case.p.tolist(), case.i.tolist(), None
    assert factor(cs.cs_pin(P)._dev.handle) == _csx.EINVAL
    R = cs.cs_spalloc(n + 1, n, len(case.i), True, False)                  # not square
    R.p, R.i, R.x = case.p.tolist(), case.i.tolist(), case.x.tolist()
    assert factor(cs.cs_pin(R)._dev.handle) == _csx.EINVAL
    wrong = cp.copy()                                                      # an S that is not A's: the counts, then the tree
    wrong[1:] += 1
    assert factor(A._dev.handle, cp=wrong) == _csx.EINVAL
    assert factor(A._dev.handle, parent=np.full(n, -1, np.int32)) == _csx.EINVAL
    twice = np.arange(n, dtype=np.int32)                                   # not a permutation, as prow and as pinv
    twice[1] = 0
    assert factor(A._dev.handle, prow=twice) == _csx.EINVAL and factor(A._dev.handle, pinv=twice) == _csx.EINVAL
    swap = np.arange(n, dtype=np.int32)                                    # permutations that are not this S's
    swap[[0, n - 1]] = [n - 1, 0]
    assert factor(A._dev.handle, prow=swap) == _csx.EINVAL and factor(A._dev.handle, pinv=swap) == _csx.EINVAL
    # refactor: another pattern with the same shape and entry count, a short vector
    F = cs.slusol_factor(A, 0)
    i2 = case.i.copy()
    first_off = int(np.flatnonzero(case.i != case.cols)[0])
    i2[first_off] = 0 if i2[first_off] != 0 else 1
    B = cs.cs_spalloc(n, n, len(case.i), True, False)
    B.p, B.i, B.x = case.p.tolist(), i2.tolist(), case.x.tolist()
    before = _download(F.factors.L)[2].tobytes(), _download(F.factors.U)[2].tobytes()
    with pytest.raises(ValueError):
        F.refactor(B)
    with pytest.raises(ValueError):
        F.refactor(case.x[:-1])
    assert (_download(F.factors.L)[2].tobytes(), _download(F.factors.U)[2].tobytes()) == before
    # the Python face
    Tr = cs.cs_spalloc(3, 3, 1, True, True)
    assert cs.slusol_factor(Tr) is None and cs.slusol_factor(R) is None
    with pytest.raises(ValueError):
        cs.slusol_factor(A, 0, perturb=-1.0)
