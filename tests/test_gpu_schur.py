"""schur_factor on the device on the cases of tests/schur_cases.py: Lp.p, Lp.i, Lp.x, d, S, the inertia and the
statistics byte-equal to csx_schur_host (which tests/test_schur_cpu.py holds to the Python restatement) for every case, order and
value set; ldlsol_factor's bytes for ns = 0 -- the two stand on one core: the walker's cap stays the entry point's,
the two handle kinds stay apart, Lp.x keeps its unit tail through every refactor, the two info() faces; which launches ran; refactor against a fresh factor, a breaking refactor that
changes nothing, and a refactor after it; condense / expand of lists against the plain-Python restatement and exact blocks
against the lists; rounding-equal blocks through solve(b, interface) held to twice the backward error of the exact route; the
CSX_EINVAL cases of the C ABI."""
import math

import numpy as np
import pytest

import schur_cases as SC
import schur_oracle as SO
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


def _values(sc, which):
    return sc.kept_zero() if which == "kept-zero" else sc.values(which)


def _factor(cs, sc, which="A", exact=None, pin=False):
    A = sc.matrix(cs, _values(sc, which))
    if pin:
        cs.cs_pin(A)
    return cs.schur_factor(A, sc.keep, sc.order, 0.0, exact)


def _S(F, sc):
    return F.schur.numpy().reshape(-1)[:sc.ns * sc.ns].reshape(sc.ns, sc.ns)


def _is_reference(cs, F, sc, which):
    Lfp, Lfi, _ = SO.pattern_of(sc)
    Lpx, d, S, info = SO.reference(sc, which)
    rp, ri = SO.lp_pattern(Lfp, Lfi, sc.n, sc.n1)
    p, i, x = _download(cs, F.factors.L)
    assert p.tolist() == rp and i.tolist() == ri
    assert x.tobytes() == Lpx.tobytes(), which
    assert F.factors.D.numpy().reshape(-1).tobytes() == d.tobytes(), which
    got = _S(F, sc)
    assert got.tobytes() == S.tobytes(), which
    assert got.tobytes() == np.ascontiguousarray(got.T).tobytes()       # both triangles, the same bytes
    g = F.info()
    assert (g["pos"], g["neg"], g["perturbed"], g["breakdown"]) == info, which
    assert F.inertia() == info[:2]
    assert (g["n"], g["n1"], g["ns"], g["lnz"]) == (sc.n, sc.n1, sc.ns, len(ri))
    if sc.n1:
        off = np.ones(len(Lpx), bool)
        off[np.asarray(rp[:-1])] = False
        assert g["min_abs_d"] == np.min(np.abs(d)) and g["max_abs_d"] == np.max(np.abs(d))
        assert g["max_abs_l"] == (np.max(np.abs(Lpx[off])) if off.any() else 0.0)
        s, l = F.logdet()
        assert s == (-1.0 if info[1] % 2 else 1.0) and l == math.fsum(np.log(np.abs(d)).tolist())


def _condensed(F, b):
    g, state = F.condense(list(b))
    return np.asarray(g).tobytes() + state.numpy().tobytes()


@pytest.mark.parametrize("name", SC.NAMES)
def test_factor_and_refactor_are_the_host_rule(cs, name):
    sc = SC.BY_NAME[name]
    for which in SC.VALUE_SETS + (("kept-zero",) if sc.ns else ()):      # a zero kept diagonal is data: it factors
        F = _factor(cs, sc, which)
        assert F is not None, which
        assert F.symbolic.pinv == SO.pinv_of(sc) and F.keep == sc.keep
        _is_reference(cs, F, sc, which)
    b = SC.rhs(sc, 1)[0].tolist()
    F = _factor(cs, sc, "A")
    c0 = _condensed(F, b)                                               # the triangular plan of A's factor is cached now
    assert F.refactor(sc.matrix(cs, sc.case.A2[0])) is True
    _is_reference(cs, F, sc, 0)
    fresh = _factor(cs, sc, 0)
    c1 = _condensed(F, b)
    assert c1 == _condensed(fresh, b)                                   # ... and must not outlive the refactor
    if sc.n1 and sc.n > 2:
        assert c1 != c0
    assert F.refactor(sc.case.A2[1]) is True
    _is_reference(cs, F, sc, 1)
    c2 = _condensed(F, b)
    assert c2 == _condensed(_factor(cs, sc, 1), b)
    if sc.n1:
        # a breaking refactor: False, and Lp.x, d, S and the next condense's bytes are what they were
        bad = sc.case.breaking(SO.first_column(sc))
        assert F.refactor(bad) is False
        assert F.info()["breakdown"] == 0
        Lpx, d, S, info = SO.reference(sc, 1)
        assert _download(cs, F.factors.L)[2].tobytes() == Lpx.tobytes()
        assert F.factors.D.numpy().reshape(-1).tobytes() == d.tobytes() and _S(F, sc).tobytes() == S.tobytes()
        assert F.inertia() == info[:2]
        assert _condensed(F, b) == c2
        # a fresh factor of the breaking values: None
        assert cs.schur_factor(sc.matrix(cs, bad), sc.keep, sc.order) is None
    # ... and the factor still takes new values
    assert F.refactor(cs.dvec(sc.case.A2[0])) is True
    _is_reference(cs, F, sc, 0)


def test_nothing_kept_is_ldlsol_factor(cs):
    for name in ("one-keep-none", "grid-line-1"):
        sc = SC.BY_NAME[name]
        A = sc.matrix(cs)
        F, G = cs.schur_factor(A, [], 1), cs.ldlsol_factor(A, 1)
        a, b = _download(cs, F.factors.L), _download(cs, G.factors.L)
        assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
        assert F.factors.D.numpy().tobytes() == G.factors.D.numpy().tobytes()
        assert F.inertia() == G.inertia() and F.logdet() == G.logdet() and F.symbolic.pinv == G.symbolic.pinv
        f, g = F.info(), G.info()
        assert (f["ns"], f["schur_launches"], f["schur_chunks"]) == (0, 0, 0)
        assert all(f[k] == g[k] for k in ("n", "lnz", "levels", "level_launches", "pos", "neg", "min_abs_d", "max_abs_d", "max_abs_l"))


def test_everything_kept_is_the_matrix(cs):
    sc = SC.BY_NAME["one-keep-all"]
    F = _factor(cs, sc)
    assert _S(F, sc).tolist() == [[-3.0]] and F.inertia() == (0, 0) and F.logdet() == (1.0, 0.0)
    i = F.info()
    assert (i["n1"], i["ns"], i["levels"], i["level_launches"], i["run_launches"], i["schur_launches"], i["schur_chunks"]) == \
        (0, 1, 0, 0, 0, 1, 1)
    x = [6.0]
    assert F.solve(x, lambda g: g / -3.0) is True and x == [-2.0]


def test_which_launches_ran(cs):
    i = _factor(cs, SC.BY_NAME["chain600"]).info()
    assert (i["levels"], i["level_launches"], i["run_launches"]) == (598, 0, 3) and -(-598 // 256) == 3      # the walker, cut at 256 levels
    assert (i["schur_launches"], i["schur_chunks"], i["launches"]) == (1, 2, 4)
    for name in SC.BORDERS:
        sc = SC.BY_NAME[name]
        i = _factor(cs, sc).info()
        assert i["window"] == SC.WINDOW
        assert i["schur_chunks"] == SC.BORDER_CHUNKS[name] == sc.chunks(), name
        assert i["schur_launches"] == 1 and i["kernel_us"] > 0
        assert i["long_columns"] == (3 if sc.ns + 3 > SC.WINDOW else 0)   # an interior column reaches every kept row
    sc = SC.BY_NAME["grid-cross-1"]
    i = _factor(cs, sc).info()
    assert i["schur_chunks"] == sc.ns and i["level_launches"] >= 1 and i["long_columns"] == 0


def test_the_walker_cap_is_the_entry_points(cs):
    """257 levels of one column: ldlsol_factor's walker takes them in one launch, schur_factor's is cut at 256 -- with nothing kept
    too.  257 is the smallest size at which one cap for both would show."""
    import ldl_cases as LC
    A = LC.BY_NAME["chain"].matrix(cs)
    G, F = cs.ldlsol_factor(A, 0), cs.schur_factor(A, [], 0)
    g, f = G.info(), F.info()
    assert (g["levels"], g["run_launches"], g["level_launches"]) == (257, 1, 0)
    assert (f["levels"], f["run_launches"], f["level_launches"]) == (257, 2, 0)
    assert _download(cs, F.factors.L)[2].tobytes() == _download(cs, G.factors.L)[2].tobytes()
    assert F.factors.D.numpy().tobytes() == G.factors.D.numpy().tobytes()


def test_handle_kinds_stay_apart(cs):
    """an ldl handle is no schur handle and the reverse: CSX_EINVAL from info, parts, stats and refactor, `ok` of a refactor untouched"""
    import _csx
    lib, C = _csx.lib(), _csx.C
    sc = SC.BY_NAME["grid-line-0"]
    A = cs.cs_pin(sc.matrix(cs))
    S = cs.schur_factor(A, sc.keep, 0).symbolic
    parent, cp, pinv = (_csx.pi(_csx.i32(v)) for v in (S.parent, S.cp, S.pinv))
    hl, hs, ok = _csx.new_handle(), _csx.new_handle(), C.c_int(0)
    try:
        assert lib.csx_ldl_factor(A._dev.handle, parent, cp, pinv, 0.0, hl, ok) == _csx.OK and ok.value == 1
        assert lib.csx_schur_factor(A._dev.handle, parent, cp, pinv, sc.n1, 0.0, hs, ok) == _csx.OK and ok.value == 1
        raw, st = (C.c_int64 * 32)(), np.zeros(3)
        a, b, c = _csx.new_handle(), _csx.new_handle(), _csx.new_handle()
        assert lib.csx_ldl_info(hl, raw) == _csx.OK and lib.csx_schur_info(hs, raw) == _csx.OK
        assert lib.csx_schur_info(hl, raw) == _csx.EINVAL and lib.csx_ldl_info(hs, raw) == _csx.EINVAL
        assert lib.csx_schur_parts(hl, a, b, c) == _csx.EINVAL and lib.csx_ldl_parts(hs, a, b) == _csx.EINVAL
        assert lib.csx_schur_stats(hl, _csx.pd(st)) == _csx.EINVAL and lib.csx_ldl_stats(hs, _csx.pd(st)) == _csx.EINVAL
        for fn, h in ((lib.csx_schur_refactor, hl), (lib.csx_ldl_refactor, hs)):
            ok.value = 7
            assert fn(h, A._dev.handle, 0.0, ok) == _csx.EINVAL and ok.value == 7
    finally:
        _csx.free(hl)
        _csx.free(hs)


@pytest.mark.parametrize("name", ["one-keep-all", "grid-line-0"])
def test_the_unit_tail_survives_every_path(cs, name):
    """the last ns values of Lp.x are 1.0 and Lp.x is the host rule's of the values last committed: after a refactor, a breaking
    refactor and a refactor again.  one-keep-all: n1 = 0, Lp.x is the tail alone."""
    sc = SC.BY_NAME[name]
    F = _factor(cs, sc, "A")

    def is_committed(which):
        x = _download(cs, F.factors.L)[2]
        assert x[len(x) - sc.ns:].tolist() == [1.0] * sc.ns
        assert x.tobytes() == SO.reference(sc, which)[0].tobytes()

    is_committed("A")
    assert F.refactor(sc.case.A2[0]) is True
    is_committed(0)
    if sc.n1:
        assert F.refactor(sc.case.breaking(SO.first_column(sc))) is False
        is_committed(0)
    else:
        assert F.refactor(sc.kept_zero()) is True        # no interior column, nothing can break: a zero kept diagonal is data
        is_committed("kept-zero")
        assert _S(F, sc).tolist() == [[0.0]]
    assert F.refactor(sc.matrix(cs, sc.case.A2[1])) is True
    is_committed(1)


def test_info_faces(cs):
    sc = SC.BY_NAME["kkt-sqd"]
    A = sc.matrix(cs)
    F, G = cs.schur_factor(A, [], 1), cs.ldlsol_factor(A, 1)
    stats = ["min_abs_d", "max_abs_d", "max_abs_l"]
    assert list(G.info()) == ["n", "lnz", "levels", "launches", "pos", "neg", "perturbed", "breakdown", "kernel_us", "level_launches",
                              "run_launches", "long_columns", "window"] + stats
    assert list(F.info()) == ["n", "n1", "ns", "lnz", "levels", "launches", "level_launches", "run_launches", "schur_launches",
                              "schur_chunks", "pos", "neg", "perturbed", "breakdown", "kernel_us", "long_columns", "window"] + stats
    assert F.inertia() == G.inertia() and F.logdet() == G.logdet()
    assert sum(F.inertia()) == sc.n


def _lists(sc, F, cols, x2):
    """(g, state, x) of every column by the list calls, and the plain-Python restatement's bytes held against them"""
    Lfp, Lfi, _ = SO.pattern_of(sc)
    Lpx, d, _, _ = SO.reference(sc, "A")
    p, i = SO.lp_pattern(Lfp, Lfi, sc.n, sc.n1)
    pinv, lx, ld = SO.pinv_of(sc), Lpx.tolist(), d.tolist()
    out = []
    for c in range(len(cols)):
        b = cols[c].tolist()
        g, state = F.condense(b)
        assert b == cols[c].tolist() and isinstance(g, list) and (state.n, state.k) == (sc.n, 1)
        x = F.expand(state, x2[:, c].tolist())
        assert isinstance(x, list)
        st = state.numpy().reshape(-1)
        if c < 3:
            ref = SO.condense_list(sc.n, sc.n1, pinv, p, i, lx, ld, b)
            assert st.tobytes() == np.asarray(ref).tobytes() and np.asarray(g).tobytes() == np.asarray(ref[sc.n1:]).tobytes()
            rx = SO.expand_list(sc.n, sc.n1, pinv, p, i, lx, ref, x2[:, c].tolist())
            assert np.asarray(x).tobytes() == np.asarray(rx).tobytes()
        out.append((np.asarray(g), st, np.asarray(x)))
    return out


@pytest.mark.parametrize("name", ["grid-line-1", "kkt-sqd", "grid-cross-0"])
def test_lists_and_exact_blocks(cs, name):
    sc = SC.BY_NAME[name]
    n, ns = sc.n, sc.ns
    F, FX = _factor(cs, sc, pin=True), _factor(cs, sc, exact=True, pin=True)
    cols, x2 = SC.rhs(sc, max(BLOCKS)), SC.x2(sc, max(BLOCKS))
    lists = _lists(sc, F, cols, x2)
    for k in BLOCKS:
        B = np.ascontiguousarray(cols[:k].T)
        dB = cs.dvec(B)
        g, state = FX.condense(dB)
        assert dB.numpy().tobytes() == B.tobytes()                      # b is not modified
        assert isinstance(g, cs.dvec) and (g.n, g.k, state.n, state.k) == (ns, k, n, k)
        Gm, St = g.numpy().reshape(ns, k), state.numpy().reshape(n, k)
        X2 = np.ascontiguousarray(x2[:, :k])
        for form in (X2, cs.dvec(X2)):
            X = FX.expand(state, form).numpy().reshape(n, k)
            for c in range(k):
                assert X[:, c].tobytes() == lists[c][2].tobytes(), (k, c)
        assert state.numpy().reshape(n, k).tobytes() == St.tobytes()    # expand works on a copy of state
        for c in range(k):
            assert Gm[:, c].tobytes() == lists[c][0].tobytes() and St[:, c].tobytes() == lists[c][1].tobytes(), (k, c)


def _omegas(cs, F, sc, A, B, S):
    """per column omega of solve(b, interface = numpy's solve on S) by residual_block(sym=True)"""
    dX = cs.dvec(B)
    assert F.solve(dX, lambda g: np.linalg.solve(S, g)) is True
    _, omega, _ = cs.residual_block(A, dX, cs.dvec(B), residual=False, sym=True)
    return omega


@pytest.mark.parametrize("name", ["kkt-sqd", "kkt-zero", "grid-line-1"])
def test_rounding_equal_blocks_through_solve(cs, name):
    """omega of every column of a block solved in the rounding-equal order <= 2 omega of the same column by the exact route, floor
    2 eps: the factor and S are the same bytes, the factor 2 covers the reassociated sums of the two sweeps alone.
    Observed on an MI355X: see DESIGN.md §25."""
    sc = SC.BY_NAME[name]
    A = cs.cs_pin(sc.matrix(cs))
    F, FX = _factor(cs, sc, pin=True), _factor(cs, sc, exact=True, pin=True)
    S = _S(F, sc).copy()
    assert S.tobytes() == _S(FX, sc).tobytes()
    for k in (1, 3, 65):
        B = np.ascontiguousarray(SC.rhs(sc, k).T)
        w, wx = _omegas(cs, F, sc, A, B, S), _omegas(cs, FX, sc, A, B, S)
        print("schur solve omega / eps", name, k, "block", w.min() / EPS, w.max() / EPS, "exact", wx.min() / EPS, wx.max() / EPS)
        assert w.shape == (k,) and (w <= np.maximum(2.0 * wx, 2.0 * EPS)).all()
    b = SC.rhs(sc, 1)[0].tolist()
    x = list(b)
    assert F.solve(x, lambda g: np.linalg.solve(S, g)) is True and x != b


def test_bad_arguments(cs):
    import _csx
    lib, C = _csx.lib(), _csx.C
    sc = SC.BY_NAME["grid-line-0"]
    case = sc.case
    A = cs.cs_pin(sc.matrix(cs))
    F = cs.schur_factor(A, sc.keep, 0)
    S = F.symbolic
    parent, cp, pinv = _csx.i32(S.parent), _csx.i32(S.cp), _csx.i32(S.pinv)

    def factor(h, parent=parent, cp=cp, pinv=pinv, n1=sc.n1, tau=0.0):
        out, ok = _csx.new_handle(), C.c_int(0)
        st = lib.csx_schur_factor(h, _csx.pi(parent), _csx.pi(cp), _csx.pi(pinv), n1, tau, out, ok)
        if st == _csx.OK:
            assert ok.value == 1
            _csx.free(out)
        return st

    assert factor(A._dev.handle) == _csx.OK
    assert factor(A._dev.handle, tau=-1.0) == _csx.EINVAL and factor(A._dev.handle, tau=float("nan")) == _csx.EINVAL
    assert factor(A._dev.handle, n1=-1) == _csx.EINVAL and factor(A._dev.handle, n1=sc.n + 1) == _csx.EINVAL
    P = cs.cs_spalloc(case.n, case.n, len(case.i), False, False)          # pattern only
    P.p, P.i, P.x = case.p.tolist(), case.i.tolist(), None
    assert factor(cs.cs_pin(P)._dev.handle) == _csx.EINVAL
    R = cs.cs_spalloc(case.n + 1, case.n, len(case.i), True, False)        # not square
    R.p, R.i, R.x = case.p.tolist(), case.i.tolist(), case.x.tolist()
    assert factor(cs.cs_pin(R)._dev.handle) == _csx.EINVAL
    wrong = cp.copy()                                                      # an S_sym that is not A's: the counts, then the tree
    wrong[1:] += 1
    assert factor(A._dev.handle, cp=wrong) == _csx.EINVAL
    assert factor(A._dev.handle, parent=np.full(case.n, -1, np.int32)) == _csx.EINVAL
    assert factor(A._dev.handle, pinv=None) == _csx.EINVAL                 # a pinv that is not the analysis's
    # ns ns >= 2^31: refused before anything is built
    n = 46341
    D = cs.cs_spalloc(n, n, n, True, False)
    D.p, D.i, D.x = list(range(n + 1)), list(range(n)), [1.0] * n
    big = _csx.i32(np.arange(n + 1))
    assert factor(cs.cs_pin(D)._dev.handle, parent=np.full(n, -1, np.int32), cp=big, pinv=None, n1=0) == _csx.EINVAL
    # refactor: another pattern with the same shape and entry count, a short vector
    i2 = case.i.copy()
    first_off = int(np.flatnonzero(case.i != case.cols)[0])
    i2[first_off] = 0 if i2[first_off] != 0 else 1
    B = cs.cs_spalloc(case.n, case.n, len(case.i), True, False)
    B.p, B.i, B.x = case.p.tolist(), i2.tolist(), case.x.tolist()
    before = _download(cs, F.factors.L)[2].tobytes() + F.schur.numpy().tobytes()
    with pytest.raises(ValueError):
        F.refactor(B)
    with pytest.raises(ValueError):
        F.refactor(case.x[:-1])
    assert _download(cs, F.factors.L)[2].tobytes() + F.schur.numpy().tobytes() == before
    g, state = F.condense(SC.rhs(sc, 1)[0].tolist())
    with pytest.raises(ValueError):
        F.expand(state, [0.0] * (sc.ns + 1))
    # the Python face
    T = cs.cs_spalloc(3, 3, 1, True, True)
    assert cs.schur_factor(T, [0]) is None and cs.schur_factor(R, [0]) is None
    with pytest.raises(ValueError):
        cs.schur_factor(A, [0, 0])
    with pytest.raises(ValueError):
        cs.schur_factor(A, [case.n])
    with pytest.raises(ValueError):
        cs.schur_factor(A, [0], perturb=-1.0)
