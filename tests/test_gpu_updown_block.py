"""updown_block and cholsol_factor(...).update / .downdate on the device: L.x byte-equal to the loop of rank-1
cs_updown calls it stands for -- the device's loop, and the oracle's where that is quick -- on bcsstk01 / bcsstk16 factors and
on forests of cliques at 130 000 rows, with failures mid-batch, both all-or-nothing and not; the solver's plans follow the new
values; errors leave L as it was."""
import numpy as np
import pytest

import csparse_oracle as O
import synth
import tol as TOL
import updown_block_oracle as UB
from conftest import golden, unpack
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu


def _dev_cs(cs, n, p, i, x):
    import _csx
    p, i, x = np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64)
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(n, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), h), "csx_csc_upload")
    return cs._from_device(h, lambda nnz: max(nnz, 1))


def _arrays(L):
    """(p, i, x) of a factor as numpy arrays, without materialising a device-backed one"""
    import _csx
    if L._lazy:
        m, n, nnz, hv = L._dev.info()
        p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
        _csx.check(_csx.lib().csx_csc_download(L._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
        return p, i[:nnz], x[:nnz]
    nz = L.p[L.n]
    return np.asarray(L.p, np.int32), np.asarray(L.i[:nz], np.int32), np.asarray(L.x[:nz])


def _xb(L):
    return _arrays(L)[2].tobytes()


def _tree(p, i):
    n = len(p) - 1
    has = np.diff(p) > 1
    par = np.full(n, -1, np.int64)
    par[has] = i[p[:-1][has] + 1]
    return par


def _columns(p, i, fs, seed, scale):
    """one column per f in fs: f and three rows of L(:, f)'s pattern (so the pattern does not change)"""
    rng = np.random.default_rng(seed)
    cols = []
    for f in fs:
        pat = i[p[f]:p[f + 1]]
        rows = [int(f)] + [int(r) for r in rng.choice(pat, size=min(len(pat), 3), replace=False) if r != f]
        cols.append((rows, [float(v) for v in scale * rng.uniform(0.5, 1.0, len(rows)) * rng.choice([-1, 1], len(rows))]))
    return cols


def _C(mod, n, cols):
    C = mod.cs_spalloc(n, len(cols), max(1, sum(len(r) for r, _ in cols)), True, False)
    p, i, x = [0], [], []
    for r, v in cols:
        i += r
        x += v
        p.append(len(i))
    C.p, C.i, C.x = p, i or [0], x or [0.0]
    return C


def _loop(cs, L, sigma, cols, parent):
    """cs_updown (device) column by column until one fails"""
    n = L.n
    for t, (r, v) in enumerate(cols):
        W = cs.cs_spalloc(n, 1, max(1, len(r)), True, False)
        W.p, W.i, W.x = [0, len(r)], list(r) or [0], list(v) or [0.0]
        if not cs.cs_updown(L, sigma[t], W, parent):
            return t
    return len(cols)


def _sigmas(k, seed):
    return [1 if s else -1 for s in np.random.default_rng(seed).integers(0, 4, k) > 0]   # mostly updates, some downdates


def _bcsstk(cs, name):
    """the factor as tests/test_updown.py builds it: the fixture's L for bcsstk01, cs_chol of the matrix for bcsstk16"""
    if name == "bcsstk01":
        g = golden("updown")
        return g["bcsstk01_L_p"], g["bcsstk01_L_i"], g["bcsstk01_L_x"]
    C = unpack(cs, golden(name), "C")
    N = cs.cs_chol(C, cs.cs_schol(0, C))
    return _arrays(N.L)


@pytest.mark.parametrize("name", ["bcsstk01", "bcsstk16"])
@pytest.mark.parametrize("k", [1, 8, 64, 65, 200])
def test_block_is_the_loop_on_bcsstk(cs, name, k):
    p, i, x = _bcsstk(cs, name)
    n = len(p) - 1
    par = _tree(p, i)
    rng = np.random.default_rng(k)
    fs = rng.integers(0, n, k)
    if k >= 64:
        fs[: k // 2] = rng.integers(0, min(n, 8), k // 2)      # long shared paths: many terms on one column
    cols = _columns(p, i, fs, k, 0.002 * float(np.median(x[p[:-1]])))
    sig = _sigmas(k, k)
    La = cs.cs_spalloc(n, n, len(i), True, False)
    La.p, La.i, La.x = p.tolist(), i.tolist(), x.tolist()
    Lb = cs.cs_spalloc(n, n, len(i), True, False)
    Lb.p, Lb.i, Lb.x = p.tolist(), i.tolist(), x.tolist()
    xlist = Lb.x
    want = _loop(cs, La, sig, cols, par.tolist())
    assert cs.updown_block(Lb, sig, _C(cs, n, cols)) == want
    assert Lb.x is xlist                                        # the caller's list, updated in place
    assert np.asarray(Lb.x).tobytes() == np.asarray(La.x).tobytes()
    info = cs.updown_info()
    assert info["columns"] == k and info["applied"] == want and 1 <= info["chunks"] <= (k + 63) // 64
    if name == "bcsstk01" or k <= 8:
        Lo = O.cs_spalloc(n, n, len(i), True, False)
        Lo.p, Lo.i, Lo.x = p.tolist(), i.tolist(), x.tolist()
        assert UB.loop(Lo, sig, _C(O, n, cols), par.tolist(), O) == want
        assert np.asarray(Lo.x).tobytes() == np.asarray(Lb.x).tobytes()


def _forest(kind):
    if kind == "gspd64":
        p, i, x = synth.gspd(2031, 64, 7)
        return len(p) - 1, p, i, x
    if kind == "gspd16":
        p, i, x = synth.gspd(8125, 16, 8)
        return len(p) - 1, p, i, x
    n, p, i, x, _ = synth.ragged_cliques(130000, 8, 64, 9)
    return n, p, i, x


@pytest.mark.parametrize("kind", ["gspd64", "gspd16", "ragged"])
def test_block_is_the_loop_on_forests(cs, kind):
    n, Ap, Ai, Ax = _forest(kind)
    A = _dev_cs(cs, n, Ap, Ai, Ax)
    cs.cs_pin(A)
    S = cs.cs_schol(0, A)
    La, Lb = cs.cs_chol(A, S).L, cs.cs_chol(A, S).L
    p, i, x = _arrays(La)
    rng = np.random.default_rng(3)
    k = 300
    fs = np.concatenate([rng.integers(0, 8, 100),                      # 100 terms in the first block: two chunks of that tree
                         rng.integers(1000, 1400, 60),                 # several to a block
                         rng.integers(0, n, 140)])
    rng.shuffle(fs)
    cols = _columns(p, i, fs, 5, 0.05)
    sig = _sigmas(k, 4)
    assert _loop(cs, La, sig, cols, S.parent) == k
    assert cs.updown_block(Lb, sig, _C(cs, n, cols)) == k
    assert _xb(Lb) == _xb(La)
    info = cs.updown_info()
    assert info["chunks"] == 2 and info["groups"] > 100


@pytest.mark.parametrize("aon", [False, True])
def test_failing_downdate_mid_batch(cs, aon):
    p, i, x = _bcsstk(cs, "bcsstk16")
    n = len(p) - 1
    par = _tree(p, i)
    k, bad = 90, 70
    fs = np.random.default_rng(1).integers(0, n, k)
    cols = _columns(p, i, fs, 2, 0.01 * float(np.median(x[p[:-1]])))
    f = int(fs[bad])
    r = int(par[f])
    cols[bad] = ([r, f], [3.0 * x[p[r]], 0.3 * x[p[f]]]) if r >= 0 else ([f], [2.0 * x[p[f]]])
    sig = _sigmas(k, 6)
    sig[bad] = -1
    La = _dev_cs(cs, n, p, i, x)
    Lb = _dev_cs(cs, n, p, i, x)
    assert _loop(cs, La, sig, cols, par.tolist()) == bad
    C = _C(cs, n, cols)
    if not aon:
        assert cs.updown_block(Lb, sig, C) == bad
        assert _xb(Lb) == _xb(La)
    else:
        # through the solver: all or nothing -- False, and L.x as it was
        A = unpack(cs, golden("bcsstk16"), "C")
        F = cs.cholsol_factor(A, exact=True)
        x0 = _xb(F.L)
        b = golden("bcsstk16")["b"]
        s0 = b.tolist()
        assert F.solve(s0)
        assert F.downdate(C) is False                       # column `bad` fails, 70 columns in
        assert _xb(F.L) == x0
        s1 = b.tolist()
        assert F.solve(s1)
        assert np.asarray(s1).tobytes() == np.asarray(s0).tobytes()


def _grid(gx, gy):
    import scipy.sparse as sp
    Tx = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gx, gx))
    Ty = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gy, gy))
    A = (sp.kron(sp.identity(gy), Tx) + sp.kron(Ty, sp.identity(gx)) + 0.5 * sp.identity(gx * gy)).tocsc()
    A.sort_indices()
    return A


def _solver_case(which):
    import scipy.sparse as sp
    if which == "grid":
        return _grid(40, 37), 1
    p, i, x = synth.gspd(200, 64, 11)
    n = len(p) - 1
    return sp.csc_matrix((x, i, p), shape=(n, n)), 0


@pytest.mark.parametrize("which,exact", [("gspd", None), ("gspd", True), ("grid", None)])
def test_solver_update_and_downdate(cs, which, exact):
    import _csx
    import scipy.sparse as sp
    Asp, order = _solver_case(which)
    n = Asp.shape[0]
    A = _dev_cs(cs, n, Asp.indptr, Asp.indices, Asp.data)
    cs.cs_pin(A)
    F = cs.cholsol_factor(A, order=order, exact=exact)
    b = synth.rhs(n, 1, 0)[:, 0].copy()
    B = synth.rhs(n, 16, 3)
    x0 = b.tolist()
    assert F.solve(x0)                                           # plans exist before the update
    assert F.solve(cs.dvec(B.copy()))
    p, i, x = _arrays(F.L)
    pinv = None if order == 0 else np.asarray(F.symbolic.pinv, np.int64)
    rng = np.random.default_rng(5)
    colsL = _columns(p, i, rng.integers(0, n, 24), 6, 0.3)
    if pinv is not None:                                         # C in A's numbering: row r of L is row perm[r] of A
        perm = np.empty(n, np.int64)
        perm[pinv] = np.arange(n)
        cols = [([int(perm[r]) for r in rows], v) for rows, v in colsL]
    else:
        cols = colsL
    C = _C(cs, n, cols)
    assert F.update(C) is True
    info = F.updown_info()
    assert info["columns"] == 24 and info["applied"] == 24
    p, i, x = _arrays(F.L)
    # the list solve: cs_lsolve + cs_ltsolve on the updated L, bit for bit (permutations are exact)
    xs = b.tolist()
    assert F.solve(xs)
    y = b.copy() if pinv is None else np.empty(n)
    if pinv is not None:
        y[pinv] = b
    yl = y.tolist()
    Lh = cs.cs_spalloc(n, n, len(i), True, False)
    Lh.p, Lh.i, Lh.x = p.tolist(), i.tolist(), x.tolist()
    assert cs.cs_lsolve(Lh, yl) and cs.cs_ltsolve(Lh, yl)
    ref = np.asarray(yl) if pinv is None else np.asarray(yl)[pinv]
    assert np.asarray(xs).tobytes() == ref.tobytes()
    # the block solve: a fresh plan of the updated L, in the order the solver uses for blocks
    dB = cs.dvec(B.copy())
    assert F.solve(dB)
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_cholsol_plan(F.L._dev.handle, None if pinv is None else _csx.pi(_csx.i32(pinv)), h),
               "csx_cholsol_plan")
    try:
        _csx.check(_csx.lib().csx_cholsol_set_order(h, 1 if exact else 0), "csx_cholsol_set_order")
        dB2 = cs.dvec(B.copy())
        _csx.check(_csx.lib().csx_cholsol_solve(h, dB2.handle, dB2.k), "csx_cholsol_solve")
    finally:
        _csx.free(h)
    assert dB.numpy().tobytes() == dB2.numpy().tobytes()
    # against a fresh factor of A + C C'
    Cs = sp.csc_matrix((np.concatenate([v for _, v in cols]), np.concatenate([r for r, _ in cols]),
                        np.cumsum([0] + [len(r) for r, _ in cols])), shape=(n, len(cols)))
    A2 = (Asp + Cs @ Cs.T).tocsc()
    A2.sort_indices()
    F2 = cs.cholsol_factor(_dev_cs(cs, n, A2.indptr, A2.indices, A2.data), order=order)
    xf = b.tolist()
    assert F2.solve(xf)
    assert TOL.normwise(xs, xf) <= TOL.cross_bound(TOL.cond1(A2))
    # downdate: back to the first solution, to rounding
    assert F.downdate(C) is True
    xd = b.tolist()
    assert F.solve(xd)
    assert TOL.normwise(xd, x0) <= TOL.cross_bound(TOL.cond1(A2) * TOL.cond1(Asp.tocsc()))


def test_inputs_and_errors(cs):
    g = golden("updown")
    p, i, x = g["bcsstk01_L_p"], g["bcsstk01_L_i"], g["bcsstk01_L_x"]
    n = len(p) - 1
    par = _tree(p, i)
    cols = _columns(p, i, [0, 5, 5, 20, 40], 1, 0.01 * float(np.median(x[p[:-1]])))

    def L_():
        L = cs.cs_spalloc(n, n, len(i), True, False)
        L.p, L.i, L.x = p.tolist(), i.tolist(), x.tolist()
        return L

    La, Lb = L_(), L_()
    assert cs.updown_block(La, 1, _C(cs, n, cols)) == 5
    assert cs.updown_block(Lb, [1] * 5, _C(cs, n, cols), par.tolist()) == 5
    assert La.x == Lb.x
    Lc = L_()
    wrong = par.copy()
    wrong[3] = n - 1 if par[3] != n - 1 else -1
    with pytest.raises(ValueError):
        cs.updown_block(Lc, 1, _C(cs, n, cols), wrong.tolist())
    assert np.asarray(Lc.x).tobytes() == x.tobytes()
    with pytest.raises(ValueError):
        cs.updown_block(Lc, 2, _C(cs, n, cols))
    with pytest.raises(ValueError):
        cs.updown_block(Lc, [1, -1, 1, 1, 0], _C(cs, n, cols))
    with pytest.raises(ValueError):
        cs.updown_block(Lc, 1, _C(cs, n + 1, cols))
    with pytest.raises(IndexError):
        cs.updown_block(Lc, 1, _C(cs, n, [([0, n + 3], [1.0, 1.0])]))
    assert np.asarray(Lc.x).tobytes() == x.tobytes()
    assert cs.updown_block(Lc, 1, _C(cs, n, [])) == 0
    assert cs.updown_block(Lc, -1, _C(cs, n, [([], []), ([], [])])) == 2
    assert np.asarray(Lc.x).tobytes() == x.tobytes()
    # the solver: a column of C outside L(:, f)'s pattern changes the pattern -> ValueError, nothing changed
    A = unpack(cs, golden("bcsstk01"), "C")
    F = cs.cholsol_factor(A)
    Fp, Fi, Fx = _arrays(F.L)
    f = 0
    out = [r for r in range(n) if r not in set(Fi[Fp[f]:Fp[f + 1]].tolist())]
    assert out
    with pytest.raises(ValueError):
        F.update(_C(cs, n, [([f, out[0]], [1.0, 1.0])]))
    assert _xb(F.L) == Fx.tobytes()
