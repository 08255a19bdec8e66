"""sparseinv and cholsol_factor(...).inverse / .inverse_diag / .logdet on the device: Z.x byte-equal to the
pure-Python restatement of the Takahashi recurrence (tests/sparseinv_oracle.py) run on exactly the factor the device holds, and
within tol.cross_bound(cond_1(A)) of numpy.linalg.inv -- the bound tests/test_sparseinv_cpu.py holds the restatement to.
On the large forests the trees are independent: the restatement runs on a seeded sample of whole trees (200 of them, always
the first, the last and the largest) and those trees' bytes are compared."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import sparseinv_oracle as SI
import synth
import tol as TOL
from conftest import golden, unpack
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

SAMPLE = 200


def _dev_cs(cs, n, p, i, x, m=None):
    import _csx
    p, i = np.asarray(p, np.int32), np.asarray(i, np.int32)
    x = None if x is None else np.asarray(x, np.float64)
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(m or n, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), h), "csx_csc_upload")
    return cs._from_device(h, lambda nnz: max(nnz, 1))


def _arrays(M):
    """(p, i, x) of a device-backed matrix as numpy arrays, without materialising it"""
    import _csx
    m, n, nnz, hv = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return p, i[:nnz], x[:nnz]


def _sp(p, i, x):
    n = len(p) - 1
    A = sp.csc_matrix((np.asarray(x, float), np.asarray(i), np.asarray(p)), shape=(n, n))
    A.sort_indices()
    return A


def _grid(gx, gy):
    Tx = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gx, gx))
    Ty = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gy, gy))
    A = (sp.kron(sp.identity(gy), Tx) + sp.kron(Ty, sp.identity(gx)) + 0.5 * sp.identity(gx * gy)).tocsc()
    A.sort_indices()
    return A


def _oracle_bytes(p, i, x):
    n = len(p) - 1
    return np.asarray(SI.sparseinv_x(n, p.tolist(), i.tolist(), x.tolist())).tobytes()


def _factor(cs, Asp, order):
    """the device factor of cs_chol at this order: (L, pinv or None)"""
    n = Asp.shape[0]
    A = _dev_cs(cs, n, Asp.indptr, Asp.indices, Asp.data)
    cs.cs_pin(A)
    S = cs.cs_schol(order, A)
    N = cs.cs_chol(A, S)
    assert N is not None
    return N.L, (None if S.pinv is None else np.asarray(S.pinv, np.int64))


def _against_dense(Asp, p, i, zx, pinv=None):
    """componentwise error of Z's stored entries against inv(A) (through pinv), and the bound"""
    n = Asp.shape[0]
    Ad = Asp.toarray()
    if pinv is not None:
        perm = np.empty(n, np.int64)
        perm[pinv] = np.arange(n)
        Ad = Ad[np.ix_(perm, perm)]
    ref = np.linalg.inv(Ad)
    cols = np.repeat(np.arange(n), np.diff(p))
    return TOL.componentwise(zx, ref[i, cols]), TOL.cross_bound(TOL.cond1(Asp))


def _bcsstk(cs, name):
    A = unpack(cs, golden(name), "C")
    nz = A.p[A.n]
    return _sp(A.p, A.i[:nz], A.x[:nz])


@pytest.mark.parametrize("name,order", [("bcsstk01", 0), ("bcsstk01", 1), ("bcsstk16", 0), ("bcsstk16", 1)])
def test_bytes_of_the_loop_on_bcsstk(cs, name, order):
    """bcsstk16 at order 0 is nearly a chain: thousands of depths, most of them walked inside one launch; with
    "sparseinv.walk" = 0 every depth is a launch of its own and the bytes are the same"""
    import _csx
    Asp = _bcsstk(cs, name)
    L, pinv = _factor(cs, Asp, order)
    p, i, x = _arrays(L)
    Z = cs.sparseinv(L)
    info = cs.sparseinv_info()
    zp, zi, zx = _arrays(Z)
    assert Z is not L and np.array_equal(zp, p) and np.array_equal(zi, i)
    assert _arrays(L)[2].tobytes() == x.tobytes()                  # L is not changed
    m = np.diff(p).astype(np.int64) - 1
    assert info["n"] == len(p) - 1 and info["terms"] == int(np.sum(m * m)) and info["depths"] >= int(m.max()) + 1
    print(name, order, info)
    if name == "bcsstk16" and order == 0:
        assert info["depths"] > 4000
    want = _oracle_bytes(p, i, x)
    assert zx.tobytes() == want
    with _csx.option("sparseinv.walk", 0):
        assert _arrays(cs.sparseinv(L))[2].tobytes() == want
    if name == "bcsstk01" or order == 1:
        err, bound = _against_dense(Asp, p, i, zx, pinv)
        print(name, order, "componentwise", err, "bound", bound)
        assert err <= bound


def _sample(starts, seed):
    """SAMPLE trees of a forest given the first column of every tree (+ n): the first, the last, the largest, the rest drawn"""
    nt = len(starts) - 1
    sizes = np.diff(starts)
    pick = {0, nt - 1, int(np.argmax(sizes))}
    rng = np.random.default_rng(seed)
    while len(pick) < min(SAMPLE, nt):
        pick.add(int(rng.integers(0, nt)))
    return sorted(pick)


def _tree_factor(p, i, x, c0, c1):
    """columns [c0, c1) of a block-diagonal factor as a factor of their own: (p, i, x) lists, rows renumbered"""
    b, e = int(p[c0]), int(p[c1])
    rows = i[b:e].astype(np.int64) - c0
    assert rows.min() >= 0 and rows.max() < c1 - c0            # the tree is closed: nothing of it lies outside the block
    return (p[c0:c1 + 1].astype(np.int64) - b).tolist(), rows.tolist(), x[b:e].tolist()


def _compare_sampled(p, i, x, zx, starts, seed):
    picked = _sample(starts, seed)
    for t in picked:
        c0, c1 = int(starts[t]), int(starts[t + 1])
        tp, ti, tx = _tree_factor(p, i, x, c0, c1)
        want = np.asarray(SI.sparseinv_x(c1 - c0, tp, ti, tx))
        assert zx[p[c0]:p[c1]].tobytes() == want.tobytes(), "tree %d (columns %d..%d)" % (t, c0, c1)
    return picked


def _arrow_trees(nb, bs, seed):
    """nb blocks of bs columns, tridiagonal plus a full last row / column: small elimination trees that are no cliques
    (the matrix of test_gpu_fullsize.py's forest of small sparse trees)"""
    cols = []
    for c in range(bs):
        rows = {c, bs - 1} | ({c - 1} if c > 0 else set()) | ({c + 1} if c + 1 < bs else set())
        cols.append(sorted(range(bs)) if c == bs - 1 else sorted(rows))
    bi = np.concatenate([np.asarray(r, np.int64) for r in cols])
    bp = np.concatenate([[0], np.cumsum([len(r) for r in cols])])
    rng = np.random.default_rng(seed)
    Ap = np.concatenate([(np.arange(nb)[:, None] * bp[-1] + bp[None, :-1]).reshape(-1), [nb * bp[-1]]]).astype(np.int32)
    Ai = (bi[None, :] + (np.arange(nb) * bs)[:, None]).reshape(-1).astype(np.int32)
    colof = np.repeat(np.arange(bs), np.diff(bp))
    lo, hi = np.minimum(bi, colof), np.maximum(bi, colof)
    U = rng.uniform(0.5, 1.0, size=(nb, bs))
    Ax = np.where(lo[None, :] == hi[None, :], 8.0 + U[:, lo], -U[:, lo] * U[:, hi] / (1.0 + (hi - lo)[None, :])).reshape(-1)
    return Ap, Ai, Ax


def _forest(kind):
    """(Ap, Ai, Ax, first column of every tree + [n])"""
    if kind == "gspd64":
        p, i, x = synth.gspd(2031, 64, 7)
        return p, i, x, np.arange(2032) * 64
    if kind == "gspd16":
        p, i, x = synth.gspd(8125, 16, 8)
        return p, i, x, np.arange(8126) * 16
    if kind == "ragged":
        n, p, i, x, sizes = synth.ragged_cliques(130000, 8, 64, 9)
        return p, i, x, np.concatenate([[0], np.cumsum(sizes)])
    p, i, x = _arrow_trees(200000, 24, 5)
    return p, i, x, np.arange(200001) * 24


@pytest.mark.parametrize("kind", ["gspd64", "gspd16", "ragged", "trees24"])
def test_bytes_of_the_loop_on_forests(cs, kind):
    Ap, Ai, Ax, starts = _forest(kind)
    n = len(Ap) - 1
    A = _dev_cs(cs, n, Ap, Ai, Ax)
    cs.cs_pin(A)
    L = cs.cs_chol(A, cs.cs_schol(0, A)).L
    p, i, x = _arrays(L)
    Z = cs.sparseinv(L)
    info = cs.sparseinv_info()
    zp, zi, zx = _arrays(Z)
    assert np.array_equal(zp, p) and np.array_equal(zi, i)
    assert info["depths"] == int(np.max(np.diff(starts))) and info["widest"] == len(starts) - 1
    picked = _compare_sampled(p, i, x, zx, starts, 11)
    print(kind, info, "trees compared byte for byte: %d of %d" % (len(picked), len(starts) - 1))
    assert len(picked) == SAMPLE
    # the sampled blocks against their dense inverses
    Asp = _sp(Ap, Ai, Ax)
    worst = 0.0
    for t in picked[:20] + picked[-2:]:
        c0, c1 = int(starts[t]), int(starts[t + 1])
        B = Asp[c0:c1, c0:c1].tocsc()
        tp, ti, _ = _tree_factor(p, i, x, c0, c1)
        err, bound = _against_dense(B, np.asarray(tp), np.asarray(ti), zx[p[c0]:p[c1]])
        worst = max(worst, err / bound)
        assert err <= bound
    print(kind, "worst error / bound over the sampled blocks: %.3g" % worst)


def test_dense_block_of_600_columns_more_than_one_chunk_per_row(cs):
    """columns with up to 599 rows below the diagonal: k_si_wide's rows take their products through LDS in more than one
    chunk of 512; bytes of the restatement, and the dense inverse within the bound"""
    n = 600
    rng = np.random.default_rng(8)
    R = rng.uniform(-1.0, 1.0, (n, n))
    Asp = sp.csc_matrix(R @ R.T / n + 2.0 * np.eye(n))
    Asp.sort_indices()
    L, _ = _factor(cs, Asp, 0)
    p, i, x = _arrays(L)
    assert int(np.max(np.diff(p))) - 1 == n - 1
    Z = cs.sparseinv(L)
    info = cs.sparseinv_info()
    zx = _arrays(Z)[2]
    assert info["depths"] == n and info["widest"] == 1
    assert zx.tobytes() == _oracle_bytes(p, i, x)
    err, bound = _against_dense(Asp, p, i, zx)
    print("dense 600", info, "componentwise", err, "bound", bound)
    assert err <= bound


def test_tridiagonal_of_200000_rows_one_column_per_depth(cs):
    n = 200000
    rng = np.random.default_rng(4)
    d = rng.uniform(2.5, 3.5, n)
    o = rng.uniform(-1.0, 1.0, n - 1)
    Asp = sp.diags([o, d, o], [-1, 0, 1], shape=(n, n)).tocsc()
    Asp.sort_indices()
    L, _ = _factor(cs, Asp, 0)
    p, i, x = _arrays(L)
    Z = cs.sparseinv(L)
    info = cs.sparseinv_info()
    assert info["depths"] == n and info["widest"] == 1 and info["terms"] == n - 1
    assert _arrays(Z)[2].tobytes() == _oracle_bytes(p, i, x)
    print("tridiagonal", info)


@pytest.mark.parametrize("which,order", [("bcsstk01", 0), ("bcsstk01", 1), ("grid", 0), ("grid", 1), ("gspd", 0)])
def test_solver_inverse_diag_and_logdet(cs, which, order):
    if which == "bcsstk01":
        Asp = _bcsstk(cs, which)
    elif which == "grid":
        Asp = _grid(40, 37)
    else:
        Asp = _sp(*synth.gspd(200, 64, 11))
    n = Asp.shape[0]
    A = _dev_cs(cs, n, Asp.indptr, Asp.indices, Asp.data)
    cs.cs_pin(A)
    F = cs.cholsol_factor(A, order=order)
    ref = np.linalg.inv(Asp.toarray())
    bound = TOL.cross_bound(TOL.cond1(Asp))
    dg = F.inverse_diag()
    assert isinstance(dg, np.ndarray) and dg.shape == (n,)
    err = TOL.componentwise(dg, np.diag(ref))
    print(which, order, "inverse_diag componentwise", err, "bound", bound)
    assert err <= bound
    Z = F.inverse()
    p, i, zx = _arrays(Z)
    Lp, Li, Lx = _arrays(F.L)
    assert np.array_equal(p, Lp) and np.array_equal(i, Li)
    pinv = None if order == 0 else np.asarray(F.symbolic.pinv, np.int64)
    assert (pinv is None) == (order == 0)
    err, _ = _against_dense(Asp, p, i, zx, pinv)
    assert err <= bound
    d = zx[p[:-1]]
    assert dg.tobytes() == (d if pinv is None else d[pinv]).tobytes()    # entry i of inverse_diag is Z(pinv[i], pinv[i])
    sign, ld = np.linalg.slogdet(Asp.toarray())
    got = F.logdet()
    print(which, order, "logdet", got, ld)
    assert sign == 1.0 and isinstance(got, float) and abs(got - ld) <= 1e-12 * abs(ld)
    assert got == 2.0 * math.fsum(np.log(Lx[Lp[:-1]]).tolist())
    b = synth.rhs(n, 1, 0)[:, 0].tolist()
    assert F.solve(b)                                              # the solver is as usable as before


def _columns(p, i, fs, seed, scale):
    """one column per f in fs: f and up to three rows of L(:, f)'s pattern (so the pattern does not change)"""
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


@pytest.mark.parametrize("which,order", [("gspd", 0), ("grid", 0), ("grid", 1)])
def test_solver_answers_follow_update_and_survive_a_failed_downdate(cs, which, order):
    """After update(C) the answers are those of A + C C': inverse_diag and Z against the dense inverse and against a fresh
    factor, componentwise within cross_bound(cond_1(A + C C')), and logdet.  ONE comparison is normwise instead: the entries of
    Z off the diagonal on the natural-order grid.  Its factor is a band of 40 rows, so Z stores entries that have decayed to
    1e-10 of the largest and below.  The updated factor is a backward-stable factor of A + C C' in the norm (k rank-1 rotations:
    L L' = A + C C' + E, |E| a modest multiple of eps |L| |L'|), not entry by entry, so the inverse it stands for moves by
    inv E inv: small against the largest entries, not against the decayed ones.  Measured: 2.0e-10 componentwise against the
    bound of 1e-10 there, on the device and with the CPU restatements of cs_updown and sparseinv alike (the figure is printed);
    the diagonal of the same Z is at 3e-15 and is held componentwise like everything else.  Normwise within the same bound is
    the measure tests/test_gpu_updown_block.py uses for the solutions after an update.  Z itself is the restatement's on the
    updated factor, byte for byte."""
    Asp = _grid(40, 37) if which == "grid" else _sp(*synth.gspd(200, 64, 11))
    n = Asp.shape[0]
    A = _dev_cs(cs, n, Asp.indptr, Asp.indices, Asp.data)
    cs.cs_pin(A)
    F = cs.cholsol_factor(A, order=order)
    d0, ld0 = F.inverse_diag(), F.logdet()                         # answers exist before the update: nothing of them may stick
    depths0 = cs.sparseinv_info()["depths"]
    p, i, x = _arrays(F.L)
    pinv = None if order == 0 else np.asarray(F.symbolic.pinv, np.int64)
    colsL = _columns(p, i, np.random.default_rng(5).integers(0, n, 24), 6, 0.3)
    if pinv is not None:                                           # C in A's numbering: row r of L is row perm[r] of A
        perm = np.empty(n, np.int64)
        perm[pinv] = np.arange(n)
        cols = [([int(perm[r]) for r in rows], v) for rows, v in colsL]
    else:
        cols = colsL
    assert F.update(_C(cs, n, cols)) is True
    Cs = sp.csc_matrix((np.concatenate([v for _, v in cols]), np.concatenate([r for r, _ in cols]),
                        np.cumsum([0] + [len(r) for r, _ in cols])), shape=(n, len(cols)))
    A2 = (Asp + Cs @ Cs.T).tocsc()
    A2.sort_indices()
    bound = TOL.cross_bound(TOL.cond1(A2))
    ref = np.linalg.inv(A2.toarray())
    d1, ld1 = F.inverse_diag(), F.logdet()
    assert cs.sparseinv_info()["depths"] == depths0                # the pattern's schedule is reused
    assert d1.tobytes() != d0.tobytes() and ld1 != ld0
    err = TOL.componentwise(d1, np.diag(ref))
    print(which, order, "after update: inverse_diag against the dense inverse, componentwise", err, "bound", bound)
    assert err <= bound
    sign, ld = np.linalg.slogdet(A2.toarray())
    assert abs(ld1 - ld) <= 1e-12 * abs(ld)
    Z1 = F.inverse()
    p1, i1, z1 = _arrays(Z1)
    Ad = A2.toarray() if pinv is None else A2.toarray()[np.ix_(perm, perm)]
    decayed = which == "grid" and order == 0                       # see the docstring: the one normwise comparison
    zref = np.linalg.inv(Ad)[i1, np.repeat(np.arange(n), np.diff(p1))]
    print(which, order, "after update: Z against the dense inverse, componentwise", TOL.componentwise(z1, zref),
          "normwise", TOL.normwise(z1, zref), "bound", bound)
    assert (TOL.normwise if decayed else TOL.componentwise)(z1, zref) <= bound
    assert TOL.componentwise(z1[p1[:-1]], zref[p1[:-1]]) <= bound     # its diagonal componentwise in every case
    # a fresh factor of A + C C'
    F2 = cs.cholsol_factor(_dev_cs(cs, n, A2.indptr, A2.indices, A2.data), order=order)
    d2 = F2.inverse_diag()
    assert TOL.componentwise(d1, d2) <= bound
    assert abs(ld1 - F2.logdet()) <= bound * abs(ld)
    if order == 0:                                                 # the same numbering and the same pattern: Z entry by entry
        p2, i2, z2 = _arrays(F2.inverse())
        assert np.array_equal(p1, p2) and np.array_equal(i1, i2)
        same = _arrays(F.L)[2].tobytes() == _arrays(F2.L)[2].tobytes()
        print(which, order, "after update: Z against the fresh factor's, componentwise", TOL.componentwise(z1, z2),
              "normwise", TOL.normwise(z1, z2), "bound", bound)
        assert z1.tobytes() == z2.tobytes() if same else (TOL.normwise if decayed else TOL.componentwise)(z1, z2) <= bound
        print(which, order, "updated L.x byte-equal to the fresh factor's:", same)
    # the restatement on the updated factor, byte for byte
    pu, iu, xu = _arrays(F.L)
    assert z1.tobytes() == _oracle_bytes(pu, iu, xu)
    xs = synth.rhs(n, 1, 0)[:, 0].copy()
    sol = xs.tolist()
    assert F.solve(sol)
    assert float(np.max(np.abs(A2 @ np.asarray(sol) - xs))) <= bound * float(np.max(np.abs(xs)))
    # a downdate that is not positive definite: False, and the three answers are exactly as before
    f = int(np.argmax(np.diff(pu) > 1))
    fa = f if pinv is None else int(perm[f])
    big = ([fa], [2.0 * float(np.sqrt(A2[fa, fa]))])
    assert F.downdate(_C(cs, n, [big])) is False
    assert F.inverse_diag().tobytes() == d1.tobytes() and F.logdet() == ld1
    assert _arrays(F.inverse())[2].tobytes() == z1.tobytes()


def test_bad_input_raises_and_the_next_call_is_right(cs):
    g = golden("updown")
    p, i, x = (np.asarray(g["bcsstk01_L_" + k]) for k in "pix")
    n = len(p) - 1
    want = _oracle_bytes(p, i, x)

    def good():
        assert _arrays(cs.sparseinv(_dev_cs(cs, n, p, i, x)))[2].tobytes() == want

    def bad(L):
        with pytest.raises(ValueError) as e:
            cs.sparseinv(L)
        assert "csx_chol_inverse" in str(e.value)
        good()

    good()
    R = cs.cs_spalloc(3, 2, 2, True, False)                        # rectangular
    R.p, R.i, R.x = [0, 1, 2], [0, 1], [1.0, 1.0]
    bad(R)
    bad(_dev_cs(cs, n, p, i, None))                                # pattern only
    Pl = cs.cs_spalloc(n, n, len(i), False, False)
    Pl.p, Pl.i, Pl.x = p.tolist(), i.tolist(), None
    bad(Pl)
    for v in (0.0, -1.0, float("nan"), float("inf")):              # a diagonal that is not positive and finite
        xb = x.copy()
        xb[p[17]] = v
        bad(_dev_cs(cs, n, p, i, xb))
    j = int(np.argmax(np.diff(p) >= 4))                            # rows out of order below the diagonal
    ib = i.copy()
    ib[p[j] + 1], ib[p[j] + 2] = i[p[j] + 2], i[p[j] + 1]
    bad(_dev_cs(cs, n, p, ib, x))
    ib = i.copy()                                                  # a repeated row
    ib[p[j] + 2] = i[p[j] + 1]
    bad(_dev_cs(cs, n, p, ib, x))
    ib = i.copy()                                                  # the diagonal not first
    ib[p[j]], ib[p[j] + 1] = i[p[j] + 1], i[p[j]]
    bad(_dev_cs(cs, n, p, ib, x))
    pe = p.copy()                                                  # an empty column
    pe[n - 1] = pe[n]
    bad(_dev_cs(cs, n, pe, i, x))
    # one entry below the diagonal removed: rows a < b of column j are a pair that column a no longer stores
    a, b = int(i[p[j] + 1]), int(i[p[j] + 2])
    q = int(p[a] + np.nonzero(i[p[a]:p[a + 1]] == b)[0][0])
    pd_ = p.copy()
    pd_[a + 1:] -= 1
    Ld = _dev_cs(cs, n, pd_, np.delete(i, q), np.delete(x, q))
    bad(Ld)
    bad(Ld)                                                        # (its schedule is cached by now: the answer is the same)
    # the solver stays usable after a refused matrix elsewhere
    F = cs.cholsol_factor(unpack(cs, golden("bcsstk01"), "C"))
    z = _arrays(F.inverse())[2]
    bad(R)
    assert _arrays(F.inverse())[2].tobytes() == z.tobytes()
    with pytest.raises(ValueError):
        cs.sparseinv(None)


def test_full_size_gspd_5m_rows(cs):
    """csx_gen_gspd at 5M rows (156 250 dense blocks of 32 columns): 32 depths of 156 250 independent columns; 200 sampled
    blocks byte-equal to the restatement, and 22 of them within the bound of numpy.linalg.inv of the block of A"""
    import _csx
    lib = _csx.lib()
    nb, bs = 156250, 32
    n = nb * bs
    hA = _csx.new_handle()
    _csx.check(lib.csx_gen_gspd(nb, bs, 20240606, hA))
    A = cs._from_device(hA, lambda z: max(z, 1))
    A._pinned = True
    F = cs.cholsol_factor(A, exact=True)
    Z = F.inverse()
    info = cs.sparseinv_info()
    print("gspd 5M", info)
    assert info["depths"] == 32 and info["widest"] == nb and info["terms"] == nb * sum(m * m for m in range(bs))
    p, i, x = _arrays(F.L)
    zp, zi, zx = _arrays(Z)
    assert np.array_equal(zp, p) and np.array_equal(zi, i)
    starts = np.arange(nb + 1, dtype=np.int64) * bs
    picked = _compare_sampled(p, i, x, zx, starts, 13)
    assert len(picked) == SAMPLE
    print("gspd 5M: blocks compared byte for byte: %d of %d" % (len(picked), nb))
    for t in picked[:20] + picked[-2:]:
        c0 = t * bs
        hw = _csx.new_handle()
        _csx.check(lib.csx_csc_col_block(hA, c0, bs, hw))
        bp, bi, bx = _arrays(cs._from_device(hw, lambda z: max(z, 1)))
        B = sp.csc_matrix((bx, bi.astype(np.int64) - c0, bp), shape=(bs, bs))
        tp, ti, _ = _tree_factor(p, i, x, c0, c0 + bs)
        err, bound = _against_dense(B, np.asarray(tp), np.asarray(ti), zx[p[c0]:p[c0 + bs]])
        assert err <= bound
    dg = F.inverse_diag()
    assert dg.tobytes() == zx[p[:-1]].tobytes()
