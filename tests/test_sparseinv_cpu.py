"""sparseinv without a GPU: the pure-Python restatement of the Takahashi recurrence, tests/sparseinv_oracle.py
-- the loop the device kernel is byte-equal to -- against numpy.linalg.inv on the stored positions, within the project's bound
for two different routes to one answer (tol.cross_bound of the 1-norm condition estimate); and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import csparse_oracle as O
import sparseinv_oracle as SI
import synth
import tol as TOL
from conftest import ROOT, golden, unpack


def _oracle_cs(Asp):
    Asp = sp.csc_matrix(Asp)
    Asp.sort_indices()
    n = Asp.shape[0]
    A = O.cs_spalloc(n, n, max(Asp.nnz, 1), True, False)
    A.p, A.i, A.x = Asp.indptr.tolist(), Asp.indices.tolist(), Asp.data.tolist()
    return A


def _factor(Asp, order=0):
    """(L, pinv) of the oracle's cs_chol; order 1: the product's host ordering (the oracle defines the natural order only)"""
    A = _oracle_cs(Asp)
    if order == 0:
        S = O.cs_schol(0, A)
    else:
        import csparse as cs
        Ap = cs.cs_spalloc(A.n, A.n, len(A.i), True, False)
        Ap.p, Ap.i, Ap.x = list(A.p), list(A.i), list(A.x)
        pinv = O.cs_pinv(cs.cs_amd(1, Ap), A.n)
        S = O.cs_schol(0, O.cs_symperm(A, pinv, False))
        S.pinv = pinv
    N = O.cs_chol(A, S)
    assert N is not None
    return N.L, (None if S.pinv is None else np.asarray(S.pinv, np.int64))


def _check(Asp, L, pinv=None):
    """Z = oracle sparseinv(L) against inv(A) at the stored positions (through pinv), and diag(Z A) = 1"""
    Asp = sp.csc_matrix(Asp)
    n = Asp.shape[0]
    Z = SI.sparseinv(L)
    assert Z.p == list(L.p) and Z.i == list(L.i) and Z is not L
    nz = L.p[n]
    p, i = np.asarray(L.p), np.asarray(L.i[:nz])
    zx = np.asarray(Z.x[:nz])
    Ad = Asp.toarray()
    if pinv is not None:                     # L L' = P A P': row r of A is row pinv[r] of L
        perm = np.empty(n, np.int64)
        perm[pinv] = np.arange(n)
        Ad = Ad[np.ix_(perm, perm)]
    ref = np.linalg.inv(Ad)
    cols = np.repeat(np.arange(n), np.diff(p))
    bound = TOL.cross_bound(TOL.cond1(Asp))
    err = TOL.componentwise(zx, ref[i, cols])
    D = SI.dense_symmetric(n, p, i, zx)
    # row j of Z times column j of A: the stored entries suffice where A's pattern lies inside L + L'
    unit = np.einsum("ij,ji->i", D, Ad)
    uerr = float(np.max(np.abs(unit - 1.0)))
    print("n %d lnz %d componentwise %.3g diag(Z A) - 1 %.3g bound %.3g" % (n, nz, err, uerr, bound))
    assert err <= bound
    assert uerr <= bound
    return Z


def _sp(p, i, x):
    n = len(p) - 1
    return sp.csc_matrix((x, i, p), shape=(n, n))


def test_bcsstk01_against_dense_inverse():
    A = unpack(O, golden("bcsstk01"), "C")
    Asp = _sp(np.asarray(A.p), np.asarray(A.i[:A.p[A.n]]), np.asarray(A.x[:A.p[A.n]]))
    L, _ = _factor(Asp)
    Z = _check(Asp, L)
    # log det from the factor's diagonal
    d = np.asarray([L.x[L.p[j]] for j in range(L.n)])
    sign, ld = np.linalg.slogdet(Asp.toarray())
    assert sign == 1.0 and abs(2.0 * float(np.sum(np.log(d))) - ld) <= 1e-12 * abs(ld)
    assert all(Z.x[Z.p[j]] > 0.0 for j in range(Z.n))


@pytest.mark.parametrize("bs", [8, 16, 32])
def test_gspd_blocks(bs):
    Asp = _sp(*synth.gspd(40, bs, 3 + bs))
    L, _ = _factor(Asp)
    _check(Asp, L)


def test_ragged_cliques():
    n, p, i, x, sizes = synth.ragged_cliques(600, 3, 40, 5)
    Asp = _sp(p, i, x)
    L, _ = _factor(Asp)
    _check(Asp, L)


def test_tridiagonal_and_arrow():
    n = 300
    T = sp.diags([-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n)).tocsc()
    L, _ = _factor(T)
    _check(T, L)
    rng = np.random.default_rng(2)
    w = rng.uniform(-1.0, 1.0, n - 1)
    Aw = sp.lil_matrix((n, n))
    Aw.setdiag(rng.uniform(2.0, 3.0, n))
    Aw[n - 1, :n - 1] = w
    Aw[:n - 1, n - 1] = w.reshape(-1, 1)
    Aw[n - 1, n - 1] = 4.0 + float(np.sum(w * w))
    Aw = Aw.tocsc()
    L, _ = _factor(Aw)
    _check(Aw, L)


def test_order_1_through_pinv():
    gx, gy = 14, 11
    Tx = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gx, gx))
    Ty = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gy, gy))
    Asp = (sp.kron(sp.identity(gy), Tx) + sp.kron(Ty, sp.identity(gx)) + 0.5 * sp.identity(gx * gy)).tocsc()
    L, pinv = _factor(Asp, 1)
    assert pinv is not None and not np.array_equal(pinv, np.arange(gx * gy))
    _check(Asp, L, pinv)


def test_sampled_columns_equal_the_full_loop():
    """whole trees of the forest can be computed on their own (what the GPU tests do on the large forests)"""
    p, i, x = synth.gspd(12, 8, 9)
    L, _ = _factor(_sp(p, i, x))
    nz = L.p[L.n]
    full = SI.sparseinv_x(L.n, L.p, L.i[:nz], L.x[:nz])
    cols = list(range(16, 24)) + list(range(88, 96))
    part = SI.sparseinv_x(L.n, L.p, L.i[:nz], L.x[:nz], cols)
    for j in range(L.n):
        for q in range(L.p[j], L.p[j + 1]):
            assert part[q] == (full[q] if j in cols else None)


def test_not_a_cholesky_pattern_raises():
    p, i, x = synth.gspd(1, 8, 1)
    L, _ = _factor(_sp(p, i, x))
    nz = L.p[L.n]
    Lp, Li, Lx = list(L.p), list(L.i[:nz]), list(L.x[:nz])
    q = Lp[2] + 2                                   # entry (4, 2) leaves: column 0 still pairs rows 2 and 4
    del Li[q], Lx[q]
    Lp = [v if c <= 2 else v - 1 for c, v in enumerate(Lp)]
    with pytest.raises(ValueError):
        SI.sparseinv_x(L.n, Lp, Li, Lx)


def test_abi_declares_and_binds_the_three_functions():
    import _csx
    text = open(os.path.join(ROOT, "include", "csx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in (("csx_chol_inverse", 2), ("csx_chol_inverse_info", 4), ("csx_csc_diag", 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
        assert len(_csx._PROTOS[name]) == arity, name
        assert hasattr(_csx.load(), name)
