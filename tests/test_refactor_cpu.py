"""Refactor on the CPU: the rule of tests/refactor_oracle.py applied to csparse_oracle.cs_lu's factors is
byte-equal to cs_lu of the new values wherever the pivots hold, and the product's host loop (csx_lu_refactor_host) is
byte-equal to the rule -- duplicates, a column order, a zero pivot and a changed pattern included."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import btf_oracle
import csparse_oracle as O
import refactor_oracle as R
from conftest import golden


def _fixture(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])
    p = g["C_p"].astype(np.int64)
    S = sp.coo_matrix(sp.csc_matrix((g["C_x"][:p[n]], g["C_i"][:p[n]], p), shape=(m, n))).tocsc()
    S.sum_duplicates()
    return S


def _reducible():
    S, _, _ = btf_oracle.reducible(btf_oracle.block_sizes(600, 5), 4, 5)
    return S


def _ocs(n, p, i, x):
    A = O.cs_spalloc(n, n, max(len(i), 1), True, False)
    A.p, A.i, A.x = [int(v) for v in p], [int(v) for v in i] or [0], [float(v) for v in x] or [0.0]
    return A


def _lu(n, p, i, x, tol):
    A = _ocs(n, p, i, x)
    return O.cs_lu(A, O.cs_sqr(0, A, False), tol)


def _entrywise(S, seed):
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, S.nnz)
    return S.data * (1.0 + 1e-3 * u)


def _columnwise(S, seed):
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, S.shape[1])
    return S.data * (1.0 + 1e-3 * u)[np.repeat(np.arange(S.shape[1]), np.diff(S.indptr))]


def _factors(N):
    n = len(N.pinv)
    out = []
    for M in (N.L, N.U):
        nnz = M.p[n]
        out.append((list(M.p[:n + 1]), list(M.i[:nnz]), [float(v) for v in M.x[:nnz]]))
    return out


def _host_refactor(N, n, Ap, Ai, Ax):
    """csx_lu_refactor_host on the oracle's factors: (Lx, Ux, ok, ratio), or the status when it is not CSX_OK"""
    import _csx
    (Lp, Li, Lx), (Up, Ui, Ux) = _factors(N)
    Lx2, Ux2 = np.zeros(max(len(Li), 1)), np.zeros(max(len(Ui), 1))
    ok, ratio = C.c_int(-1), C.c_double(-1.0)
    st = _csx.load().csx_lu_refactor_host(n, _csx.pi(_csx.i32(Ap)), _csx.pi(_csx.i32(Ai)), _csx.pd(_csx.f64(Ax)),
                                          _csx.pi(_csx.i32(N.pinv)), _csx.pi(_csx.i32(Lp)), _csx.pi(_csx.i32(Li)),
                                          _csx.pd(Lx2), _csx.pi(_csx.i32(Up)), _csx.pi(_csx.i32(Ui)), _csx.pd(Ux2),
                                          ok, ratio)
    if st != _csx.OK:
        return st
    return Lx2[:len(Li)], Ux2[:len(Ui)], bool(ok.value), ratio.value


CASES = [  # (name, perturbation, tol): cases whose pinv holds under the perturbation (checked below, loudly)
    ("reducible", _entrywise, 1.0),
    ("reducible", _entrywise, 0.001),
    ("fs_183_1", _entrywise, 0.001),
    ("bcsstk01", _entrywise, 0.001),
    ("west0067", _columnwise, 0.001),
]


def _matrix(name):
    return _reducible() if name == "reducible" else _fixture(name)


@pytest.mark.parametrize("name,perturb,tol", CASES)
def test_rule_equals_cs_lu_of_the_new_values(name, perturb, tol):
    S = _matrix(name)
    n = S.shape[0]
    N = _lu(n, S.indptr, S.indices, S.data, tol)
    x2 = perturb(S, 7)
    N2 = _lu(n, S.indptr, S.indices, x2, tol)
    assert N is not None and N2 is not None
    assert list(N2.pinv) == list(N.pinv), "the perturbation moved a pivot: pick another case"
    Lx, Ux, ok, ratio = R.refactor(N.L, N.U, N.pinv, (S.indptr.tolist(), S.indices.tolist(), x2.tolist()))
    assert ok and 0.0 < ratio <= 1.0
    (_, _, Lx2), (_, _, Ux2) = _factors(N2)
    assert np.asarray(Lx).tobytes() == np.asarray(Lx2).tobytes()
    assert np.asarray(Ux).tobytes() == np.asarray(Ux2).tobytes()
    if tol == 1.0:
        assert ratio == 1.0       # partial pivoting chose every pivot as a largest candidate


@pytest.mark.parametrize("name,perturb,tol", CASES)
def test_host_loop_equals_rule(name, perturb, tol):
    S = _matrix(name)
    n = S.shape[0]
    N = _lu(n, S.indptr, S.indices, S.data, tol)
    x2 = perturb(S, 11)
    want = R.refactor(N.L, N.U, N.pinv, (S.indptr.tolist(), S.indices.tolist(), x2.tolist()))
    Lx, Ux, ok, ratio = _host_refactor(N, n, S.indptr, S.indices, x2)
    assert ok == want[2] and ok
    assert Lx.tobytes() == np.asarray(want[0]).tobytes()
    assert Ux.tobytes() == np.asarray(want[1]).tobytes()
    assert np.float64(ratio).tobytes() == np.float64(want[3]).tobytes()


def test_host_loop_with_duplicates():
    """cs_spsolve assigns: of two entries of one row in a column the later one counts, in the rule and in the host loop"""
    S = _fixture("west0067")
    n = S.shape[0]
    p, i, x = [0], [], []
    rng = np.random.default_rng(3)
    for j in range(n):
        a, e = S.indptr[j], S.indptr[j + 1]
        i += S.indices[a:e].tolist()
        x += S.data[a:e].tolist()
        if j % 3 == 0 and e > a:                   # a second entry for the column's first row, after the others
            i.append(int(S.indices[a]))
            x.append(float(S.data[a]) * 2.0)
        p.append(len(i))
    N = _lu(n, p, i, x, 0.001)
    assert N is not None
    u = rng.uniform(-1, 1, n)
    x2 = (np.asarray(x) * (1.0 + 1e-3 * u)[np.repeat(np.arange(n), np.diff(p))]).tolist()
    want = R.refactor(N.L, N.U, N.pinv, (p, i, x2))
    Lx, Ux, ok, ratio = _host_refactor(N, n, p, i, x2)
    assert ok and Lx.tobytes() == np.asarray(want[0]).tobytes() and Ux.tobytes() == np.asarray(want[1]).tobytes()
    assert ratio == want[3]


def test_host_loop_with_a_column_order():
    """order > 0: column k of the factorisation is column q[k] of A, so the refactor reads A2(:, q)"""
    S = _fixture("fs_183_1")
    n = S.shape[0]
    q = np.random.default_rng(5).permutation(n)
    Sq = S[:, q].tocsc()
    N = _lu(n, Sq.indptr, Sq.indices, Sq.data, 0.001)
    x2 = _columnwise(S, 13)
    S2q = sp.csc_matrix((x2, S.indices, S.indptr), shape=S.shape)[:, q].tocsc()
    assert np.array_equal(S2q.indptr, Sq.indptr) and np.array_equal(S2q.indices, Sq.indices)
    N2 = _lu(n, S2q.indptr, S2q.indices, S2q.data, 0.001)
    assert list(N2.pinv) == list(N.pinv)
    Lx, Ux, ok, ratio = _host_refactor(N, n, S2q.indptr, S2q.indices, S2q.data)
    (_, _, Lw), (_, _, Uw) = _factors(N2)
    assert ok and Lx.tobytes() == np.asarray(Lw).tobytes() and Ux.tobytes() == np.asarray(Uw).tobytes()


def test_zero_pivot_is_not_ok():
    # [[1, 1], [1, 1]] after [[2, 1], [1, 1]]: the second pivot becomes 1 - 1 * 1 = 0
    p, i = [0, 2, 4], [0, 1, 0, 1]
    N = _lu(2, p, i, [2.0, 1.0, 1.0, 1.0], 1.0)
    assert list(N.pinv) == [0, 1]
    want = R.refactor(N.L, N.U, N.pinv, (p, i, [1.0, 1.0, 1.0, 1.0]))
    assert want[2] is False
    got = _host_refactor(N, 2, p, i, [1.0, 1.0, 1.0, 1.0])
    assert got[2] is False
    got = _host_refactor(N, 2, p, i, [np.nan, 1.0, 1.0, 1.0])
    assert got[2] is False


def test_changed_pattern_is_rejected():
    import _csx
    S = _fixture("west0067")
    n = S.shape[0]
    N = _lu(n, S.indptr, S.indices, S.data, 0.001)
    # an entry in a row that neither L(:,k) nor U(:,k) holds
    Lp, Li = N.L.p, N.L.i
    Up, Ui = N.U.p, N.U.i
    k = 10
    held = set(Li[Lp[k]:Lp[k + 1]]) | set(Ui[Up[k]:Up[k + 1]])
    pinv_inv = np.argsort(N.pinv)
    row = next(int(pinv_inv[r]) for r in range(n) if r not in held)
    D = S.tolil()
    D[row, k] = 1.0
    D = D.tocsc()
    D.sort_indices()
    assert _host_refactor(N, n, D.indptr, D.indices, D.data) == _csx.EINVAL
