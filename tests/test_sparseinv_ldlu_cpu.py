"""The restatements of sparseinv_ldl / sparseinv_lu (tests/sparseinv_ldlu_oracle.py) and the cases (tests/sparseinv_ldlu_cases.py)
without a device: the numpy forms against the scalar loops byte for byte, the loops against numpy.linalg.inv, the gather rule
under random permutations, the cases against the edges they are named for, and the library's new entry points.

ACCURACY_LDL / ACCURACY_SLU fix, here and not on the device, the solver cases on which tests/test_gpu_sparseinv_ldlu.py holds the
device's entries to the dense inverse: those where the restatement itself, run on a factor made by the same recurrences in
numpy, meets tol.cross_bound(cond_1(A))."""
import numpy as np
import pytest

import sparseinv_ldlu_cases as CASES
import sparseinv_ldlu_oracle as SI
import tol as TOL

# solver cases (tests/ldl_cases.py, tests/slu_cases.py) whose inverse entries are held to the dense inverse on the device
ACCURACY_LDL = ("kkt-sqd", "kkt-sqd-natural", "sparse-trees")
ACCURACY_SLU = ("grid24", "grid24-natural", "blocks")
# ... and those that are not (a shifted operator: static pivots grow, max |l| 79 and more): byte equality only
GROWTH_LDL = ("grid24-shift", "dups")
GROWTH_SLU = ("grid24-shift", "west", "west-nd")


def _lists(c):
    return c.n, c.p.tolist(), c.i.tolist()


@pytest.mark.parametrize("name", CASES.SMALL)
def test_numpy_forms_have_the_bits_of_the_loops(name):
    c = CASES.BY_NAME[name]
    n, p, i = _lists(c)
    z = SI.ldl_x(n, p, i, c.lx.tolist(), c.d.tolist())
    assert np.asarray(z).tobytes() == SI.ldl_x_np(n, c.p, c.i, c.lx, c.d).tobytes()
    zl, zu = SI.lu_x(n, p, i, c.lx.tolist(), c.ux.tolist())
    vl, vu = SI.lu_x_np(n, c.p, c.i, c.lx, c.ux)
    assert np.asarray(zl).tobytes() == vl.tobytes() and np.asarray(zu).tobytes() == vu.tobytes()
    assert np.array_equal(vl[c.p[:-1]], vu[c.p[:-1]])


@pytest.mark.parametrize("name", CASES.SMALL)
def test_loops_against_the_dense_inverse(name):
    c = CASES.BY_NAME[name]
    n, p, i = _lists(c)
    cols = np.repeat(np.arange(n), np.diff(c.p))
    A = c.dense_ldl()
    ref = np.linalg.inv(A)
    bound = TOL.cross_bound(np.linalg.cond(A, 1))
    z = np.asarray(SI.ldl_x(n, p, i, c.lx.tolist(), c.d.tolist()))
    err = TOL.componentwise(z, ref[c.i, cols])
    print(name, "ldl componentwise", err, "bound", bound)
    assert err <= bound
    A = c.dense_lu()
    ref = np.linalg.inv(A)
    bound = TOL.cross_bound(np.linalg.cond(A, 1))
    zl, zu = (np.asarray(v) for v in SI.lu_x(n, p, i, c.lx.tolist(), c.ux.tolist()))
    err = max(TOL.componentwise(zl, ref[c.i, cols]), TOL.componentwise(zu, ref[cols, c.i]))
    print(name, "lu componentwise", err, "bound", bound)
    assert err <= bound


def test_cases_sit_on_the_edges_they_are_named_for():
    for c in CASES.CASES:
        assert CASES.kernels(c) >= c.expect, (c.name, CASES.kernels(c))
        assert float(np.max(np.abs(c.lx))) <= 1.0 and float(np.min(np.abs(c.d))) >= 0.5
        assert np.any(c.d < 0) == (c.n > 1) and (np.any(c.d > 0) or c.n == 1)
    by = CASES.BY_NAME
    assert [k for k, _, _ in CASES.model(by["cliques2x9"])[2]] == ["group<8>"] * 9
    assert "group<16>" not in CASES.kernels(by["cliques2x9"]) and "group<16>" in CASES.kernels(by["cliques2x10"])
    assert "group<32>" not in CASES.kernels(by["cliques2x17"]) and "group<64>" not in CASES.kernels(by["cliques2x33"])
    assert "block<256>" not in CASES.kernels(by["cliques2x65"]) and "wide/1" not in CASES.kernels(by["cliques2x129"])
    assert not any(k.startswith("walk") for c in CASES.CASES if c.name.startswith("cliques2x") for k in CASES.kernels(c))
    # 129 rows below the diagonal: 33 row blocks of four, the last of one row
    assert (129 + 3) // 4 == 33 and 129 % 4 == 1
    nd, widest, launches = CASES.model(by["clique130"])
    assert (nd, widest) == (130, 1) and launches == [("walk<256>", 0, 129), ("wide/1", 129, 1)]
    assert CASES.kernels(by["clique130"], walk=False) == {"group<8>", "group<16>", "group<32>", "group<64>", "block<256>", "wide/1"}
    assert CASES.model(by["chain300"])[2] == [("walk<64>", 0, 300)]
    assert CASES.model(by["cliques2x514"])[:2] == (514, 2)


def test_gather_rule_under_random_permutations():
    """A = L U in a numbering of its own: C = P A(prow, :) P' is what is factored, so inv(A)(x, y) = Z(pinv[x], pinv[prow^-1[y]])"""
    c = CASES.BY_NAME["arrow24x5"]
    n, p, i = _lists(c)
    rng = np.random.default_rng(7)
    C = c.dense_lu()
    pinv, prow = rng.permutation(n), rng.permutation(n)
    perm = np.argsort(pinv)                       # C = A1[perm][:, perm], A1 = A[prow, :]
    A1 = np.empty_like(C)
    A1[np.ix_(perm, perm)] = C
    A = np.empty_like(A1)
    A[prow, :] = A1
    ref = np.linalg.inv(A)
    prinv = np.argsort(prow)
    comb = pinv[prinv]
    zl, zu = SI.lu_x(n, p, i, c.lx.tolist(), c.ux.tolist())
    # every entry of A that is stored: A(r, c) -> inv(A)(c, r) is on the pattern
    r, cc = np.nonzero(A)
    got, missing = SI.gather(n, p, i, zl, zu, pinv, comb, cc, r)
    assert missing == 0
    bound = TOL.cross_bound(np.linalg.cond(A, 1))
    err = TOL.componentwise(got, ref[cc, r])
    print("gather componentwise", err, "bound", bound)
    assert err <= bound
    # a pair off the pattern is NaN and counted
    off = np.argwhere(SI.dense_lower_upper(n, p, i, np.ones(len(i)), None) == 0)[0]
    got, missing = SI.gather(n, p, i, zl, zu, None, None, [off[0], 0], [off[1], 0])
    assert missing == 1 and np.isnan(got[0]) and got[1] == zl[0]
    # the symmetric rule: one array serves both triangles
    z = SI.ldl_x(n, p, i, c.lx.tolist(), c.d.tolist())
    refs = np.linalg.inv(c.dense_ldl())
    got, missing = SI.gather(n, p, i, z, None, None, None, np.asarray(i), np.repeat(np.arange(n), np.diff(c.p)))
    got2, _ = SI.gather(n, p, i, z, None, None, None, np.repeat(np.arange(n), np.diff(c.p)), np.asarray(i))
    assert missing == 0 and got.tobytes() == np.asarray(z).tobytes() == got2.tobytes()
    assert TOL.componentwise(got, refs[i, np.repeat(np.arange(n), np.diff(c.p))]) <= TOL.cross_bound(np.linalg.cond(c.dense_ldl(), 1))


@pytest.mark.parametrize("name", ["cliques2x17", "arrow24x5", "ragged"])
def test_lu_of_a_symmetric_matrix_has_equal_triangles(name):
    """Ut = L D: the factor of the symmetric L D L'; ZL and ZUt then agree to the bound (not to the bit: ZUt divides by d)"""
    c = CASES.BY_NAME[name]
    n, p, i = _lists(c)
    cols = np.repeat(np.arange(n), np.diff(c.p))
    ux = c.lx * c.d[cols]
    zl, zu = (np.asarray(v) for v in SI.lu_x(n, p, i, c.lx.tolist(), ux.tolist()))
    bound = TOL.cross_bound(np.linalg.cond(c.dense_ldl(), 1))
    err = TOL.componentwise(zl, zu)
    print(name, "ZL against ZUt", err, "bound", bound)
    assert err <= bound
    z = np.asarray(SI.ldl_x(n, p, i, c.lx.tolist(), c.d.tolist()))
    assert TOL.componentwise(zl, z) <= bound


def _factor_ldl(A):
    """unit L and d of a dense symmetric A without pivoting (the static order): numpy, for the accuracy lists only"""
    n = A.shape[0]
    A = A.copy()
    L, d = np.eye(n), np.zeros(n)
    for j in range(n):
        d[j] = A[j, j]
        L[j + 1:, j] = A[j + 1:, j] / d[j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], A[j, j + 1:])
    return L, d


def _factor_lu(A):
    n = A.shape[0]
    A = A.copy()
    L = np.eye(n)
    for j in range(n):
        L[j + 1:, j] = A[j + 1:, j] / A[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], A[j, j + 1:])
        A[j + 1:, j] = 0.0
    return L, A


def _symbolic(pattern):
    """the filled lower pattern (boolean) of a symmetric boolean pattern, by elimination in the natural order"""
    F = np.tril(pattern | pattern.T) | np.eye(len(pattern), dtype=bool)
    for j in range(len(F)):
        r = np.nonzero(F[j + 1:, j])[0] + j + 1
        F[np.ix_(r, r)] |= np.tril(np.ones((len(r), len(r)), dtype=bool))
    return F


def _restatement_error(A, kind):
    """componentwise error against inv(A) of the restatement run on a numpy no-pivot factor of the dense A, and the bound"""
    n = A.shape[0]
    F = _symbolic(A != 0.0)
    cols, rows = np.nonzero(F.T)                   # column-major: columns ascending, rows ascending inside
    p = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).tolist()
    ref = np.linalg.inv(A)
    bound = TOL.cross_bound(np.linalg.cond(A, 1))
    if kind == "ldl":
        L, d = _factor_ldl(A)
        z = SI.ldl_x_np(n, p, rows, L[rows, cols], d)
        return TOL.componentwise(z, ref[rows, cols]), bound, float(np.max(np.abs(np.tril(L, -1)))) if n > 1 else 0.0
    L, U = _factor_lu(A)
    zl, zu = SI.lu_x_np(n, p, rows, L[rows, cols], U[cols, rows])
    err = max(TOL.componentwise(zl, ref[rows, cols]), TOL.componentwise(zu, ref[cols, rows]))
    return err, bound, float(np.max(np.abs(np.tril(L, -1))))


def _ldl_dense(name):
    import ldl_cases
    c = ldl_cases.BY_NAME[name]
    return c.dense()


def _slu_dense(name):
    import slu_cases
    c = slu_cases.BY_NAME[name]
    A = c.dense()
    if c.prow is not None:
        A = A[c.prow, :]
    return A


@pytest.mark.parametrize("name", ACCURACY_LDL + GROWTH_LDL)
def test_which_ldl_solver_cases_the_restatement_itself_holds_to_the_dense_inverse(name):
    """natural order here whatever the case's: the list is about the operator's growth under static pivots"""
    err, bound, growth = _restatement_error(_ldl_dense(name), "ldl")
    print(name, "restatement against the dense inverse", err, "bound", bound, "max |l|", growth)
    assert (err <= bound) == (name in ACCURACY_LDL)


@pytest.mark.parametrize("name", ACCURACY_SLU + GROWTH_SLU)
def test_which_slu_solver_cases_the_restatement_itself_holds_to_the_dense_inverse(name):
    err, bound, growth = _restatement_error(_slu_dense(name), "lu")
    print(name, "restatement against the dense inverse", err, "bound", bound, "max |l|", growth)
    assert (err <= bound) == (name in ACCURACY_SLU)


def test_library_exports_the_new_entry_points():
    import _csx
    lib = _csx.load()
    for name in ("csx_ldl_inverse", "csx_slu_inverse", "csx_inverse_at"):
        assert hasattr(lib, name), name
        assert name in _csx._PROTOS and getattr(lib, name).argtypes == _csx._PROTOS[name]
