"""csx_residual_sym_host (the value rule of csx_residual_sym_block on host arrays) against the Python
restatement tests/residual_sym_oracle.py: byte-equal R, omega and rnorm on the golden matrices as cs_compress left them and on
seeded values of magnitudes 1e-8 .. 1e8, k = 1 and 3, R stored, not stored and in place; the two mistakes the restatement
keeps give other bytes; the storages of one operator give the same bytes, and the full sorted one those of csx_residual_host;
the special cases of the rule; and the refinement fixture of tests/residual_sym_cases.py does, on restated solves, what
tests/test_gpu_cholsol_refine.py relies on.  No GPU.

ibm32a (32 x 31) and mbeacxc (492 x 490) are not square as the fixtures hold them: their leading n x n part is taken (the
entries of the rows past n left out, the rest where it was).  bcsstk01 and bcsstk16 are stored as their LOWER triangle, so
their S is the diagonal alone; their transposes (the fixtures' AT: the upper triangle) are run as well."""
import numpy as np
import pytest

import c_oracle as CO
import refine_cases
import residual_sym_cases as SC
import residual_sym_oracle as RSO
from chol_refactor_cases import CASES
from conftest import golden

GOLDEN = ("bcsstk01", "bcsstk16", "west0067", "fs_183_1", "ibm32a", "mbeacxc", "bcsstk01'", "bcsstk16'")
KS = (1, 3)
EPS = SC.EPS


def _matrix(name):
    """cs_compress's output of the fixture (unsorted columns, duplicates kept), cut to its leading square part"""
    prefix = "AT" if name.endswith("'") else "A"
    g = golden(name.rstrip("'"))
    m, n = int(g[prefix + "_mn"][0]), int(g[prefix + "_mn"][1])
    p = g[prefix + "_p"].astype(np.int64)
    nnz = int(p[n])
    i, x = g[prefix + "_i"][:nnz].astype(np.int64), g[prefix + "_x"][:nnz].astype(np.float64)
    cols = np.repeat(np.arange(n), np.diff(p))
    n = min(m, n)
    keep = (i < n) & (cols < n)
    return SC._csc(n, cols[keep], i[keep], x[keep])


def _wide(rng, count):
    """signed values of magnitudes 1e-8 .. 1e8"""
    return rng.choice([-1.0, 1.0], count) * 10.0 ** rng.uniform(-8.0, 8.0, count)


def _host(n, p, i, x, k, X, B, store=True, in_place=False, status=False):
    import _csx
    lib = _csx.load()
    p, i, x = np.ascontiguousarray(p, np.int32), np.ascontiguousarray(i, np.int32), np.ascontiguousarray(x, np.float64)
    X, B = np.ascontiguousarray(X, dtype=np.float64), np.array(B, dtype=np.float64)
    R = B if in_place else (np.full(n * k, 7.0) if store else None)
    omega, rnorm = np.full(k, -1.0), np.full(k, -1.0)
    st = lib.csx_residual_sym_host(n, _csx.pi(p), _csx.pi(i), _csx.pd(x), k, _csx.pd(X), _csx.pd(B), _csx.pd(R), _csx.pd(omega),
                                   _csx.pd(rnorm))
    if status:
        return st
    assert st == _csx.OK
    return R, omega, rnorm


def _general(n, p, i, x, k, X, B):
    import _csx
    p, i, x = np.ascontiguousarray(p, np.int32), np.ascontiguousarray(i, np.int32), np.ascontiguousarray(x, np.float64)
    X, B = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(B, dtype=np.float64)
    R, omega, rnorm = np.empty(n * k), np.empty(k), np.empty(k)
    assert _csx.load().csx_residual_host(n, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), k, 0, _csx.pd(X), _csx.pd(B), _csx.pd(R),
                                         _csx.pd(omega), _csx.pd(rnorm)) == _csx.OK
    return R, omega, rnorm


def _inputs(name, k, seeded):
    n, p, i, x = _matrix(name)
    rng = np.random.default_rng(1000 * k + 10 * len(name) + (100 if seeded else 0))
    if seeded:
        x = _wide(rng, len(x))
        X, B = _wide(rng, n * k), _wide(rng, n * k)
    else:
        X, B = rng.standard_normal(n * k) * 4.0, rng.standard_normal(n * k)
    return n, p, i, x, X, B


def _same(got, ref):
    return np.asarray(got, dtype=np.float64).tobytes() == np.asarray(ref, dtype=np.float64).tobytes()


@pytest.mark.parametrize("name", GOLDEN)
def test_host_rule_is_the_restatement(name):
    for seeded in (False, True):
        for k in KS:
            n, p, i, x, X, B = _inputs(name, k, seeded)
            R, omega, rnorm = _host(n, p, i, x, k, X, B)
            Rr, wr, ar = RSO.residual(n, p, i, x, k, X, B)
            assert _same(R, Rr), (name, k, seeded)
            assert _same(omega, wr) and _same(rnorm, ar), (name, k, seeded)
            # omega and rnorm alone, and in place: the same numbers
            none, w2, a2 = _host(n, p, i, x, k, X, B, store=False)
            assert none is None and _same(w2, wr) and _same(a2, ar)
            R3, w3, a3 = _host(n, p, i, x, k, X, B, in_place=True)
            assert _same(R3, Rr) and _same(w3, wr) and _same(a3, ar)


@pytest.mark.parametrize("name", GOLDEN)
def test_the_phases_swapped_or_the_lower_entries_kept_give_other_bytes(name):
    """on the inputs of the test above.  Where the stored matrix has nothing strictly above the diagonal (bcsstk01 and bcsstk16
    as stored: S is their diagonal) every row has one term and the order of the phases cannot show: the same bytes there;
    where it has nothing strictly below (their transposes), keeping the lower entries cannot show."""
    k = 3
    n, p, i, x, X, B = _inputs(name, k, True)
    cols = np.repeat(np.arange(n), np.diff(p))
    right = _host(n, p, i, x, k, X, B)[0]
    swapped = RSO.residual(n, p, i, x, k, X, B, phase2_first=True)[0]
    lower = RSO.residual(n, p, i, x, k, X, B, keep_lower=True)[0]
    assert _same(swapped, right) == (not (i < cols).any()), name
    assert _same(lower, right) == (not (i > cols).any()), name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_storages_of_one_operator_give_the_same_bytes(case):
    n = case.n
    k = 3
    rng = np.random.default_rng(case.n + len(case.name))
    X, B = rng.standard_normal(n * k) * 4.0, rng.standard_normal(n * k)
    stored = (n, case.p, case.i, case.x)
    want = _host(*stored, k, X, B)
    for other in (SC.upper_only(*stored), SC.with_lower(*stored, 1, False), SC.with_lower(*stored, 2, True)):
        got = _host(*other, k, X, B)
        assert all(_same(a, b) for a, b in zip(got, want)), case.name
    full = SC.full_sorted(*stored)
    sym, gen = _host(*full, k, X, B), _general(*full, k, X, B)
    assert all(_same(a, b) for a, b in zip(sym, gen)), case.name
    # (the full sorted storage takes the upper entries in sorted order: the bytes of the stored one where that is sorted too)
    cols = np.repeat(np.arange(n), np.diff(case.p))
    up = case.i <= cols
    if all((np.diff(case.i[up][cols[up] == j]) >= 0).all() for j in range(n)):
        assert all(_same(a, b) for a, b in zip(sym, want)), case.name


def test_special_cases():
    i32, f64 = (lambda v: np.asarray(v, np.int32)), (lambda v: np.asarray(v, np.float64))
    # n = 0: nothing to do, the maxima are 0
    R, w, a = _host(0, i32([0]), i32([]), f64([]), 2, f64([]), f64([]))
    assert w.tolist() == [0.0, 0.0] and a.tolist() == [0.0, 0.0]
    # n = 1
    R, w, a = _host(1, i32([0, 1]), i32([0]), f64([-1.5]), 1, f64([2.0]), f64([1.0]))
    assert R.tolist() == [4.0] and w.tolist() == [1.0] and a.tolist() == [4.0]
    assert all(_same(g, r) for g, r in zip((R, w, a), RSO.residual(1, [0, 1], [0], [-1.5], 1, [2.0], [1.0])))
    # nnz = 0: R = B, omega by the 0 / 0 rule
    B = f64([1.0, 0.0, -2.0, 0.0, 3.0, 0.0])
    R, w, a = _host(3, i32([0, 0, 0, 0]), i32([]), f64([]), 2, f64([5.0] * 6), B)
    assert _same(R, B) and w.tolist() == [1.0, 0.0] and a.tolist() == [3.0, 0.0]
    # a missing diagonal: S = [[0, 2], [2, 3]] from the entries (0, 1) and (1, 1), and a lower entry that is not read
    p, i, x = i32([0, 1, 3]), i32([1, 0, 1]), f64([50.0, 2.0, 3.0])
    R, w, a = _host(2, p, i, x, 1, f64([1.0, 1.0]), f64([2.0, 5.0]))
    assert R.tolist() == [0.0, 0.0] and w.tolist() == [0.0] and a.tolist() == [0.0]
    assert all(_same(g, r) for g, r in zip((R, w, a), RSO.residual(2, p, i, x, 1, [1.0, 1.0], [2.0, 5.0])))
    # skipped entries are not added as zeros: b = -0.0 on a row whose only stored entry is strictly lower stays -0.0
    p, i, x = i32([0, 1, 1]), i32([1]), f64([4.0])
    R, w, a = _host(2, p, i, x, 1, f64([0.0, 0.0]), f64([-0.0, -0.0]))
    assert np.signbit(R).tolist() == [True, True] and w.tolist() == [0.0]
    # bad structure
    assert _host(2, i32([0, 1, 2]), i32([0, 2]), f64([1.0, 1.0]), 1, f64([1.0, 1.0]), f64([1.0, 1.0]), status=True) != 0
    assert _host(2, i32([0, 1, 2]), i32([0, 1]), f64([1.0, 1.0]), 0, f64([1.0, 1.0]), f64([1.0, 1.0]), status=True) != 0


def test_a_nan_stays_in_its_column():
    n, p, i, x = _matrix("fs_183_1")
    k = 3
    rng = np.random.default_rng(4)
    X, B = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    X[int(i[0]), 1] = np.nan
    R, w, a = _host(n, p, i, x, k, X, B)
    Rr, wr, ar = RSO.residual(n, p, i, x, k, X.reshape(-1), B.reshape(-1))
    assert np.isnan(w[1]) and np.isnan(a[1]) and np.isnan(wr[1])
    clean = _host(n, p, i, x, k, np.where(np.isnan(X), 0.0, X), B)
    for c in (0, 2):
        assert w[c] == clean[1][c] and a[c] == clean[2][c] and _same(w[c], wr[c])
        assert R.reshape(n, k)[:, c].tobytes() == clean[0].reshape(n, k)[:, c].tobytes()


def test_residual_block_answers_bad_arguments_without_the_device():
    import csparse as cs
    T = cs.cs_spalloc(3, 3, 4, True, True)
    A = cs.cs_spalloc(3, 2, 4, True, False)
    A.p = [0, 0, 0]
    Q = cs.cs_spalloc(3, 3, 4, True, False)
    Q.p = [0, 0, 0, 0]
    assert cs.residual_block(T, np.ones((3, 4)), np.ones((3, 4)), sym=True) is False
    assert cs.residual_block(A, np.ones((2, 4)), np.ones((3, 4)), sym=True) is False          # not square
    assert cs.residual_block(A, np.ones((3, 4)), np.ones((3, 4)), trans=True, sym=True) is False
    assert cs.residual_block(Q, None, np.ones((3, 4)), sym=True) is False
    assert cs.residual_block(Q, np.ones((3, 4)), np.ones((3, 5)), sym=True) is False          # unequal k
    with pytest.raises(IndexError):
        cs.residual_block(Q, np.ones((2, 4)), np.ones((3, 4)), sym=True)
    with pytest.raises(IndexError):
        cs.residual_block(Q, np.ones((3, 4)), np.ones((2, 4)), sym=True, trans=True)
    P = cs.cs_spalloc(3, 3, 4, False, False)
    P.p = [0, 0, 0, 0]
    with pytest.raises(TypeError):
        cs.residual_block(P, np.ones((3, 4)), np.ones((3, 4)), sym=True)


# --------------------------------------------------------------------------------------- the refinement fixture --

def _restatement(seed, k=3):
    """solve(B): the plain-C cs_lsolve / cs_ltsolve on the plain-C factor of A; residual(X, B): the host rule on A2 (and on A),
    which the tests above hold to the restatement -- as is the final omega here"""
    n, Ap, Ai, Ax, Ax2 = SC.perturbed_spd(seed)
    parent, cp = CO.schol(n, Ap, Ai)
    L = CO.chol(n, Ap, Ai, Ax, parent, cp)
    assert L is not None
    Lp, Li, Lx = L

    def solve(Bk):
        return np.column_stack([CO.ltsolve(n, Lp, Li, Lx, CO.lsolve(n, Lp, Li, Lx, np.ascontiguousarray(Bk[:, c])))
                                for c in range(Bk.shape[1])])

    def residual_on(values):
        def residual(X, Bk):
            kk = Bk.shape[1]
            R, w, _ = _host(n, Ap, Ai, values, kk, X, Bk)
            return R.reshape(n, kk), w
        return residual

    def restated(X, Bk):
        return RSO.residual(n, Ap, Ai, Ax2, Bk.shape[1], X.reshape(-1).tolist(), Bk.reshape(-1).tolist())[1]

    return SC.rhs(n, k, seed), solve, residual_on(Ax2), residual_on(Ax), restated


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_a_stale_factor_loses_digits_and_refinement_wins_them_back(seed):
    B, solve, residual, own, restated = _restatement(seed)
    out = refine_cases.refine_loop(solve, residual, B)
    print("omega0 / eps", out["omega0"] / EPS, "omega / eps", out["omega"] / EPS, "steps", out["steps"])
    assert (out["omega0"] >= 1e6 * EPS).all()
    assert (out["omega"] <= EPS).all() and (out["steps"] <= 3).all()
    assert (out["omega"] <= out["omega0"]).all()
    assert np.asarray(residual(out["x"], B)[1]).tobytes() == out["omega"].tobytes()
    assert np.asarray(restated(out["x"], B)).tobytes() == out["omega"].tobytes()
    # against the factored matrix itself a solve is backward stable: at most one step
    mine = refine_cases.refine_loop(solve, own, B)
    print("own matrix: omega0 / eps", mine["omega0"] / EPS, "omega / eps", mine["omega"] / EPS, "steps", mine["steps"])
    assert (mine["steps"] <= 1).all()
