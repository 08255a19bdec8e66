"""csx_ldl_host (the value rule of csx_ldl_factor on host arrays) against the Python restatement
(tests/ldl_oracle.py), the textbook backward-error bound of the recurrence in exact rational arithmetic, the restated cs_chol on
an SPD matrix, Sylvester's law against the dense spectrum, and the conditions that the GPU tests (tests/test_gpu_ldl.py) rely on,
held here so that the host rule alone meets them.  No device.

The Cholesky comparison is against oracle/csparse_oracle.py's cs_chol: the reference's own cs_chol does not run, so
tests/golden/ holds no factor of it; the restatement is what every other Cholesky test of this repository compares with."""
from fractions import Fraction

import numpy as np
import pytest

import c_oracle as CO
import csparse_oracle as O
import ldl_cases as LC
import ldl_oracle as LO
import residual_sym_oracle as RSO
from chol_refactor_cases import _golden_C

EPS = 2.0 ** -52
VECTORISED = ("long-column", "long-column-updated")     # see ldl_oracle.ldl


def _same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def _rule(case, x, tau, **kw):
    Lp, Li, _ = LO.pattern_of(case)
    return LO.ldl(case.n, case.p, case.i, x, LO.pinv_of(case), Lp, Li, tau, **kw)


@pytest.mark.parametrize("name", LC.NAMES)
def test_host_rule_is_the_restatement(name):
    case = LC.BY_NAME[name]
    for which in LC.VALUE_SETS:
        x = case.values(which)
        Lx, d, info = LO.reference(case, which)
        rx, rd, rinfo = _rule(case, x, LO.tau_of(case, x), vectorised=name in VECTORISED)
        assert info == rinfo and info[3] == -1, which
        assert _same(Lx, rx) and _same(d, rd), which
    # the breaking value set: the same column reported, nothing said about the values
    bad = case.breaking(LO.first_column(case))
    tau = LO.tau_of(case, bad)
    st, _, _, info = LO.host(case, bad, tau)
    assert st == 0 and info[3] == 0
    assert _rule(case, bad, tau, vectorised=name in VECTORISED)[2][3] == 0


@pytest.mark.parametrize("name", [n for n in LC.NAMES if n not in VECTORISED])
def test_the_vectorised_restatement_is_the_plain_one(name):
    case = LC.BY_NAME[name]
    x = case.A2[0]
    tau = LO.tau_of(case, x)
    a, b = _rule(case, x, tau), _rule(case, x, tau, vectorised=True)
    assert a[2] == b[2] and _same(a[0], b[0]) and _same(a[1], b[1])


@pytest.mark.parametrize("name", ["grid24-shift", "grid24-shift-natural"])
def test_descending_updates_or_a_fused_subtraction_give_other_bytes(name):
    case = LC.BY_NAME[name]
    Lx, d, _ = LO.reference(case, "A")
    for mistake in ("descending", "fused"):
        rx, rd, _ = _rule(case, case.x, 0.0, **{mistake: True})
        assert not _same(Lx, rx), mistake
        assert np.allclose(Lx, rx, rtol=1e-6, atol=1e-9), mistake     # (a mistake of rounding, not of arithmetic)


def test_update_batches_has_the_rows_it_names_and_no_vanishing_pivot():
    """the forest of stars: L has no fill, the hub rows hold exactly 0, 1, 7, 8, 9, 16 and 17 entries before the diagonal (the
    updates their columns take), every other row none; no pivot of any value set is zero, perturbed or a breakdown"""
    case = LC.BY_NAME["update-batches"]
    Lp, Li, _ = LO.pattern_of(case)
    assert case.n == 65 and Lp[-1] == case.n + sum(LC.STAR_LEAVES)
    updates = np.bincount(np.asarray(Li), minlength=case.n) - 1
    hubs = LC.star_hubs()
    assert sorted(hubs.values()) == [0, 1, 7, 8, 9, 16, 17]
    assert all(updates[j] == hubs.get(j, 0) for j in range(case.n))
    diag = case.x[case.i == case.cols]
    assert len(set(diag.tolist())) == case.n and np.any(diag > 0) and np.any(diag < 0)
    for which in LC.VALUE_SETS:
        _, d, info = LO.reference(case, which)
        assert info[2:] == (0, -1) and np.all(np.isfinite(d)) and np.all(d != 0.0), which


def _bound_holds(n, Lp, Li, Lx, d, C):
    """|C - L D L'| <= (n + 1) 2^-52 |L| |D| |L'| entry by entry on the lower triangle, in exact rationals.  C: {(r, c): value},
    r >= c, in L's numbering.  Entries outside the pattern of L are structurally zero on both sides."""
    exact, size = {}, {}
    fx, fd = [Fraction(float(v)) for v in Lx], [Fraction(float(v)) for v in d]
    for k in range(n):
        for a in range(Lp[k], Lp[k + 1]):
            t = fx[a] * fd[k]
            for b in range(Lp[k], a + 1):
                key = (Li[a], Li[b])
                term = t * fx[b]
                exact[key] = exact.get(key, 0) + term
                size[key] = size.get(key, 0) + abs(term)
    gamma = (n + 1) * Fraction(EPS)
    assert set(C) <= set(exact)
    return all(abs(Fraction(C.get(key, 0.0)) - exact[key]) <= gamma * size[key] for key in exact)


def _lower_entries(case, x):
    pinv = LO.pinv_of(case)
    out = {}
    for q in range(len(case.i)):
        r, c = int(case.i[q]), int(case.cols[q])
        if r <= c:
            r2, c2 = (r, c) if pinv is None else (pinv[r], pinv[c])
            out[(max(r2, c2), min(r2, c2))] = float(x[q])
    return out


@pytest.mark.parametrize("name", ["grid24-shift", "kkt-sqd"])
def test_componentwise_backward_error_of_the_factorisation(name):
    case = LC.BY_NAME[name]
    Lp, Li, _ = LO.pattern_of(case)
    Lx, d, _ = LO.reference(case, "A")
    assert _bound_holds(case.n, Lp, Li, Lx, d, _lower_entries(case, case.x))


@pytest.fixture(scope="module")
def bcsstk01():
    n, p, i, x = _golden_C("bcsstk01")
    case = LC.Case("bcsstk01", n, p, i, x, seed=99)
    return case, LO.reference(case, "A")


def test_bcsstk01_bound_and_cholesky(bcsstk01):
    case, (Lx, d, info) = bcsstk01
    Lp, Li, _ = LO.pattern_of(case)
    assert info == (case.n, 0, 0, -1)
    assert _bound_holds(case.n, Lp, Li, Lx, d, _lower_entries(case, case.x))
    # SPD: L sqrt(D) is the Cholesky factor, the restated cs_chol's to the north-star tolerance
    A = case.matrix(O)
    N = O.cs_chol(A, O.cs_schol(0, A))
    assert list(N.L.p) == Lp and list(N.L.i[:Lp[-1]]) == Li
    ref = np.asarray(N.L.x[:Lp[-1]])
    got = Lx * np.sqrt(d)[np.repeat(np.arange(case.n), np.diff(Lp))]
    assert np.all(ref != 0.0) and np.all(np.abs(got - ref) <= 1e-10 * np.abs(ref))       # (observed: 2.8e-12 at the worst entry)


def _factor(case, which="A", perturb=None):
    x = case.values(which)
    st, Lx, d, info = LO.host(case, x, LO.tau_of(case, x, perturb))
    assert st == 0
    return Lx, d, info


@pytest.mark.parametrize("name", LC.SMALL)
def test_pivot_signs_are_the_eigenvalue_signs(name):
    case = LC.BY_NAME[name]
    for which in LC.VALUE_SETS:
        _, d, info = LO.reference(case, which)
        w = np.linalg.eigvalsh(case.dense(case.values(which)))
        assert info[3] == -1
        assert (info[0], info[1]) == (int(np.sum(w > 0)), int(np.sum(w < 0))) == (int(np.sum(d > 0)), int(np.sum(d < 0))), which


def solve(case, Lx, d, b):
    """P' L^-T D^-1 L^-1 P b with the plain-C triangular solves"""
    Lp, Li, _ = LO.pattern_of(case)
    pinv, n = LO.pinv_of(case), case.n
    x = np.asarray(b, np.float64).copy()
    if pinv is not None:
        y = np.empty(n)
        y[pinv] = x
        x = y
    x = CO.lsolve(n, Lp, Li, Lx, x)
    x = x / d
    x = CO.ltsolve(n, Lp, Li, Lx, x)
    return x if pinv is None else x[pinv]


def omega(case, xs, b, values=None):
    """(R, omega) of one system by the symmetric residual's restatement"""
    R, w, _ = RSO.residual(case.n, case.p, case.i, case.x if values is None else values, 1, xs, b)
    return np.asarray(R), w[0]


def refined(case, Lx, d, b, steps):
    """[omega0, omega1, ...] of plain iterative refinement"""
    x = solve(case, Lx, d, b)
    R, w = omega(case, x, b)
    out = [w]
    for _ in range(steps):
        x = x + solve(case, Lx, d, R)
        R, w = omega(case, x, b)
        out.append(w)
    return out


rhs = LC.rhs


def test_conditions_grid24_shift():
    """what tests/test_gpu_ldl.py relies on: refinement has work to do and does it, the growth is moderate, sigma is no eigenvalue"""
    for name in ("grid24-shift", "grid24-shift-natural"):
        case = LC.BY_NAME[name]
        Lx, d, _ = LO.reference(case, "A")
        off = np.ones(len(Lx), bool)
        off[np.asarray(LO.pattern_of(case)[0][:-1])] = False
        assert np.max(np.abs(Lx[off])) <= 1e4
        for b in rhs(case):
            ws = refined(case, Lx, d, b, 3)
            print(name, [w / EPS for w in ws])
            assert ws[0] >= 16 * EPS
            assert min(ws) <= EPS
    w = np.linalg.eigvalsh(LC.BY_NAME["grid24-shift"].dense())
    assert np.min(np.abs(w)) >= 1e-3                                   # dense() is K - sigma I: its eigenvalues are lambda - sigma


def test_conditions_kkt():
    for name in ("kkt-sqd", "kkt-sqd-natural"):
        case = LC.BY_NAME[name]
        Lx, d, _ = LO.reference(case, "A")
        for b in rhs(case):
            w = refined(case, Lx, d, b, 0)[0]
            print(name, w / EPS)
            assert w <= 4 * EPS                                        # (see ldl_cases.RHS_SEED)
    case = LC.BY_NAME["kkt-zero"]
    assert case.breaks and _factor(case, perturb=0.0)[2][3] >= 0       # an exact zero pivot without the perturbation
    Lx, d, info = LO.reference(case, "A")
    assert case.perturb == 1e-10 and info[2] >= 1 and info[3] == -1
    assert (info[0], info[1]) == (LC.KKT_NH, LC.KKT_NC)
    for b in rhs(case):
        ws = refined(case, Lx, d, b, 3)
        print(case.name, info, [w / EPS for w in ws])
        assert min(ws) <= EPS
