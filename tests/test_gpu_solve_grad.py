"""solve_grad() of the six solvers.  Wiring: gb is the solver's own solve of gx in the other direction and gA the
host rule applied to the downloaded (gb, x) -- the roles of U and V, the sign, the mode and the direction, byte for byte.  Exact:
on the dyadic fixtures of tests/outer_cases.py (shown exact on the host rules by tests/test_outer_cases_cpu.py) gb and gA EQUAL
the computation in fractions.Fraction, no tolerance (the sign of a zero aside, which a Fraction does not hold).  Real matrices:
gA against numpy's dense solve within tests/grad_tol.py's measured bound.  And refine=, the operator rule of the symmetric
solvers, and the argument checks."""
import numpy as np
import pytest

import _csx
import grad_tol as GT
import hqr_cases as HC
import outer_cases as OC
import refine_cases as RC
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

WIRING = ("stale-pivot-lusol", "stale-pivot-btf", "slu-saddle-natural", "hqr-west", "ldl-kkt-sqd", "chol-bcsstk01")


def _solved(cs, F, B, **kw):
    """the solver's own solve of the block B (numpy) as a dvec"""
    d = cs.dvec(B)
    out = F.solve(d, **kw)
    return out if isinstance(out, cs.dvec) else d


def _host_rule(s, gb, X, k, trans):
    U, V = (X, gb) if trans else (gb, X)
    return _csx.pattern_outer_host(s.n, s.n, s.p, s.i, U, V, k, -1.0, s.sym)


@pytest.mark.parametrize("name", WIRING)
def test_wiring_blocks(cs, name):
    s = GT.BY_NAME[name]
    F = s.factor(cs)
    B, GX = s.blocks()
    for trans in s.directions:
        kw = {} if s.sym else {"trans": trans}
        adj = {} if s.sym else {"trans": not trans}
        dX, dG = _solved(cs, F, B, **kw), cs.dvec(GX)
        gb, gA = F.solve_grad(dX, dG, **kw)
        assert isinstance(gb, cs.dvec) and (gb.n, gb.k) == (s.n, GT.K) and isinstance(gA, cs.dvec) and gA.n * gA.k == len(s.i)
        assert dG.numpy().tobytes() == GX.tobytes() and gb is not dG                     # gx is not modified
        assert gb.numpy().tobytes() == _solved(cs, F, GX, **adj).numpy().tobytes()
        assert gA.numpy().tobytes() == _host_rule(s, gb.numpy(), dX.numpy(), GT.K, trans).tobytes()
        assert np.abs(gA.numpy()).max() > 0
        # host blocks in: the same gradient out (dvec blocks, the order of a solve of a host block)
        gb2, gA2 = F.solve_grad(dX.numpy(), GX, **kw)
        assert isinstance(gb2, cs.dvec) and isinstance(gA2, cs.dvec)
        assert gA2.numpy().tobytes() == _host_rule(s, gb2.numpy(), dX.numpy(), GT.K, trans).tobytes()


@pytest.mark.parametrize("name", WIRING)
def test_wiring_one_host_vector(cs, name):
    s = GT.BY_NAME[name]
    F = s.factor(cs)
    B, GX = s.blocks()
    for trans in s.directions:
        kw = {} if s.sym else {"trans": trans}
        adj = {} if s.sym else {"trans": not trans}
        x = B[:, 0].tolist()
        assert F.solve(x, **kw) is True
        gx = GX[:, 1].copy()
        gb, gA = F.solve_grad(np.asarray(x), gx, **kw)
        assert isinstance(gb, np.ndarray) and gb.shape == (s.n,) and isinstance(gA, np.ndarray) and gA.shape == (len(s.i),)
        assert gx.tobytes() == GX[:, 1].tobytes()
        lam = GX[:, 1].tolist()
        assert F.solve(lam, **adj) is True
        assert gb.tobytes() == np.asarray(lam).tobytes()
        assert gA.tobytes() == _host_rule(s, gb, np.asarray(x), 1, trans).tobytes()
        gbl, gAl = F.solve_grad(x, gx.tolist(), **kw)                                   # lists are host vectors too
        assert gbl.tobytes() == gb.tobytes() and gAl.tobytes() == gA.tobytes()


EXACT_SOLVERS = {
    "lusol_factor": ("lower", lambda cs, A: cs.lusol_factor(A, 0, 1.0)),
    "btf_factor": ("lower", lambda cs, A: cs.btf_factor(A, 1.0)),
    "slusol_factor": ("lower", lambda cs, A: cs.slusol_factor(A, 0)),
    "cholsol_factor": ("chol", lambda cs, A: cs.cholsol_factor(A, 0)),
    "ldlsol_factor": ("ldl", lambda cs, A: cs.ldlsol_factor(A, 0)),
}


@pytest.mark.parametrize("block", (True, False), ids=("block", "lists"))
@pytest.mark.parametrize("solver", sorted(EXACT_SOLVERS))
def test_exact_fixture_equals_the_rational_gradient(cs, solver, block):
    which, factor = EXACT_SOLVERS[solver]
    fx = OC.EXACT[which]
    F = factor(cs, fx.matrix(cs))
    assert F is not None
    col = fx.cols
    for trans in ((False,) if fx.sym else (False, True)):
        kw = {} if fx.sym else {"trans": trans}
        Xr, lr, gr = (OC.as_floats(v) for v in fx.rational(trans))
        if block:
            dX = _solved(cs, F, fx.B, **kw)
            gb, gA = F.solve_grad(dX, cs.dvec(fx.GX), **kw)
            X, gb, gA = dX.numpy(), gb.numpy(), gA.numpy().reshape(-1)
        else:                                   # column by column, as lists: the order of a solve of a list
            X, gb = np.empty_like(Xr), np.empty_like(lr)
            gA = np.zeros(len(fx.i))
            for c in range(OC.EXACT_K):
                x = fx.B[:, c].tolist()
                assert F.solve(x, **kw) is True
                X[:, c] = x
                gb[:, c], g1 = F.solve_grad(x, fx.GX[:, c], **kw)
                gA = gA + g1                    # exact: every partial sum is a dyadic rational of a few bits
        assert np.array_equal(X, Xr), (solver, trans)
        assert np.array_equal(gb, lr), (solver, trans)
        assert np.array_equal(gA, gr), (solver, trans)
        assert np.abs(gA).max() > 0
        if fx.sym and block:
            low = fx.i > col
            assert low.any() and gA[low].tobytes() == np.zeros(int(low.sum())).tobytes()


@pytest.mark.parametrize("name", GT.NAMES)
def test_real_matrices_against_numpy(cs, name):
    s = GT.BY_NAME[name]
    for trans in s.directions:
        gA, cond = GT.device_gradient(cs, s, trans)
        units = GT.eps_units(s, trans, gA, cond)
        print(name, "trans" if trans else "plain", "condest %.3e" % cond, "eps units %.4g" % units, "bound", GT.GRAD_EPS_UNITS)
        assert units <= GT.GRAD_EPS_UNITS, (name, trans, units)


@pytest.mark.parametrize("which", ["lusol", "btf"])
@pytest.mark.parametrize("trans", [False, True])
def test_refine_lowers_the_adjoints_backward_error_and_changes_gA(cs, which, trans):
    n, Ap, Ai, Ax, Ax2, B = RC.stale_pivot(RC.SEEDS[0])
    A = cs.cs_spalloc(n, n, len(Ai), True, False)
    A.p, A.i, A.x = Ap.tolist(), Ai.tolist(), Ax.tolist()
    F = cs.lusol_factor(cs.cs_pin(A), 0, 1.0) if which == "lusol" else cs.btf_factor(cs.cs_pin(A), 1.0)
    assert F.refactor(Ax2) is True
    GX = np.random.default_rng(5).uniform(-1.0, 1.0, (n, RC.K))
    dX = cs.dvec(B)
    F.refine(dX, trans=trans)
    gb0, gA0 = F.solve_grad(dX, cs.dvec(GX), trans=trans)
    gb2, gA2 = F.solve_grad(dX, cs.dvec(GX), trans=trans, refine=2)
    w0 = F.backward_error(gb0, cs.dvec(GX), trans=not trans)
    w2 = F.backward_error(gb2, cs.dvec(GX), trans=not trans)
    print(which, trans, "adjoint omega / eps: plain", w0 / RC.EPS, "refine=2", w2 / RC.EPS)
    assert (w2 < w0).all()
    assert gA2.numpy().tobytes() != gA0.numpy().tobytes()
    again = cs.dvec(GX)
    F.refine(again, maxit=2, trans=not trans)
    assert gb2.numpy().tobytes() == again.numpy().tobytes()
    U, V = (dX.numpy(), gb2.numpy()) if trans else (gb2.numpy(), dX.numpy())
    assert gA2.numpy().tobytes() == _csx.pattern_outer_host(n, n, Ap, Ai, U, V, RC.K, -1.0, False).tobytes()
    assert len(gA2.numpy()) == len(Ai)                                                  # on the pattern of the factored matrix


def test_symmetric_operator_rule(cs):
    s = GT.BY_NAME["chol-bcsstk01"]
    A = s.matrix(cs)
    F = cs.cholsol_factor(A, 0)
    B, GX = s.blocks()
    dX = _solved(cs, F, B)
    F.solve_grad(dX, cs.dvec(GX))
    C = cs.cs_spalloc(s.n, 1, 1, True, False)
    C.p, C.i, C.x = [0, 1], [s.n - 1], [0.5]
    assert F.update(C) is True
    with pytest.raises(RuntimeError):
        F.solve_grad(dX, cs.dvec(GX))
    # A= names the matrix the factor stands for now; only its pattern is read
    P = cs.cs_spalloc(s.n, s.n, len(s.i), False, False)
    P.p, P.i = s.p.tolist(), s.i.tolist()
    dX = _solved(cs, F, B)
    gb, gA = F.solve_grad(dX, cs.dvec(GX), A=P)
    assert gb.numpy().tobytes() == _solved(cs, F, GX).numpy().tobytes()
    assert gA.numpy().tobytes() == _host_rule(s, gb.numpy(), dX.numpy(), GT.K, False).tobytes()
    with pytest.raises(ValueError):
        F.solve_grad(dX, cs.dvec(GX), A=C)
    # refine > 0 measures against A=, which then needs values
    with pytest.raises(TypeError):
        F.solve_grad(dX, cs.dvec(GX), refine=1, A=P)


def test_argument_checks(cs):
    s = GT.BY_NAME["stale-pivot-lusol"]
    F = s.factor(cs)
    B, GX = s.blocks()
    dX = _solved(cs, F, B)
    with pytest.raises(ValueError):
        F.solve_grad(dX, cs.dvec(GX[:, :2]))
    with pytest.raises(ValueError):
        F.solve_grad(dX.numpy(), GX[:, 0])
    with pytest.raises(IndexError):
        F.solve_grad(dX, cs.dvec(GX[:-1]))
    with pytest.raises(IndexError):
        F.solve_grad(dX.numpy()[:-1], GX)
    c = HC.BY_NAME["three-by-one"]
    Q = cs.hqrsol_factor(c.matrix(cs), c.order)
    with pytest.raises(ValueError):
        Q.solve_grad(np.ones(1), np.ones(1))
    c = HC.BY_NAME["ash219"]
    Q = cs.hqrsol_factor(c.matrix(cs), c.order)
    with pytest.raises(ValueError):
        Q.solve_grad(np.ones(c.n), np.ones(c.n))
