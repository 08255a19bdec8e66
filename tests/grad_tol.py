"""The bound of solve_grad() against numpy on real matrices, and the systems it is measured on -- TEST
INFRASTRUCTURE, NOT PRODUCT.

The reference of gA is -(Aop^-T GX) X' sampled on the pattern, with X = Aop^-1 B and both solves by numpy's dense float64 solve
(LAPACK, partial pivoting) -- never this code's earlier output.  The error of an entry is taken in units of

    2^-52 * condest() * s_ij,    s_ij = (|Lambda| |X|')[i, j]   (sym mode, i < j: s_ij + s_ji; below the diagonal gA is +0.0)

with Lambda, X the reference's and condest() the solver's own 1-norm estimate: gA is a product of two solutions of systems with
A, each of which moves by about cond(A) roundings of itself, so the unit is one rounding of the entry's terms times the
conditioning.  GRAD_EPS_UNITS is 8 x the largest figure tools/measure_solve_grad.py measured over SYSTEMS on an MI355X
(profiles/solve_grad_edges.jsonl has every system): tests/tol.py's convention -- a maximum over a handful of systems
underestimates the tail, and the results are the same bits on every run, so the factor covers other right-hand sides and a
legitimate regrouping of a solve, not noise."""
import numpy as np

import chol_refactor_cases as CRC
import hqr_cases as HC
import ldl_cases as LC
import refine_cases as RC
import slu_cases as SC

EPS = 2.0 ** -52
GRAD_EPS_UNITS_MEASURED = 10.569145255970264       # the largest figure of profiles/solve_grad_edges.jsonl (ldl-grid24-shift)
GRAD_EPS_UNITS = 8 * GRAD_EPS_UNITS_MEASURED
K = 3


class System(object):
    """name; solver (the factor call's name); n, p, i, x; sym; factor(cs) -> the solver; directions: the trans values"""

    def __init__(self, name, solver, n, p, i, x, factor, sym=False, seed=0):
        self.name, self.solver, self.n, self.sym, self.factor, self.seed = name, solver, int(n), sym, factor, seed
        self.p, self.i, self.x = np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64)
        self.cols = np.repeat(np.arange(self.n), np.diff(self.p))
        self.directions = (False,) if sym else (False, True)
        assert len(set(zip(self.i.tolist(), self.cols.tolist()))) == len(self.i), "a system with duplicate entries"

    def matrix(self, mod):
        A = mod.cs_spalloc(self.n, self.n, max(len(self.i), 1), True, False)
        A.p, A.i, A.x = self.p.tolist(), self.i.tolist(), self.x.tolist()
        return A

    def dense(self):
        """the operator: the stored entries (no system here has duplicates), the upper triangle mirrored when sym"""
        D = np.zeros((self.n, self.n))
        if self.sym:
            up = self.i <= self.cols
            D[self.i[up], self.cols[up]] = self.x[up]
            return D + np.triu(D, 1).T
        D[self.i, self.cols] = self.x
        return D

    def blocks(self):
        rng = np.random.default_rng(20250100 + self.seed)
        return rng.uniform(-1.0, 1.0, (self.n, K)), rng.uniform(-1.0, 1.0, (self.n, K))

    def reference(self, trans):
        """(X, Lambda, gA, scale) by numpy: X = op^-1 B, Lambda = op^-T GX, gA and the scale s of the docstring per stored entry"""
        A = self.dense()
        B, GX = self.blocks()
        X = np.linalg.solve(A.T if trans else A, B)
        lam = np.linalg.solve(A if trans else A.T, GX)
        U, V = (X, lam) if trans else (lam, X)
        i, j = self.i, self.cols
        gA = -np.einsum("qc,qc->q", U[i], V[j])
        s = np.einsum("qc,qc->q", np.abs(U[i]), np.abs(V[j]))
        if self.sym:
            off = i < j
            gA = np.where(off, gA - np.einsum("qc,qc->q", U[j], V[i]), gA)
            s = np.where(off, s + np.einsum("qc,qc->q", np.abs(U[j]), np.abs(V[i])), s)
            gA, s = np.where(i > j, 0.0, gA), np.where(i > j, 0.0, s)
        return X, lam, gA, s


def eps_units(system, trans, gA, cond):
    """the largest error of gA (device) in the docstring's units; entries of scale 0 must be equal"""
    _, _, ref, s = system.reference(trans)
    gA = np.asarray(gA, np.float64).reshape(-1)
    live = s > 0.0
    assert np.array_equal(gA[~live], ref[~live])
    return float(np.max(np.abs(gA[live] - ref[live]) / (EPS * cond * s[live]))) if live.any() else 0.0


def device_gradient(cs, system, trans):
    """(gA as numpy, condest) of the product's solver on the system, X by the solver's own solve"""
    F = system.factor(cs)
    assert F is not None
    B, GX = system.blocks()
    dX = cs.dvec(B)
    if system.sym:
        F.solve(dX)
        gb, gA = F.solve_grad(dX, cs.dvec(GX))
    else:
        X = F.solve(dX, trans=trans)
        dX = X if isinstance(X, cs.dvec) else dX    # hqrsol_factor returns the solution of a dvec block
        gb, gA = F.solve_grad(dX, cs.dvec(GX), trans=trans)
    return gA.numpy().reshape(-1), float(F.condest())


def _systems():
    out = []
    n, Ap, Ai, Ax, _, _ = RC.stale_pivot(RC.SEEDS[0])
    out.append(System("stale-pivot-lusol", "lusol_factor", n, Ap, Ai, Ax, lambda cs, s=None: None, seed=1))
    out.append(System("stale-pivot-btf", "btf_factor", n, Ap, Ai, Ax, lambda cs, s=None: None, seed=2))
    out[0].factor = lambda cs, S=out[0]: cs.lusol_factor(cs.cs_pin(S.matrix(cs)), 0, 1.0)
    out[1].factor = lambda cs, S=out[1]: cs.btf_factor(cs.cs_pin(S.matrix(cs)), 1.0)
    for k, name in enumerate(("grid24-shift", "fs183", "saddle-natural")):
        c = SC.BY_NAME[name]
        out.append(System("slu-" + name, "slusol_factor", c.n, c.p, c.i, c.x,
                          lambda cs, c=c: cs.slusol_factor(c.matrix(cs), c.order, c.perturb, c.match, c.match_seed), seed=3 + k))
    for k, name in enumerate(("grid24-shift", "kkt-sqd")):
        c = LC.BY_NAME[name]
        out.append(System("ldl-" + name, "ldlsol_factor", c.n, c.p, c.i, c.x,
                          lambda cs, c=c: cs.ldlsol_factor(c.matrix(cs), c.order, c.perturb), sym=True, seed=6 + k))
    c = CRC.BY_NAME["bcsstk01-natural"]
    out.append(System("chol-bcsstk01", "cholsol_factor", c.n, c.p, c.i, c.x, lambda cs, c=c: cs.cholsol_factor(c.matrix(cs), c.order),
                      sym=True, seed=8))
    c = CRC.BY_NAME["bcsstk01-ordered"]
    out.append(System("chol-bcsstk01-ordered", "cholsol_factor", c.n, c.p, c.i, c.x,
                      lambda cs, c=c: cs.cholsol_factor(c.matrix(cs), c.order), sym=True, seed=9))
    for k, name in enumerate(("grid24-shift", "west")):
        c = HC.BY_NAME[name]
        assert c.m == c.n
        out.append(System("hqr-" + name, "hqrsol_factor", c.n, c.p, c.i, c.x, lambda cs, c=c: cs.hqrsol_factor(c.matrix(cs), c.order),
                          seed=10 + k))
    return out


SYSTEMS = _systems()
NAMES = [s.name for s in SYSTEMS]
BY_NAME = {s.name: s for s in SYSTEMS}
