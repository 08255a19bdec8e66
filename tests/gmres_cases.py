"""Shapes for the csx_gs_* kernels and the systems gmres() is tested on -- TEST INFRASTRUCTURE, NOT PRODUCT.

KERNEL_CASES: every shape sits on an edge of the ordered sum or of a kernel, taken from _csx.gmres_limits(): rows around one leaf
(GS_CHUNK), around one full inner node (GS_CHUNK GS_FAN) and one row past two full levels; widths around a wave and around the
16-byte pairs (even / odd); basis sizes around the register group (GS_GROUP) and 17 (restart 16); the three masks; a NaN and an
Inf column.  Values are full-mantissa doubles of mixed sign and scale, so byte equality says the order of every sum is right.

SYSTEMS: (a) the stale Cholesky factor of the 24 x 24 grid Laplacian K against K + sigma sum e_i e_i' on committed nodes; (b) the
permuted saddle-point matrix of slu_cases under static pivots perturbed at 1e-10 and at SADDLE_PERTURB; (c) K - 3.7 I under
LDL' with perturbed pivots; (d) an LU refactor on stale pivots; (e) a diagonal system, whose solve is already at omega <= 2^-52.
Every system brings the host model of its solver -- the host factor rule the project has, the plain-C triangular loops, the C
residual rule -- as callables solve(B) -> X and residual(X, B) -> (R, omega) for refine_cases.refine_loop and
gmres_oracle.gmres_loop, and `device(cs)`: the product's solver with the arguments of its gmres() call."""
import numpy as np

import _csx
import c_oracle as CO
import csparse_oracle as O
import ldl_cases as LC
import ldl_oracle as LO
import refactor_oracle
import refine_cases as RC
import slu_cases as SC
import slu_oracle as SO
from chol_refactor_cases import grid_upper

LIMITS = _csx.gmres_limits()
CHUNK, FAN, GROUP = LIMITS["GS_CHUNK"], LIMITS["GS_FAN"], LIMITS["GS_GROUP"]
EPS = 2.0 ** -52
MAXIT = 64                                    # gmres()'s default

ROWS = (1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * FAN - 1, CHUNK * FAN, CHUNK * FAN + 1)
TWO_LEVELS = CHUNK * FAN * FAN + 1            # one row past two full levels: reached at k = 1 with one basis vector
NOT_REACHED = ()                              # (every edge the issue lists is reached)
WIDTHS = (1, 3, 63, 64, 65, 130)
BASES = (1, 2, GROUP - 1, GROUP, GROUP + 1, 17)
MASKS = ("live", "dead", "alternating")


class KernelCase(object):
    def __init__(self, name, rows, k, nv, mask="live", special=None, seed=0):
        self.name, self.rows, self.k, self.nv, self.mask_kind, self.special = name, rows, k, nv, mask, special
        self.seed = seed

    def mask(self):
        if self.mask_kind == "live":
            return np.ones(self.k, np.int32)
        if self.mask_kind == "dead":
            return np.zeros(self.k, np.int32)
        return (np.arange(self.k) % 2 == 0).astype(np.int32)

    def data(self):
        """(V (nv + 1 blocks: the last is the slot csx_gs_scale writes), W, h, s, y, length)"""
        rng = np.random.default_rng(20241000 + self.seed)

        def values(*shape):
            return rng.standard_normal(shape) * 2.0 ** rng.integers(-12, 13, shape)

        V, W = values(self.nv + 1, self.rows, self.k), values(self.rows, self.k)
        if self.special is not None:
            W[self.rows // 2, 1] = self.special
            V[0, self.rows // 3, 2] = self.special
        h, s, y = values(self.nv, self.k), values(self.k), values(self.nv, self.k)
        length = rng.integers(0, self.nv + 1, self.k).astype(np.int32)
        length[0] = self.nv
        return V, W, h, s, y, length


def _kernel_cases():
    out, seed = [], 0

    def add(name, *a, **kw):
        nonlocal seed
        seed += 1
        out.append(KernelCase(name, *a, seed=seed, **kw))

    for rows in ROWS:
        add("rows%d" % rows, rows, 3, 2, mask="alternating")
    add("rows%d" % TWO_LEVELS, TWO_LEVELS, 1, 1)
    for k in WIDTHS:
        add("k%d" % k, CHUNK + 1, k, 2)
        add("k%d-alternating" % k, CHUNK + 1, k, 2, mask="alternating")
    for nv in BASES:
        add("nv%d" % nv, CHUNK + 1, 3, nv)
        add("nv%d-pairs" % nv, CHUNK + 1, 4, nv, mask="alternating")
    for m in MASKS:
        add("mask-" + m, CHUNK * FAN + 1, 4, 2, mask=m)
    add("nan-column", CHUNK + 1, 4, 2, special=np.nan)
    add("inf-column", CHUNK + 1, 5, 2, special=np.inf)
    return out


KERNEL_CASES = _kernel_cases()
KERNEL_BY_NAME = {c.name: c for c in KERNEL_CASES}
KERNEL_NAMES = [c.name for c in KERNEL_CASES]


# ---- the C residual rules as callables ---------------------------------------------------------------------------------------------

def residual_rule(n, p, i, x, sym=False, trans=False):
    """residual(X, B) -> (R, omega) by csx_residual_sym_host / csx_residual_host on the n x n matrix (p, i, x)"""
    lib = _csx.load()
    p, i, x = _csx.i32(p), _csx.i32(i), _csx.f64(x)

    def residual(X, B):
        X, B = _csx.f64(X), _csx.f64(B)
        k = X.shape[1]
        R, w, rn = np.empty((n, k)), np.empty(k), np.empty(k)
        if sym:
            st = lib.csx_residual_sym_host(n, _csx.pi(p), _csx.pi(i), _csx.pd(x), k, _csx.pd(X), _csx.pd(B), _csx.pd(R), _csx.pd(w),
                                           _csx.pd(rn))
        else:
            st = lib.csx_residual_host(n, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), k, 1 if trans else 0, _csx.pd(X), _csx.pd(B),
                                       _csx.pd(R), _csx.pd(w), _csx.pd(rn))
        assert st == 0
        return R, w

    return residual


def by_columns(solve_one):
    def solve(B):
        B = np.asarray(B, dtype=np.float64)
        return np.column_stack([solve_one(np.ascontiguousarray(B[:, c])) for c in range(B.shape[1])])
    return solve


def rhs(n, k, seed):
    """BASE = 3 columns uniform in [-1, 1] from a committed seed; wider blocks repeat them scaled by powers of two (exact: every
    operation of the loop scales with it, omega and the step counts do not change)"""
    base = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))
    return np.column_stack([base[:, c % 3] * 2.0 ** (c // 3) for c in range(k)])


class System(object):
    """name; n; B(k); bound (inner steps gmres may take per column, or None); solve / residual (the host model); device(cs) ->
    (solver, keyword arguments of its gmres / refine beside b), with exact= handed to the factor call where it has one"""

    def __init__(self, name, n, seed, bound, model, device, refine_accepts_none=False):
        self.name, self.n, self.seed, self.bound, self._model, self.device = name, n, seed, bound, model, device
        self.refine_accepts_none = refine_accepts_none
        self._made = None

    def B(self, k=3):
        return rhs(self.n, k, self.seed)

    def model(self):
        if self._made is None:
            self._made = self._model()
        return self._made


# ---- (a) a stale Cholesky factor -----------------------------------------------------------------------------------------------------

GRID = 24
NODES = tuple(25 * t + 30 for t in range(12))    # committed: the nodes whose diagonal entry is bumped, down the grid's diagonal


def _cs(cs, n, p, i, x):
    A = cs.cs_spalloc(n, n, max(len(i), 1), True, False)
    A.p, A.i, A.x = np.asarray(p).tolist(), np.asarray(i).tolist(), np.asarray(x, np.float64).tolist()
    return A


def bumped(r, sigma):
    """the upper triangle of K + sigma sum e_i e_i' over the first r NODES, on K's pattern"""
    n, p, i, x = grid_upper(GRID)
    x = np.asarray(x, np.float64).copy()
    cols = np.repeat(np.arange(n), np.diff(p))
    for node in NODES[:r]:
        x[(np.asarray(i) == node) & (cols == node)] += sigma
    return n, np.asarray(p, np.int32), np.asarray(i, np.int32), x


def _stale_chol(order, r, sigma):
    n, p, i, x = grid_upper(GRID)
    case = LC.Case("gmres-grid%d-order%d" % (GRID, order), n, p, i, x, order=order)
    _, ap, ai, ax = bumped(r, sigma)

    def model():
        # K is positive definite: its L D L' host factor stands in for the Cholesky factor of the device (the same matrix,
        # factored to rounding; what is tested is the iteration, which the gap between K and A decides)
        st, Lx, d, info = LO.host(case, case.x, 0.0)
        assert st == 0 and info[1] == 0 and info[3] == -1
        Lp, Li, _ = LO.pattern_of(case)
        pinv = LO.pinv_of(case)

        def one(b):
            y = b.copy()
            if pinv is not None:
                y = np.empty(n)
                y[pinv] = b
            y = CO.ltsolve(n, Lp, Li, Lx, CO.lsolve(n, Lp, Li, Lx, y) / d)
            return y if pinv is None else y[pinv]

        return by_columns(one), residual_rule(n, ap, ai, ax, sym=True)

    def device(cs, exact=None):
        return cs.cholsol_factor(_cs(cs, n, p, i, x), order, exact), {"A": cs.cs_pin(_cs(cs, n, ap, ai, ax))}

    return System("chol-order%d-r%d-sigma%g" % (order, r, sigma), n, 20241001 + r, 2 * (r + 1), model, device,
                  refine_accepts_none=True)


# ---- (b) static pivots, perturbed ------------------------------------------------------------------------------------------------------

SADDLE_PERTURB = 1e-6     # chosen on the CPU: the model of refine() does not reach 2^-52 in five steps (tests/test_gmres_cpu.py)


def _saddle(perturb):
    case = SC.BY_NAME["saddle"]
    made = {}

    def factor():
        if not made:
            st, Lx, Ux, info = SO.host(case, case.x, SO.tau_of(case, case.x, perturb))
            assert st == 0 and info[3] == -1
            made["f"] = (Lx, Ux, info)
        return made["f"]

    def model():
        Lx, Ux, _ = factor()
        return by_columns(lambda b: SO.solve(case, Lx, Ux, b)), residual_rule(case.n, case.p, case.i, case.x)

    def device(cs, exact=None):
        return cs.slusol_factor(case.matrix(cs), case.order, perturb, case.match, case.match_seed, exact), {}

    s = System("saddle-perturb%g" % perturb, case.n, 20241020, lambda: 2 * (factor()[2][2] + 1), model, device)
    s.perturbed = lambda: factor()[2][2]
    return s


# ---- (c) L D L' with perturbed pivots ----------------------------------------------------------------------------------------------------

LDL_PERTURB = 1e-2        # of |S|_1: large enough that pivots of K - 3.7 I on the 24 x 24 grid are perturbed (counted on the CPU)


def _ldl_shift():
    case = LC.BY_NAME["grid24-shift"]
    made = {}

    def factor():
        if not made:
            st, Lx, d, info = LO.host(case, case.x, LO.tau_of(case, case.x, LDL_PERTURB))
            assert st == 0 and info[3] == -1
            made["f"] = (Lx, d, info)
        return made["f"]

    def model():
        Lx, d, _ = factor()
        Lp, Li, _ = LO.pattern_of(case)
        pinv, n = LO.pinv_of(case), case.n

        def one(b):
            y = b.copy()
            if pinv is not None:
                y = np.empty(n)
                y[pinv] = b
            y = CO.ltsolve(n, Lp, Li, Lx, CO.lsolve(n, Lp, Li, Lx, y) / d)
            return y if pinv is None else y[pinv]

        return by_columns(one), residual_rule(n, case.p, case.i, case.x, sym=True)

    def device(cs, exact=None):
        return cs.ldlsol_factor(case.matrix(cs), case.order, LDL_PERTURB, exact), {}

    s = System("ldl-grid24-shift-perturbed", case.n, 20241030, MAXIT, model, device)
    s.perturbed = lambda: factor()[2][2]
    return s


# ---- (d) an LU refactor on stale pivots ----------------------------------------------------------------------------------------------------

STALE_PIVOT = 1e-13       # the first diagonal entry of every block of the new values: refine_cases has 1e-6, which refinement mends


def stale_values(seed=RC.SEEDS[0]):
    """refine_cases.stale_pivot with the stale pivots at STALE_PIVOT: (n, Ap, Ai, Ax, Ax2)"""
    n, Ap, Ai, Ax, Ax2, _ = RC.stale_pivot(seed)
    Ax2 = Ax2.copy()
    cols = np.repeat(np.arange(n), np.diff(Ap))
    first = np.flatnonzero((Ai == cols) & (np.abs(Ax2) < 2e-6))
    Ax2[first] *= STALE_PIVOT / 1e-6
    return n, Ap, Ai, Ax, Ax2


def _stale_lu(which, trans):
    n, Ap, Ai, Ax, Ax2 = stale_values()

    def model():
        A = O.cs_spalloc(n, n, len(Ai), True, False)
        A.p, A.i, A.x = Ap.tolist(), Ai.tolist(), Ax.tolist()
        N = O.cs_lu(A, O.cs_sqr(0, A, False), 1.0)
        assert N is not None and list(N.pinv) == list(range(n))
        Lx, Ux, ok, _ = refactor_oracle.refactor(N.L, N.U, N.pinv, (Ap, Ai, Ax2))
        assert ok
        Lp, Li = np.asarray(N.L.p, np.int32), np.asarray(N.L.i[:N.L.p[n]], np.int32)
        Up, Ui = np.asarray(N.U.p, np.int32), np.asarray(N.U.i[:N.U.p[n]], np.int32)
        Lx, Ux = np.asarray(Lx), np.asarray(Ux)

        def one(b):
            if trans:
                return CO.pvec(N.pinv, CO.ltsolve(n, Lp, Li, Lx, CO.utsolve(n, Up, Ui, Ux, b)))
            return CO.usolve(n, Up, Ui, Ux, CO.lsolve(n, Lp, Li, Lx, CO.ipvec(N.pinv, b)))

        return by_columns(one), residual_rule(n, Ap, Ai, Ax2, trans=trans)

    def device(cs, exact=None):
        A = cs.cs_pin(_cs(cs, n, Ap, Ai, Ax))
        F = cs.lusol_factor(A, 0, 1.0, exact) if which == "lusol" else cs.btf_factor(A, 1.0)
        assert F is not None and F.refactor(Ax2) is True
        return F, {"trans": trans}

    return System("stale-%s%s" % (which, "-trans" if trans else ""), n, 20241040, MAXIT, model, device)


# ---- (e) nothing to do ----------------------------------------------------------------------------------------------------------------------

def _diagonal():
    case = SC.BY_NAME["diagonal"]

    def model():
        d = case.x.copy()
        return by_columns(lambda b: b / d), residual_rule(case.n, case.p, case.i, case.x)

    def device(cs, exact=None):
        return cs.lusol_factor(case.matrix(cs), 0, 1.0, exact), {}

    return System("diagonal", case.n, 20241050, 0, model, device)


CHOL = [_stale_chol(order, r, 50.0) for order in (0, 1) for r in (1, 5, 12)] + [_stale_chol(order, 5, 3.0) for order in (0, 1)]
SADDLE = [_saddle(1e-10), _saddle(SADDLE_PERTURB)]
# at 1e-5 column REFUSED_COLUMN of the model ends two cycles just above 2^-52 and its third cycle does not lower omega: the one
# fixture found whose cycle the acceptance rule refuses (tests/test_gmres_cpu.py shows it)
REFUSED, REFUSED_COLUMN = _saddle(1e-5), 1
LDL = [_ldl_shift()]
STALE = [_stale_lu(which, trans) for which in ("lusol", "btf") for trans in (False, True)]
DIAGONAL = _diagonal()
SYSTEMS = CHOL + SADDLE + LDL + STALE
BY_NAME = {s.name: s for s in SYSTEMS + [DIAGONAL]}
NAMES = [s.name for s in SYSTEMS]


def bound(system):
    """inner steps per column gmres() may take on the system: (a) 2 (r + 1); (b) 2 (perturbed pivots + 1), counted by the host
    factor rule; (c), (d) the default maxit"""
    return system.bound() if callable(system.bound) else system.bound
