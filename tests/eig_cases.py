"""The cases of the csx_bgs_* kernels and the pencils of eigsh() -- TEST INFRASTRUCTURE, NOT PRODUCT.

Kernel cases are a sparse cross-section of rows x (b, q) x nv, every edge of each taken once with the others small, so that the
GPU file runs in seconds: the rows sit on the edges of the ordered sum's tree (GS_CHUNK, GS_CHUNK GS_FAN, a third level) and of
the launches (more row tiles, more leaves than the grid holds), the widths on the thread tiles of csx_bgs_gram (1, 2 and 4, full
and ragged) and nv on the edges of its register group.  The pencils are small enough for dense numpy references."""
import numpy as np

import _csx

LIMITS = _csx.bgs_limits()
CHUNK, FAN, MAXW, GROUP = LIMITS["GS_CHUNK"], LIMITS["GS_FAN"], LIMITS["BGS_MAXW"], LIMITS["BGS_GROUP"]
ROWS = (1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK * FAN - 1, CHUNK * FAN, CHUNK * FAN + 1, CHUNK * FAN * FAN + 1)
WIDTHS = ((1, 1), (2, 3), (3, 2), (8, 8), (9, 7), (MAXW, MAXW), (MAXW, 1))
NVS = (1, 2, GROUP - 1, GROUP, GROUP + 1)


class KernelCase(object):
    def __init__(self, name, rows, b, q, nv, seed, special=None):
        self.name, self.rows, self.b, self.q, self.nv, self.seed, self.special = name, rows, b, q, nv, seed, special

    def data(self):
        """V (nv, rows, b), W (rows, q), H (nv, b, q)"""
        rng = np.random.default_rng(self.seed)
        V = rng.standard_normal((self.nv, self.rows, self.b))
        W = rng.standard_normal((self.rows, self.q))
        H = rng.standard_normal((self.nv, self.b, self.q))
        if self.special == "nan":
            W[:, 1] = np.nan                               # a NaN column of W
        if self.special == "inf":
            V[0, self.rows // 2, 2] = np.inf               # an Inf in column 2 of the first basis block
        return V, W, H


def _kernel_cases():
    out, seed = [], 100
    for rows in ROWS:
        out.append(KernelCase("rows%d" % rows, rows, 8, 8, 2, seed))
    for b, q in WIDTHS:
        out.append(KernelCase("w%dx%d" % (b, q), 2 * CHUNK + 1, b, q, 2, seed + 1))
    for nv in NVS:
        out.append(KernelCase("nv%d" % nv, CHUNK + 1, 9, 7, nv, seed + 2))
    # the thread tiles of the gram kernel: 2 x 2 ragged (17 x 15 at a group of 3), 4 x 4 ragged and full, with a second group
    out.append(KernelCase("tile2-ragged", CHUNK + 1, 17, 15, GROUP - 1, seed + 3))
    out.append(KernelCase("tile4-ragged", CHUNK + 1, 17, 15, GROUP + 1, seed + 4))
    out.append(KernelCase("tile4-full", CHUNK * FAN + 1, MAXW, MAXW, GROUP + 1, seed + 5))
    # more row tiles than update / combine launch workgroups (2048 on 256 CUs), more leaves than gram does (1024)
    out.append(KernelCase("many-tiles", CHUNK * FAN * FAN + 1, MAXW, MAXW, 1, seed + 6))
    out.append(KernelCase("many-leaves", CHUNK * 1025 + 1, 1, 1, 1, seed + 7))
    out.append(KernelCase("nan-column", CHUNK + 44, 8, 8, 2, seed + 8, special="nan"))
    out.append(KernelCase("inf-entry", CHUNK + 44, 8, 8, 2, seed + 9, special="inf"))
    return out


KERNEL_CASES = _kernel_cases()
KERNEL_BY_NAME = {c.name: c for c in KERNEL_CASES}
KERNEL_NAMES = [c.name for c in KERNEL_CASES]


# ---- the pencils ------------------------------------------------------------------------------------------------------------------------

def grid_laplacian(nx, ny):
    """the 5-point Laplacian of an nx x ny grid, dense: 4 on the diagonal, -1 between neighbours; its spectrum lies in (0, 8)"""
    n = nx * ny
    K = np.zeros((n, n))
    for x in range(nx):
        for y in range(ny):
            i = x * ny + y
            K[i, i] = 4.0
            if y + 1 < ny:
                K[i, i + 1] = K[i + 1, i] = -1.0
            if x + 1 < nx:
                K[i, i + ny] = K[i + ny, i] = -1.0
    return K


def tridiagonal_mass(n, seed):
    """a random SPD tridiagonal matrix, dense: diagonal in [1, 2), off-diagonal in [0, 0.25) -- diagonally dominant"""
    rng = np.random.default_rng(seed)
    M = np.diag(1.0 + rng.random(n))
    off = 0.25 * rng.random(n - 1)
    M[np.arange(n - 1), np.arange(1, n)] = off
    M[np.arange(1, n), np.arange(n - 1)] = off
    return M


def upper_csc(cs, D):
    """the upper triangle of the dense symmetric D as a `cs` of the module cs"""
    n = D.shape[0]
    p, i, x = [0], [], []
    for c in range(n):
        rows = np.flatnonzero(D[:c + 1, c])
        i.extend(int(r) for r in rows)
        x.extend(float(D[r, c]) for r in rows)
        p.append(len(i))
    A = cs.cs_spalloc(n, n, max(len(i), 1), True, False)
    A.p, A.i, A.x = p, i, x
    return A


class Pencil(object):
    """K x = lambda M x on a grid, the shift sigma, and what the tests ask of it: nev pairs with blocks of `block`"""

    def __init__(self, name, nx, ny, mass, sigma, nev, block=8):
        self.name, self.nx, self.ny, self.mass, self.sigma, self.nev, self.block = name, nx, ny, mass, sigma, nev, block
        self.n = nx * ny
        self._ref = None

    def K(self):
        return grid_laplacian(self.nx, self.ny)

    def M(self):
        return tridiagonal_mass(self.n, 7) if self.mass else None

    def A(self):
        M = self.M()
        return self.K() - self.sigma * (M if M is not None else np.eye(self.n))

    def reference(self):
        """(all eigenvalues of the pencil ascending, cond_2(M)), by numpy.linalg.eigh of the Cholesky-reduced dense pencil;
        computed once"""
        if self._ref is None:
            K, M = self.K(), self.M()
            if M is None:
                lam, cond = np.linalg.eigvalsh(K), 1.0
            else:
                L = np.linalg.cholesky(M)
                Li = np.linalg.inv(L)
                C = Li @ K @ Li.T
                lam, cond = np.linalg.eigvalsh((C + C.T) / 2.0), float(np.linalg.cond(M))
            self._ref = (lam, cond)
        return self._ref

    def nearest(self):
        """the nev reference eigenvalues nearest sigma, by ascending distance"""
        lam = self.reference()[0]
        return lam[np.argsort(np.abs(lam - self.sigma), kind="stable")[:self.nev]]

    def below(self):
        return int((self.reference()[0] < self.sigma).sum())


PENCILS = [Pencil("grid17x13-mass-3.7", 17, 13, True, 3.7, 8), Pencil("grid17x13-mass-0", 17, 13, True, 0.0, 8),
           Pencil("grid12x12-3.7", 12, 12, False, 3.7, 6), Pencil("grid40x37-mass-3.7", 40, 37, True, 3.7, 8)]
PENCIL_BY_NAME = {p.name: p for p in PENCILS}
PENCIL_NAMES = [p.name for p in PENCILS]
TOL = 2.0 ** -30
MAX_BLOCKS = 24          # the condition of the issue: about twice what the prototype took at 1e-8


def dense_callables(p):
    """solve, product, residual of the restated loop on dense numpy: the operator is A = K - sigma M"""
    A, M = p.A(), p.M()
    absA = np.abs(A)

    def solve(B):
        return np.linalg.solve(A, B)

    def product(X):
        return -(M @ X)

    def residual(X, B):
        R = B - A @ X
        den = absA @ np.abs(X) + np.abs(B)
        with np.errstate(all="ignore"):
            w = np.where(R == 0.0, 0.0, np.abs(R) / den).max(axis=0)
        return R, w

    return solve, (product if M is not None else None), residual


def breakdown_pencil():
    """a block-diagonal matrix of order 24 (three blocks of 8) and the first eight unit vectors: the starting block spans an
    invariant subspace, and every operation on it is exact where the other blocks are zero, so the first expansion is exactly 0"""
    rng = np.random.default_rng(5)
    A = np.zeros((24, 24))
    for k in range(3):
        B = rng.standard_normal((8, 8))
        A[8 * k:8 * k + 8, 8 * k:8 * k + 8] = B @ B.T + 8.0 * np.eye(8)
    return A, np.eye(24)[:, :8].copy()
