"""csparse -- drop-in for rwl/CSparse.py's sparse-direct hot path on AMD MI355X.

Same names, same positional signatures, same `cs` objects (CSC: p, i, x; nz ==
-1) and the same error conventions as the reference module
(/root/reference/csparse.py, cited as csparse.py:N): bad arguments give False /
None / -1, a zero pivot in a triangular solve raises ZeroDivisionError, vectors
are updated in place, matrix results are new `cs` objects.

What runs where
  * The loops of the hot path -- cs_gaxpy, cs_transpose, cs_multiply,
    cs_lsolve / cs_ltsolve / cs_usolve / cs_utsolve, the numeric part of cs_chol,
    and the permute/solve sequence of cs_cholsol / cs_lusol -- run as hand-written
    HIP kernels (gfx950) behind the C ABI of libcsx.so (include/csx.h), reached
    through ctypes (_csx.py).  There is no CPU fallback: without the library or a
    GPU these functions raise.
  * List-based calls behave exactly like the reference: inputs are uploaded,
    the result is written back into the caller's list.  For these calls the
    kernels keep the reference's order of floating-point operations, so y / x
    come back bit-identical.
  * Large problems stay on the device: `cs_pin(A)` keeps a matrix resident (and
    caches its analysis), `dvec` is a device-resident vector / n-by-k block that
    every function here accepts in place of a list, and results of
    cs_transpose / cs_multiply on pinned inputs are device-backed `cs` objects
    whose p / i / x are only copied to the host when read.
  * Host-side glue that the reference also does in Python (triplet assembly,
    cs_cumsum, cs_scatter on lists, permutation of a single list) stays Python.
"""
import contextlib
import math
import os
import time
import weakref
from math import sqrt

import numpy as np

import _csx
from _hostglue import (CS_FLIP, CS_MARK, CS_MARKED, CS_UNFLIP, cs_dfs, cs_ereach, cs_reach,  # noqa: F401
                       cs_spsolve)
from _csx import (GAXPY_ATOMIC, GAXPY_AUTO, GAXPY_EXACT, GAXPY_TILED,  # noqa: F401
                  GAXPY_WAVE, TRI_L, TRI_LT, TRI_U, TRI_UT)

CS_VER = 1
CS_SUBVER = 0
CS_SUBSUB = 0
CS_DATE = "May 14, 2012"
CS_COPYRIGHT = "Copyright (C) Timothy A. Davis, 2006-2011"


# --------------------------------------------------------------- containers --

class _DevMatrix(object):
    """Owner of a libcsx CSC handle (+ cached triangular-solve plans)."""

    def __init__(self, handle):
        self.handle = handle
        self.plans = {}
        self.version = 0      # bumped when the values change in place (cs_updown): solvers built on it re-plan
        self._fin = weakref.finalize(self, _DevMatrix._release, handle, self.plans)

    @staticmethod
    def _release(handle, plans):
        for h in plans.values():
            _csx.free(h)
        _csx.free(handle)

    def info(self):
        m, n, nnz, hv = (_csx.C.c_int32(), _csx.C.c_int32(), _csx.C.c_int32(), _csx.C.c_int())
        _csx.check(_csx.lib().csx_csc_info(self.handle, m, n, nnz, hv), "csx_csc_info")
        return m.value, n.value, nnz.value, bool(hv.value)


class cs(object):
    """Matrix in compressed-column or triplet form (csparse.py:37-54).

    p, i, x behave as plain attributes.  A matrix produced on the device keeps
    them there until they are first read."""

    def __init__(self):
        self.nzmax = 0
        self.m = 0
        self.n = 0
        self._p = []
        self._i = []
        self._x = []
        self.nz = 0
        self._dev = None       # _DevMatrix when a device copy exists
        self._lazy = False     # True: host lists not materialised yet
        self._pinned = False
        self._implicit = False  # device-resident because an operation produced it there, not because of cs_pin

    def _materialise(self):
        if self._lazy:
            m, n, nnz, hv = self._dev.info()
            p = np.empty(n + 1, dtype=np.int32)
            i = np.empty(max(nnz, 1), dtype=np.int32)
            x = np.empty(max(nnz, 1), dtype=np.float64) if hv else None
            _csx.check(_csx.lib().csx_csc_download(self._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)),
                       "csx_csc_download")
            keep = self.nzmax
            self._p = p.tolist()
            self._i = i[:nnz].tolist() + [0] * (keep - nnz)
            self._x = None if x is None else x[:nnz].tolist() + [0.0] * (keep - nnz)
            self._lazy = False
            if self._implicit:
                # The caller now holds plain lists and may edit them in place (C.x[k] = v, the reference's
                # idiom), which nothing here can observe: the host lists become the only copy.  cs_pin(C)
                # keeps a result resident on purpose (and then cs_invalidate applies).
                self._dev = None
                self._pinned = False
                self._implicit = False

    def _touch(self):
        # host data assigned: a non-pinned device copy is stale
        if self._dev is not None and not self._lazy:
            self._dev = None
            self._pinned = False

    @property
    def p(self):
        self._materialise()
        return self._p

    @p.setter
    def p(self, v):
        self._materialise()
        self._p = v
        self._touch()

    @property
    def i(self):
        self._materialise()
        return self._i

    @i.setter
    def i(self, v):
        self._materialise()
        self._i = v
        self._touch()

    @property
    def x(self):
        self._materialise()
        return self._x

    @x.setter
    def x(self, v):
        self._materialise()
        self._x = v
        self._touch()


class css(object):
    """Symbolic Cholesky / LU / QR analysis (csparse.py:57-76)."""

    def __init__(self):
        self.pinv = []
        self.q = []
        self.parent = []
        self.cp = []
        self.leftmost = []
        self.m2 = 0
        self.lnz = 0
        self.unz = 0


class csn(object):
    """Numeric Cholesky / LU / QR factorisation (csparse.py:79-90)."""

    def __init__(self):
        self.L = None
        self.U = None
        self.pinv = []
        self.B = []


class dvec(object):
    """Device-resident float64 vector (k == 1) or n-by-k row-major block.

    dvec(data)            upload a sequence / numpy array (2-D arrays keep their shape)
    dvec(n, k=1)          zeros
    Accepted wherever the reference takes a list x / y / b."""

    def __init__(self, data, k=None, _handle=None):
        if _handle is not None:
            self.handle, self.n, self.k = _handle, int(data), int(k or 1)
        elif isinstance(data, (int, np.integer)):
            self.n, self.k = int(data), int(k or 1)
            h = _csx.new_handle()
            _csx.check(_csx.lib().csx_vec_alloc(self.n * self.k, h), "csx_vec_alloc")
            self.handle = h
        else:
            a = _csx.f64(data)
            self.n = a.shape[0]
            self.k = 1 if a.ndim == 1 else int(np.prod(a.shape[1:]))
            h = _csx.new_handle()
            _csx.check(_csx.lib().csx_vec_upload(_csx.pd(a), a.size, h), "csx_vec_upload")
            self.handle = h
        self._fin = weakref.finalize(self, _csx.free, self.handle)

    def __len__(self):
        return self.n

    def numpy(self):
        out = np.empty(self.n * self.k, dtype=np.float64)
        _csx.check(_csx.lib().csx_vec_download(self.handle, _csx.pd(out), out.size), "csx_vec_download")
        return out if self.k == 1 else out.reshape(self.n, self.k)

    def tolist(self):
        return self.numpy().tolist()

    def assign(self, data):
        a = _csx.f64(data)
        _csx.check(_csx.lib().csx_vec_write(self.handle, _csx.pd(a), a.size), "csx_vec_write")

    def fill(self, value):
        _csx.check(_csx.lib().csx_vec_fill(self.handle, float(value)), "csx_vec_fill")

    def copy(self):
        out = dvec(self.n, self.k)
        _csx.check(_csx.lib().csx_vec_copy(self.handle, out.handle), "csx_vec_copy")
        return out

    def device_ptr(self):
        p = _csx.C.c_void_p()
        ln = _csx.C.c_int64()
        _csx.check(_csx.lib().csx_vec_ptr(self.handle, p, ln), "csx_vec_ptr")
        return p.value


# ------------------------------------------------------- predicates, alloc --

def CS_CSC(A):
    """True if A is compressed-column (csparse.py:113-119)."""
    return A is not None and A.nz == -1


def CS_TRIPLET(A):
    """True if A is a triplet matrix (csparse.py:122-128)."""
    return A is not None and A.nz >= 0


def ialloc(n):
    return [0] * n


def xalloc(n):
    return [0.0] * n


def cs_spalloc(m, n, nzmax, values, triplet):
    """Allocate a CSC or triplet matrix (csparse.py:2388-2406)."""
    A = cs()
    A.m = m
    A.n = n
    A.nzmax = nzmax = max(nzmax, 1)
    A.nz = 0 if triplet else -1
    A.p = ialloc(nzmax) if triplet else ialloc(n + 1)
    A.i = ialloc(nzmax)
    A.x = xalloc(nzmax) if values else None
    return A


def cs_sprealloc(A, nzmax):
    """Resize i / x (and p of a triplet); nzmax <= 0 trims (csparse.py:2414-2440)."""
    if A is None:
        return False
    if nzmax <= 0:
        nzmax = A.p[A.n] if CS_CSC(A) else A.nz
    A.i = (list(A.i) + [0] * nzmax)[:nzmax]
    if CS_TRIPLET(A):
        A.p = (list(A.p) + [0] * nzmax)[:nzmax]
    if A.x is not None:
        A.x = (list(A.x) + [0.0] * nzmax)[:nzmax]
    A.nzmax = nzmax
    return True


# ------------------------------------------- host glue (Python in the reference too) --

def cs_entry(T, i, j, x):
    """Append one triplet (csparse.py:1068-1091)."""
    if not CS_TRIPLET(T) or i < 0 or j < 0:
        return False
    if T.nz >= T.nzmax:
        cs_sprealloc(T, 2 * T.nzmax)
    if T.x is not None:
        T.x[T.nz] = x
    T.i[T.nz] = i
    T.p[T.nz] = j
    T.nz += 1
    T.m = max(T.m, i + 1)
    T.n = max(T.n, j + 1)
    return True


def cs_load(filename, base=0):
    """Read 'i j aij' lines into a triplet matrix (csparse.py:1307-1327)."""
    T = cs_spalloc(0, 0, 1, True, True)
    with open(filename, "rb") as fd:
        for line in fd:
            tok = line.split()
            if len(tok) != 3:
                return None
            if not cs_entry(T, int(tok[0]) - base, int(tok[1]) - base, float(tok[2])):
                return None
    return T


def cs_compress(T):
    """Triplet -> CSC, a stable sort by column (csparse.py:647-673), done with numpy."""
    if not CS_TRIPLET(T):
        return None
    nz = T.nz
    if T._pinned:   # cs_pin(T): sort on the device and keep the result there
        rows, cols = _csx.i32(T.i[:nz]), _csx.i32(T.p[:nz])
        vals = None if T.x is None else _csx.f64(T.x[:nz])
        h = _csx.new_handle()
        st = _csx.lib().csx_compress(T.m, T.n, nz, _csx.pi(rows), _csx.pi(cols), _csx.pd(vals), h)
        if st == _csx.EINVAL:
            raise IndexError("list index out of range")
        _csx.check(st, "csx_compress")
        return _from_device(h, lambda nnz: max(nnz, 1))
    C = cs_spalloc(T.m, T.n, nz, T.x is not None, False)
    cols = np.asarray(T.p[:nz], dtype=np.int64)
    order = np.argsort(cols, kind="stable")
    counts = np.bincount(cols, minlength=T.n) if nz else np.zeros(T.n, dtype=np.int64)
    C.p = [0] + np.cumsum(counts).tolist()
    pad = C.nzmax - nz
    C.i = np.asarray(T.i[:nz], dtype=np.int64)[order].tolist() + [0] * pad
    if T.x is not None:
        C.x = np.asarray(T.x[:nz], dtype=np.float64)[order].tolist() + [0.0] * pad
    return C


def cs_cumsum(p, c, n):
    """p[0..n] = exclusive prefix sums of c; c[0..n-1] = p[0..n-1] (csparse.py:767-784)."""
    if p is None or c is None:
        return -1
    total = 0
    for k in range(n):
        p[k] = total
        total += c[k]
        c[k] = p[k]
    p[n] = total
    return total


def cs_scatter(A, j, beta, w, x, mark, C, nz):
    """x += beta * A(:,j) on host lists, new rows appended to C.i (csparse.py:1961-1989).
    The device SpGEMM (cs_multiply) carries its own accumulator; this is the
    list-level primitive for callers that use it directly."""
    if not CS_CSC(A) or w is None or not CS_CSC(C):
        return -1
    Ai, Ax, Ci = A.i, A.x, C.i
    for p in range(A.p[j], A.p[j + 1]):
        r = Ai[p]
        if w[r] < mark:
            w[r] = mark
            Ci[nz] = r
            nz += 1
            if x is not None:
                x[r] = beta * Ax[p]
        elif x is not None:
            x[r] += beta * Ax[p]
    return nz


def cs_norm(A):
    """1-norm = largest column sum of |a| (csparse.py:1647-1663)."""
    if not CS_CSC(A):
        return -1
    if A._dev is not None:   # device-resident: column sums in storage order, the reference's bits
        if not A._dev.info()[3]:
            return -1
        out = _csx.C.c_double(0.0)
        _csx.check(_csx.lib().csx_norm1(A._dev.handle, out), "csx_norm1")
        return out.value
    if A.x is None:
        return -1
    best = 0
    for j in range(A.n):
        s = 0
        for p in range(A.p[j], A.p[j + 1]):
            s += abs(A.x[p])
        best = max(best, s)
    return best


def cs_pinv(p, n):
    """Inverse permutation (csparse.py:1696-1708)."""
    if p is None:
        return None
    inv = [0] * n
    for k in range(n):
        inv[p[k]] = k
    return inv


# ------------------------------------------------------------ device plumbing --

def _upload(A):
    """Host lists of a CSC `cs` -> libcsx handle.  IndexError for indices the
    reference would have tripped over."""
    n = A.n
    p = _csx.i32(A.p[:n + 1])
    nnz = int(p[n]) if n >= 0 and len(p) == n + 1 else -1
    if nnz < 0 or len(A.i) < nnz or (A.x is not None and len(A.x) < nnz):
        raise IndexError("list index out of range")
    i = _csx.i32(A.i[:nnz])
    x = None if A.x is None else _csx.f64(A.x[:nnz])
    h = _csx.new_handle()
    st = _csx.lib().csx_csc_upload(A.m, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), h)
    if st == _csx.EINVAL:
        raise IndexError("list index out of range")
    _csx.check(st, "csx_csc_upload")
    return h


class _Resident(object):
    """Context manager: a device handle for A, temporary unless A is pinned."""

    def __init__(self, A):
        self.A = A
        self.temp = None

    def __enter__(self):
        A = self.A
        if A._dev is not None:
            return A._dev
        dev = _DevMatrix(_upload(A))
        if A._pinned:
            A._dev = dev
        else:
            self.temp = dev
        return dev

    def __exit__(self, *exc):
        if self.temp is not None:
            self.temp._fin()
        return False


@contextlib.contextmanager
def _resident_handle(A):
    with _Resident(A) as d:
        yield d.handle


def cs_pin(A):
    """Keep A resident on the device (and cache its analyses) until cs_unpin /
    its host lists are reassigned.  In-place edits of A.p / A.i / A.x after
    pinning are not seen: call cs_invalidate(A)."""
    if CS_TRIPLET(A):   # nothing to upload yet: cs_compress will sort it on the device and keep it there
        A._pinned = True
        return A
    if not CS_CSC(A):
        return None
    if A._dev is None:
        A._dev = _DevMatrix(_upload(A))
    A._pinned = True
    A._implicit = False
    return A


def cs_invalidate(A):
    """Tell the library that A.p / A.i / A.x were edited in place after cs_pin: the device copy and every plan
    cached on it (SpMV plans, triangular-solve plans) are dropped and rebuilt from the lists on the next use."""
    if A is not None and not A._lazy:
        A._dev = None
    return A


def cs_unpin(A):
    if A is not None:
        A._pinned = False
        if not A._lazy:
            A._dev = None
    return A


def _from_device(handle, nzmax_rule):
    """Wrap a device result as a lazily materialised `cs`."""
    dev = _DevMatrix(handle)
    m, n, nnz, hv = dev.info()
    C = cs()
    C.m, C.n, C.nz = m, n, -1
    C.nzmax = nzmax_rule(nnz)
    C._dev = dev
    C._lazy = True
    C._pinned = True
    C._implicit = True
    return C


def _vec_in(v, need, what):
    """list / numpy / dvec -> (dvec, writeback)"""
    if isinstance(v, dvec):
        if v.n * v.k < need:
            raise IndexError("list index out of range")
        return v, None
    if len(v) < need:
        raise IndexError("list index out of range")
    return dvec(np.asarray(v, dtype=np.float64)), v


def _write_back(host, d, count):
    if host is not None:
        out = d.numpy().reshape(-1)[:count]
        if isinstance(host, np.ndarray):
            host.reshape(-1)[:count] = out
        else:
            host[:count] = out.tolist()


# -------------------------------------------------------------- hot path ----

def cs_gaxpy(A, x, y, mode=None):
    """y = A*x + y (csparse.py:1199-1213).  True on success, False on bad input.

    Lists: y is updated in place with the reference's exact summation order.
    dvec x / y: stays on the device; `mode` picks the kernel (default: exact for
    list calls, the matrix's best plan for device calls).  A dvec block with k > 1
    is read as one flat vector here; gaxpy_block takes Y += A X for every column."""
    if not CS_CSC(A) or x is None or y is None:
        return False
    if not _meta(A)[1]:     # pattern only (asked of the device for a device-backed A: no download)
        raise TypeError("'NoneType' object is not subscriptable")
    dx, _ = _vec_in(x, A.n, "x")
    dy, yhost = _vec_in(y, A.m, "y")
    if mode is None:
        mode = GAXPY_EXACT if (yhost is not None or not isinstance(x, dvec)) else GAXPY_AUTO
    with _Resident(A) as dA:
        _csx.check(_csx.lib().csx_gaxpy(dA.handle, dx.handle, dy.handle, mode), "csx_gaxpy")
    _write_back(yhost, dy, A.m)
    return True


def _block_in(v):
    """dvec / ndarray / list -> (dvec, rows, k, host object to write back or None)."""
    if isinstance(v, dvec):
        return v, v.n, v.k, None
    a = np.asarray(v)
    if a.ndim not in (1, 2):
        raise TypeError("gaxpy_block: blocks are 1-D vectors or 2-D row-major arrays")
    return dvec(np.ascontiguousarray(a, dtype=np.float64)), a.shape[0], 1 if a.ndim == 1 else a.shape[1], v


def gaxpy_block(A, X, Y, mode=None):
    """Y = A*X + Y for every column of an n-by-k block X and m-by-k block Y (cs_gaxpy, csparse.py:1199-1213, applied
    to each column), in one device call.  True on success; False for a non-CSC A, X or Y None, or unequal k.

    X, Y: dvec blocks (dvec(n, k)), 2-D row-major float64 ndarrays, or 1-D vectors (k = 1: exactly cs_gaxpy).  Y is
    updated in place (an ndarray or list Y is written back).  mode: GAXPY_EXACT (every column bit-identical to the
    reference's cs_gaxpy on it) or GAXPY_AUTO (the fastest route, within rounding); default as cs_gaxpy's: exact
    when Y is host memory or X is not a dvec, AUTO when both are dvec.  IndexError for blocks with too few rows."""
    if not CS_CSC(A) or X is None or Y is None:
        return False
    if not _meta(A)[1]:     # pattern only
        raise TypeError("'NoneType' object is not subscriptable")
    if isinstance(Y, np.ndarray) and Y.dtype != np.float64:
        raise TypeError("gaxpy_block: an ndarray Y must be float64")
    dX, xrows, k, _ = _block_in(X)
    dY, yrows, ky, yhost = _block_in(Y)
    if k != ky:
        return False
    if xrows < A.n or yrows < A.m:
        raise IndexError("list index out of range")
    if mode is None:
        mode = GAXPY_EXACT if (yhost is not None or not isinstance(X, dvec)) else GAXPY_AUTO
    with _Resident(A) as dA:
        _csx.check(_csx.lib().csx_gaxpy_block(dA.handle, dX.handle, dY.handle, k, mode), "csx_gaxpy_block")
    if yhost is not None:
        out = dY.numpy().reshape(yrows, k)[:A.m]
        if isinstance(yhost, np.ndarray):
            yhost[:A.m] = out if yhost.ndim == 2 else out[:, 0]
        else:
            yhost[:A.m] = out.tolist() if k > 1 else out[:, 0].tolist()
    return True


def _block_shape(v):
    """dvec / ndarray / list -> (dvec or float64 ndarray, rows, k); nothing is uploaded"""
    if isinstance(v, dvec):
        return v, v.n, v.k
    a = np.asarray(v, dtype=np.float64)
    if a.ndim not in (1, 2):
        raise TypeError("blocks are 1-D vectors or 2-D row-major arrays")
    return np.ascontiguousarray(a), a.shape[0], 1 if a.ndim == 1 else a.shape[1]


def _residual_into(hA, dX, dB, dR, k, trans):
    """csx_residual_block into dR (a dvec, or None: omega and rnorm only) -> (omega, rnorm)"""
    omega, rnorm = np.empty(k, dtype=np.float64), np.empty(k, dtype=np.float64)
    _csx.check(_csx.lib().csx_residual_block(hA, dX.handle, dB.handle, dR.handle if dR is not None else 0, k,
                                             1 if trans else 0, _csx.pd(omega), _csx.pd(rnorm)), "csx_residual_block")
    return omega, rnorm


def _residual_sym_into(hA, dX, dB, dR, k, trans=False):
    """csx_residual_sym_block into dR (a dvec, or None: omega and rnorm only) -> (omega, rnorm); trans has no effect"""
    omega, rnorm = np.empty(k, dtype=np.float64), np.empty(k, dtype=np.float64)
    _csx.check(_csx.lib().csx_residual_sym_block(hA, dX.handle, dB.handle, dR.handle if dR is not None else 0, k,
                                                 _csx.pd(omega), _csx.pd(rnorm)), "csx_residual_sym_block")
    return omega, rnorm


def residual_block(A, X, B, trans=False, residual=True, sym=False):
    """(R, omega, rnorm) of a block of solutions: R = B - A X (trans=True: B - A' X) as a new dvec (None when
    residual=False), omega[c] = max_i |r_ic| / (|A| |x_c| + |b_c|)_i the componentwise backward error of column c (0 / 0
    counts as 0; Oettli-Prager: x_c solves a system whose entries differ from A's and b_c's by at most omega[c] of
    themselves) and rnorm[c] = max_i |r_ic|, numpy arrays of k doubles -- one pass over the matrix, one order of operations
    fixed by the matrix: a run is deterministic, a NaN in a column shows in that column's omega and rnorm.
    trans=True reads A's stored columns as the rows of A': no plan, no transpose.
    sym=True: A is square and stands for the symmetric matrix S a Cholesky factorisation sees in it -- its stored entries with
    row <= column, mirrored; whatever lies strictly below the diagonal is ignored, so an upper-triangle-only storage, a full one
    and one with other values below give the same bytes (duplicates in the upper triangle are summed, where
    cs_chol keeps the last).  trans has no effect then (S = S').  A fully stored symmetric A with sorted columns gives the
    bytes of the general call.

    X, B: dvec blocks, 2-D row-major arrays, or 1-D vectors / lists (one column).  False for a non-CSC A, X or B None,
    unequal k, or sym=True with a non-square A; IndexError for blocks with too few rows; TypeError for a pattern-only A."""
    if not CS_CSC(A) or X is None or B is None or (sym and A.m != A.n):
        return False
    if sym:
        trans = False
    if not _meta(A)[1]:     # pattern only
        raise TypeError("'NoneType' object is not subscriptable")
    X, xrows, k = _block_shape(X)
    B, brows, kb = _block_shape(B)
    if k != kb or k < 1:
        return False
    rows, cols = (A.n, A.m) if trans else (A.m, A.n)
    if xrows < cols or brows < rows:
        raise IndexError("list index out of range")
    dX = X if isinstance(X, dvec) else dvec(X)
    dB = B if isinstance(B, dvec) else dvec(B)
    dR = dvec(rows, k) if residual else None
    with _Resident(A) as dA:
        omega, rnorm = (_residual_sym_into if sym else _residual_into)(dA.handle, dX, dB, dR, k, trans)
    return dR, omega, rnorm


def outer_on_pattern(A, U, V, alpha=1.0, sym=False):
    """alpha U V' sampled on A's pattern: a NEW dvec of nnz(A) doubles in A's storage order, out[q] = alpha * sum_c U[i_q, c] *
    V[j_q, c] for the stored entry q at (i_q, j_q) -- never the m x n product (include/csx.h "outer product ... on a pattern",
    DESIGN.md §31).  With U the adjoint solution and V the solution of a solve, alpha = -1, it is the gradient of a loss with
    respect to A's entries, in the form refactor(values) and add_plan.add(values=...) take.  Only A's pattern is read: a
    pattern-only A is accepted; duplicate and unsorted row indices are fine, every slot gets its own value.  One order of
    operations that depends on k alone: a run is deterministic, NaN and inf reach only the entries whose two rows hold them.
    sym=True: A is square and stands for the symmetric matrix S in its upper triangle, as in residual_block(sym=True): an
    entry above the diagonal stands at two places of S and takes alpha * sum_c (U[i, c] V[j, c] + U[j, c] V[i, c]), a diagonal
    entry alpha * sum_c U[i, c] V[i, c], an entry below the diagonal +0.0.

    U (m rows), V (n rows): dvec blocks, 2-D row-major arrays, or 1-D vectors / lists (one column); they may be the same
    block.  False for a non-CSC A, U or V None, unequal k, or sym=True with a non-square A; IndexError for blocks with too few
    rows."""
    if not CS_CSC(A) or U is None or V is None or (sym and A.m != A.n):
        return False
    same = U is V
    U, urows, k = _block_shape(U)
    V, vrows, kv = (U, urows, k) if same else _block_shape(V)
    if k != kv or k < 1:
        return False
    if urows < A.m or vrows < A.n:
        raise IndexError("list index out of range")
    dU = U if isinstance(U, dvec) else dvec(U)
    dV = dU if same else (V if isinstance(V, dvec) else dvec(V))
    out = dvec(_meta(A)[0])
    with _Resident(A) as dA:
        _csx.check(_csx.lib().csx_pattern_outer(dA.handle, dU.handle, dV.handle, k, 1 if sym else 0, float(alpha), out.handle),
                   "csx_pattern_outer")
    return out


def cs_gaxpy_prepare(A, mode=GAXPY_AUTO):
    """Build the SpMV plan of a pinned matrix ahead of time (outside timed regions)."""
    cs_pin(A)
    _csx.check(_csx.lib().csx_gaxpy_prepare(A._dev.handle, mode), "csx_gaxpy_prepare")
    return True


def cs_transpose(A, values):
    """C = A' (csparse.py:2292-2315); None if A is not CSC."""
    if not CS_CSC(A):
        return None
    with _Resident(A) as dA:
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_transpose(dA.handle, 1 if values else 0, h), "csx_transpose")
    C = _from_device(h, lambda nnz: max(nnz, 1))
    if not A._pinned:
        C._materialise()
        C._dev = None
        C._pinned = False
    return C


def cs_multiply(A, B):
    """C = A*B (csparse.py:1608-1642): columns in first-touch order, trimmed to nnz."""
    if not CS_CSC(A) or not CS_CSC(B):
        return None
    if A.n != B.m:
        return None
    with _Resident(A) as dA, _Resident(B) as dB:
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_multiply(dA.handle, dB.handle, h), "csx_multiply")
    C = _from_device(h, lambda nnz: nnz)
    if not (A._pinned and B._pinned):
        C._materialise()
        C._i = C._i[:C.nzmax]
        if C._x is not None:
            C._x = C._x[:C.nzmax]
        C._dev = None
        C._pinned = False
    return C



def _meta(A):
    """(number of entries, has values) of a CSC matrix without pulling a device-resident one to the host."""
    if A._lazy:
        _, _, nnz, hv = A._dev.info()
        return nnz, hv
    return A._p[A.n], A._x is not None


def _result(h, nzmax_rule, keep_on_device):
    """Device result -> cs: lazy and pinned when the inputs were pinned, host lists otherwise."""
    C = _from_device(h, nzmax_rule)
    if not keep_on_device:
        C._materialise()
        C._i = (C._i + [0] * C.nzmax)[:C.nzmax]
        if C._x is not None:
            C._x = (C._x + [0.0] * C.nzmax)[:C.nzmax]
        C._dev = None
        C._pinned = False
    return C


def _replace_in_place(A, C):
    """Give A the contents of C (the reference's in-place functions mutate their argument)."""
    A.nzmax = C.nzmax
    if C._lazy:
        A._p, A._i, A._x = [], [], []
        A._dev, A._lazy, A._pinned, A._implicit = C._dev, True, True, C._implicit
    else:
        A._dev, A._lazy, A._pinned = None, False, False
        A._p, A._i, A._x = C._p, C._i, C._x


def cs_add(A, B, alpha, beta):
    """C = alpha*A + beta*B (csparse.py:163-192): column j in first-touch order over A(:,j) then
    B(:,j); not trimmed (nzmax = nnz(A) + nnz(B)).  None if not CSC or the shapes differ."""
    if not CS_CSC(A) or not CS_CSC(B):
        return None
    if A.m != B.m or A.n != B.n:
        return None
    room = _meta(A)[0] + _meta(B)[0]
    with _Resident(A) as dA, _Resident(B) as dB:
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_add(dA.handle, dB.handle, float(alpha), float(beta), h), "csx_add")
    return _result(h, lambda nnz: max(room, 1), A._pinned and B._pinned)


def cs_dupl(A):
    """Sum duplicate entries into their first occurrence, in place (csparse.py:1035-1065)."""
    if not CS_CSC(A):
        return False
    nnz, hv = _meta(A)
    if not hv and nnz > 0:
        raise TypeError("'NoneType' object is not subscriptable")   # as the reference on a pattern-only matrix
    pinned = A._pinned
    with _Resident(A) as dA:
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_dupl(dA.handle, h), "csx_dupl")
    _replace_in_place(A, _result(h, lambda nnz: nnz, pinned))
    return True


class _FoldPlan(object):
    """What the three plans of new values into a fixed pattern share (assembly_plan, multiply_plan, add_plan; csx_fold.h): the
    handle, info(), the exact-length check of given values, the .matrix made once, and the tail of .update().  A plan sets
    _INFO (the fields of its info call, in the library's order) and _INFO_CALL, and defines _first_matrix(),
    _new_matrix(*values) and _run(out handle, *values); one whose reference does not trim its result defines _nzmax(nnz)."""

    def _own(self, h):
        self._handle = h
        self._fin = weakref.finalize(self, _csx.free, h)
        self._matrix = None

    def info(self):
        out = (_csx.C.c_int64 * len(self._INFO))()
        _csx.check(getattr(_csx.lib(), self._INFO_CALL)(self._handle, out), self._INFO_CALL)
        return dict(zip(self._INFO, (int(v) for v in out)))

    @staticmethod
    def _vector(values, count, complaint):
        """list / numpy / dvec of exactly count numbers -> a dvec (the caller's own when it is one: it is only read);
        complaint: the ValueError's text, with a %d for the count given"""
        v = values if isinstance(values, dvec) else dvec(np.asarray(values, dtype=np.float64).ravel())
        if v.n * v.k != count:
            raise ValueError(complaint % (v.n * v.k))
        return v

    @staticmethod
    def _nzmax(nnz):
        return nnz   # the reference trims: nzmax = nnz

    @property
    def matrix(self):
        if self._matrix is None:
            self._matrix = cs_pin(_from_device(self._first_matrix(), self._nzmax))
        return self._matrix

    def _fresh(self, *values):
        out = dvec(self.nnz)
        self._run(out.handle, *values)
        return out

    def _update(self, *values):
        M = self.matrix
        if M._dev is None:      # unpinned or invalidated by the caller since: resident again, from its lists
            cs_pin(M)
        dev = M._dev
        if not dev.info()[3]:   # pattern only so far: the first values allocate them
            M._dev = dev = _DevMatrix(self._new_matrix(*values))
            if not M._lazy:
                M._x = [0.0] * M.nzmax    # (filled by _refactored below)
        else:
            self._run(dev.handle, *values)
        _refactored(M, dev)
        return M


class _AssemblyPlan(_FoldPlan):
    """What assembly_plan returns: see there.  info(): nz, nnz, max_dup (the most triplets of one slot), long_slots (slots
    folded by a wave of their own), build_us (the host build of the plan) and kernel_us (the last assemble / update launch,
    between two events)."""

    _INFO = ("nz", "nnz", "max_dup", "long_slots", "build_us", "kernel_us")
    _INFO_CALL = "csx_assemble_plan_info"

    def __init__(self, T):
        nz = T.nz
        if len(T.i) < nz or len(T.p) < nz or (T.x is not None and len(T.x) < nz):
            raise IndexError("list index out of range")
        rows, cols = _csx.i32(T.i[:nz]), _csx.i32(T.p[:nz])
        h = _csx.new_handle()
        st = _csx.lib().csx_assemble_plan(T.m, T.n, nz, _csx.pi(rows), _csx.pi(cols), h)
        if st == _csx.EINVAL and T.m >= 0 and T.n >= 0 and 0 <= nz <= 2 ** 31 - 1:
            raise IndexError("list index out of range")   # the sizes are legal: an index is not
        _csx.check(st, "csx_assemble_plan")
        self._own(h)
        self.m, self.n, self.nz = T.m, T.n, nz
        self.nnz = self.info()["nnz"]
        self._x0 = None if T.x is None else np.array(T.x[:nz], dtype=np.float64)   # T's values, until .matrix is made

    def _values(self, values, what):
        if values is None:
            raise ValueError("%s: no values" % what)
        return self._vector(values, self.nz, "%s: %%d values given, the plan has %d triplets" % (what, self.nz))

    def _new_matrix(self, v):
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_assemble_matrix(self._handle, v.handle if v is not None else 0, h), "csx_assemble_matrix")
        return h

    def _first_matrix(self):
        h = self._new_matrix(None if self._x0 is None else dvec(self._x0))
        self._x0 = None
        return h

    def _run(self, hout, v):
        _csx.check(_csx.lib().csx_assemble(self._handle, v.handle, hout), "csx_assemble")

    def assemble(self, values):
        return self._fresh(self._values(values, "assemble"))

    def update(self, values=None):
        return self._update(self._values(values, "update"))

    def pullback(self, gA):
        g = self._vector(gA, self.nnz, "pullback: %%d values given, the plan's matrix has %d entries" % self.nnz)
        out = dvec(self.nz)
        _csx.check(_csx.lib().csx_assemble_pullback(self._handle, g.handle, out.handle), "csx_assemble_pullback")
        return out


def assembly_plan(T):
    """The plan of cs_dupl(cs_compress(T)) for a triplet list whose (i, j) stay and whose values change every step
    (include/csx.h "assembly plan").  Only T.m, T.n, T.nz, T.i, T.p are read for the plan (a pattern-only T is
    fine); IndexError for an index out of range, as cs_compress; None when T is not a triplet matrix.  The plan has
    m, n, nz, nnz and info(), and
      .matrix            cs_dupl(cs_compress(T)) as a device-resident pinned `cs` (nzmax = nnz, as cs_dupl leaves it) with T's values,
                         or pattern only when T has none; made on first use, once.
      .assemble(values)  values: list, numpy array or dvec of exactly nz numbers, in T's triplet order (ValueError otherwise;
                         never modified, never aliased).  A NEW dvec of nnz values in .matrix's storage order -- the reference's
                         bits -- which is what lusol_factor(P.matrix).refactor(...) and btf_factor(P.matrix).refactor(...) take.
      .update(values)    the same values straight into .matrix, in place: the plans cached on it go, solvers built on it
                         re-plan, host lists already read from it are refreshed in place.  Returns .matrix.  The first update
                         of a pattern-only .matrix gives it its values; update() without values is a ValueError.
      .pullback(gA)      the gradient with respect to the triplet values of a loss whose gradient with respect to the assembled
                         values is gA (list, numpy array or dvec of exactly nnz numbers in .matrix's storage order, as solve_grad
                         returns it; ValueError otherwise): a NEW dvec of nz doubles in T's triplet order, gT[t] = gA[slot of t]
                         -- a slot is the sum of its triplets, so each takes the slot's gradient, bit for bit; one launch."""
    if not CS_TRIPLET(T):
        return None
    return _AssemblyPlan(T)


class _MultiplyPlan(_FoldPlan):
    """What multiply_plan returns: see there.  info(): m, n, nnz, products, max_products (the most products of one slot),
    long_slots (slots folded by a wave of their own), build_us (the host build of the plan) and kernel_us (the last step
    between two events: both launches when scaled)."""

    _INFO = ("m", "n", "nnz", "products", "max_products", "long_slots", "build_us", "kernel_us")
    _INFO_CALL = "csx_multiply_plan_info"

    def __init__(self, A, B):
        self._A, self._B = A, B            # kept alive: None for ax / bx means their current values
        self._anz, self._bnz = _meta(A)[0], _meta(B)[0]
        h = _csx.new_handle()
        with _Resident(A) as dA, _Resident(B) as dB:
            st = _csx.lib().csx_multiply_plan(dA.handle, dB.handle, h)
        if st == _csx.EINVAL:
            raise ValueError(_last_error())
        _csx.check(st, "csx_multiply_plan")
        self._own(h)
        self.k = A.n
        info = self.info()
        self.m, self.n, self.nnz, self.products = info["m"], info["n"], info["nnz"], info["products"]

    def _step(self, ax, bx, scale, call):
        """call(handle of Ax, handle of Bx, handle of d or 0) with the operands resident for its duration"""
        for M, given, nz, what in ((self._A, ax, self._anz, "A"), (self._B, bx, self._bnz, "B")):
            if given is None and _meta(M) != (nz, True):
                raise ValueError("multiply plan: %s has no values (or another entry count) and none are given" % what)
        va, vb, d = (None if given is None else
                     self._vector(given, count, "multiply plan: %%d numbers given for %s, %d expected" % (what, count))
                     for given, count, what in ((ax, self._anz, "ax"), (bx, self._bnz, "bx"), (scale, self.k, "scale")))
        with contextlib.ExitStack() as held:   # an operand whose values are given is not made resident for them
            ha = va.handle if va is not None else held.enter_context(_Resident(self._A)).handle
            hb = vb.handle if vb is not None else held.enter_context(_Resident(self._B)).handle
            return call(ha, hb, d.handle if d is not None else 0)

    def _new_matrix(self, ax, bx, scale):
        """a new matrix handle with the plan's pattern and the values of a step"""
        h = _csx.new_handle()
        _csx.check(self._step(ax, bx, scale, lambda a, b, d: _csx.lib().csx_multiply_plan_matrix(self._handle, a, b, d, h)),
                   "csx_multiply_plan_matrix")
        return h

    def _first_matrix(self):
        if _meta(self._A)[1] and _meta(self._B)[1]:
            return self._new_matrix(None, None, None)
        h = _csx.new_handle()                          # as cs_multiply of a pattern-only operand: pattern only
        _csx.check(_csx.lib().csx_multiply_plan_matrix(self._handle, 0, 0, 0, h), "csx_multiply_plan_matrix")
        return h

    def _run(self, hout, ax, bx, scale):
        _csx.check(self._step(ax, bx, scale, lambda a, b, d: _csx.lib().csx_multiply_plan_run(self._handle, a, b, d, hout)),
                   "csx_multiply_plan_run")

    def multiply(self, ax=None, bx=None, scale=None):
        return self._fresh(ax, bx, scale)

    def update(self, ax=None, bx=None, scale=None):
        return self._update(ax, bx, scale)


def multiply_plan(A, B):
    """The plan of cs_multiply(A, B) for operands whose patterns stay and whose values change every step (include/csx.h
    "multiply plan").  Only the patterns are read for the plan; None where cs_multiply returns None (an operand
    that is not CSC, A.n != B.m); ValueError when the products do not fit int32.  The plan keeps A and B alive, has m, n, k,
    nnz, products and info(), and
      .matrix                       cs_multiply(A, B) as a device-resident pinned `cs` (nzmax = nnz) with the reference's bits from
                                    A's and B's values at first use, or pattern only when either has none; made once.
      .multiply(ax, bx, scale)      ax / bx: list, numpy array or dvec of exactly nnz(A) / nnz(B) numbers in storage order, None
                                    = the operand's current values; scale: None or exactly k numbers d, C = A diag(d) B.  A NEW
                                    dvec of nnz values in .matrix's storage order -- the reference's bits -- which is what
                                    cholsol_factor(P.matrix).refactor(...) takes.  ValueError on a wrong length, or when an
                                    operand has no values and none are given.  Inputs are never modified or aliased.
      .update(ax, bx, scale)        the same values straight into .matrix, in place: the plans cached on it go, solvers built on
                                    it re-plan, host lists already read from it are refreshed in place.  Returns .matrix.
    A `cs` operand is trusted to still have the pattern the plan was made from: only its shape and entry count are checked."""
    if not CS_CSC(A) or not CS_CSC(B):
        return None
    if A.n != B.m:
        return None
    return _MultiplyPlan(A, B)


class _AddPlan(_FoldPlan):
    """What add_plan returns: see there.  info(): k, m, n, nnz, terms, max_terms (the most terms of one slot), long_slots (slots
    folded by a wave of their own; 0 for an aligned plan), aligned (1: every operand has the sum's pattern in the sum's order,
    the step streams the values and reads no index), build_us (the host build of the plan), kernel_us (the last step between
    two events) and nzmax (what the reference's chain of cs_add leaves: it does not trim)."""

    _INFO = ("k", "m", "n", "nnz", "terms", "max_terms", "long_slots", "aligned", "build_us", "kernel_us", "nzmax")
    _INFO_CALL = "csx_add_plan_info"

    def __init__(self, operands, coef):
        self._ops = tuple(operands)        # kept alive: None for an operand's values means its current ones
        self.k = len(self._ops)
        self._nz = [_meta(A)[0] for A in self._ops]
        self._coef = self._coefficients(coef, None)
        h = _csx.new_handle()
        with contextlib.ExitStack() as held:
            handles = [held.enter_context(_Resident(A)).handle for A in self._ops]
            st = _csx.lib().csx_add_plan(self.k, (_csx.H * self.k)(*(v.value for v in handles)), h)
        if st == _csx.EINVAL:
            raise ValueError(_last_error())
        _csx.check(st, "csx_add_plan")
        self._own(h)
        info = self.info()
        self.m, self.n, self.nnz, self.terms = info["m"], info["n"], info["nnz"], info["terms"]
        self._room = max(info["nzmax"], 1)   # (cs_spalloc allocates at least one entry)

    def _nzmax(self, nnz):
        return self._room

    def _coefficients(self, coef, default):
        if coef is None:
            coef = default if default is not None else [1.0] * self.k
        c = np.asarray([float(v) for v in coef], dtype=np.float64)
        if c.size != self.k:
            raise ValueError("add plan: %d coefficients given for %d operands" % (c.size, self.k))
        return c

    def _step(self, coef, values, call):
        """call(k host doubles, k handles) with the operands whose values are not given resident for its duration"""
        c = self._coefficients(coef, self._coef)
        if values is None:
            values = [None] * self.k
        if len(values) != self.k:
            raise ValueError("add plan: values for %d operands given, the plan has %d" % (len(values), self.k))
        for r, (A, given, nz) in enumerate(zip(self._ops, values, self._nz)):
            if given is None and _meta(A) != (nz, True):
                raise ValueError("add plan: operand %d has no values (or another entry count) and none are given" % r)
        vecs = [None if given is None else
                self._vector(given, nz, "add plan: %%d numbers given for operand %d, %d expected" % (r, nz))
                for r, (given, nz) in enumerate(zip(values, self._nz))]
        with contextlib.ExitStack() as held:   # an operand whose values are given is not made resident for them
            handles = [v.handle if v is not None else held.enter_context(_Resident(A)).handle
                       for v, A in zip(vecs, self._ops)]
            return call(_csx.pd(c), (_csx.H * self.k)(*(v.value for v in handles)))

    def _new_matrix(self, coef, values):
        """a new matrix handle with the plan's pattern and the values of a step"""
        h = _csx.new_handle()
        _csx.check(self._step(coef, values, lambda c, x: _csx.lib().csx_add_plan_matrix(self._handle, c, x, h)),
                   "csx_add_plan_matrix")
        return h

    def _first_matrix(self):
        if all(_meta(A)[1] for A in self._ops):
            return self._new_matrix(None, None)
        h = _csx.new_handle()                          # as cs_add of a pattern-only operand: pattern only
        _csx.check(_csx.lib().csx_add_plan_matrix(self._handle, None, None, h), "csx_add_plan_matrix")
        return h

    def _run(self, hout, coef, values):
        _csx.check(self._step(coef, values, lambda c, x: _csx.lib().csx_add_plan_run(self._handle, c, x, hout)),
                   "csx_add_plan_run")

    def add(self, coef=None, values=None):
        return self._fresh(coef, values)

    def update(self, coef=None, values=None):
        return self._update(coef, values)


def add_plan(A, B, *more, coef=None):
    """The plan of c0*A + c1*B + c2*more[0] + ... for operands whose patterns stay and whose values and coefficients change every
    step (include/csx.h "add plan"): the reference's chain cs_add(cs_add(A, B, c0, c1), more[0], 1, c2) ...,
    cs_add itself for two operands.  Only the patterns are read for the plan; None where cs_add returns None (an operand that is
    not CSC, shapes that differ); ValueError for more than 8 operands or when the operands' entries together do not fit int32.
    coef: one number per operand (default all 1.0), the plan's own coefficients.  The plan keeps its operands alive, has
    m, n, k, nnz, terms and info(), and
      .matrix                 the chain as a device-resident pinned `cs` with the reference's bits from the operands' values at
                              first use (nzmax as the chain leaves it: cs_add does not trim), or pattern only when any operand
                              has no values; made once.
      .add(coef, values)      coef: k numbers (Python ints are fine), None = the plan's own; values: None, or k items, each None
                              (that operand's current values) or a list, numpy array or dvec of exactly nnz(operand) numbers in
                              storage order.  A NEW dvec of nnz values in .matrix's storage order -- the reference's bits --
                              which is what cholsol_factor / lusol_factor / btf_factor(P.matrix).refactor(...) take.
                              ValueError on a wrong length or count, or when an operand has no values and none are given.
                              Inputs are never modified or aliased.
      .update(coef, values)   the same values straight into .matrix, in place: the plans cached on it go, solvers built on it
                              re-plan, host lists already read from it are refreshed in place.  Returns .matrix.
    A `cs` operand is trusted to still have the pattern the plan was made from: only its shape and entry count are checked."""
    operands = (A, B) + tuple(more)
    if any(not CS_CSC(M) for M in operands):
        return None
    if any(M.m != A.m or M.n != A.n for M in operands):
        return None
    if len(operands) > 8:
        raise ValueError("add_plan: %d operands, at most 8" % len(operands))
    return _AddPlan(operands, coef)


def cs_fkeep(A, fkeep, other):
    """Keep the entries for which fkeep(i, j, aij, other) is true, in place; returns the new number of
    entries, -1 on bad input (csparse.py:1172-1196).  The predicate is a Python callable, so this generic
    form runs on the host; cs_dropzeros / cs_droptol are the device versions of its two uses."""
    if not CS_CSC(A) or fkeep is None:
        return -1
    Ap, Ai, Ax, n = A.p, A.i, A.x, A.n
    nz = 0
    for j in range(n):
        p = Ap[j]
        Ap[j] = nz
        while p < Ap[j + 1]:
            if fkeep(Ai[p], j, Ax[p] if Ax is not None else 1.0, other):
                if Ax is not None:
                    Ax[nz] = Ax[p]
                Ai[nz] = Ai[p]
                nz += 1
            p += 1
    Ap[n] = nz
    A.p = Ap
    A.i = (Ai + [0] * nz)[:nz] if isinstance(Ai, list) else list(Ai[:nz])
    if Ax is not None:
        A.x = (Ax + [0.0] * nz)[:nz] if isinstance(Ax, list) else list(Ax[:nz])
    A.nzmax = nz
    return nz


def _drop(A, mode, tol):
    if not CS_CSC(A):
        return -1
    if not _meta(A)[1]:   # the reference passes aij = 1 for a pattern-only matrix
        keep_all = True if mode == 0 else 1.0 > tol
        return cs_fkeep(A, lambda i, j, a, o: keep_all, None)
    pinned = A._pinned
    with _Resident(A) as dA:
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_drop(dA.handle, mode, float(tol), h), "csx_drop")
    C = _result(h, lambda nnz: nnz, pinned)
    _replace_in_place(A, C)
    return A._dev.info()[2] if A._lazy else A._p[A.n]


def cs_dropzeros(A):
    """Remove explicit zeros, in place; returns the new nnz (csparse.py:1019-1031)."""
    return _drop(A, 0, 0.0)


def cs_droptol(A, tol):
    """Remove entries with |a| <= tol, in place; returns the new nnz (csparse.py:1002-1014)."""
    return _drop(A, 1, tol)


def cs_permute(A, pinv, q, values):
    """C = P A Q, pinv the inverse row permutation, q the column permutation (csparse.py:1666-1693)."""
    if not CS_CSC(A):
        return None
    if pinv is not None and len(pinv) < A.m or q is not None and len(q) < A.n:
        raise IndexError("list index out of range")
    pv = None if pinv is None else _csx.i32(pinv)
    qv = None if q is None else _csx.i32(q)
    with _Resident(A) as dA:
        h = _csx.new_handle()
        st = _csx.lib().csx_permute(dA.handle, _csx.pi(pv), _csx.pi(qv), 1 if values else 0, h)
    if st == _csx.EINVAL:
        raise IndexError("list index out of range")
    _csx.check(st, "csx_permute")
    return _result(h, lambda nnz: max(nnz, 1), A._pinned)


def cs_symperm(A, pinv, values):
    """Upper triangle of P A P' for a symmetric A whose upper triangle is stored (csparse.py:2220-2255)."""
    if not CS_CSC(A):
        return None
    room = _meta(A)[0]
    pv = None if pinv is None else _csx.i32(pinv)
    with _Resident(A) as dA:
        h = _csx.new_handle()
        st = _csx.lib().csx_symperm(dA.handle, _csx.pi(pv), 1 if values else 0, h)
    if st == _csx.EINVAL:
        raise IndexError("list index out of range")
    _csx.check(st, "csx_symperm")
    return _result(h, lambda nnz: max(room, 1), A._pinned)

def _plan(dT, kind):
    h = dT.plans.get(kind)
    if h is None:
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_tri_analyse(dT.handle, kind, h), "csx_tri_analyse")
        dT.plans[kind] = h
    return h


def _trisolve(T, x, kind):
    if not CS_CSC(T) or x is None:
        return False
    if not _meta(T)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    if T.m != T.n:
        raise IndexError("list index out of range")
    if _HOST_CHAINS[0] and not isinstance(x, dvec):
        # "tri.host_chains" (opt-in, cs_option): one host right-hand side on a chain-like factor -- the reference's loop on the
        # host inside libcsx, same bits (csx_tri_solve_list); anything else falls through to the device
        buf = _csx.f64(x[:T.n])
        taken = _csx.C.c_int(0)
        with _Resident(T) as dT:
            _csx.check(_csx.lib().csx_tri_solve_list(_plan(dT, kind), _csx.pd(buf), taken), "csx_tri_solve_list")
        if taken.value:
            x[:T.n] = buf.tolist() if isinstance(x, list) else buf
            return True
    dx, xhost = _vec_in(x, T.n, "x")
    nrhs = dx.k
    with _Resident(T) as dT:
        plan = _plan(dT, kind)
        _csx.check(_csx.lib().csx_tri_solve(plan, dx.handle, nrhs), "csx_tri_solve")
    _write_back(xhost, dx, T.n * nrhs)
    return True


_HOST_CHAINS = [False]


def cs_option(name, value):
    """csx_set_option from the drop-in module (DESIGN.md lists the names).  "tri.host_chains" = 1 additionally lets the list-level
    cs_lsolve / cs_ltsolve / cs_usolve / cs_utsolve / cs_cholsol / cholsol_factor(...).solve(list) try the host loop first."""
    _csx.check(_csx.lib().csx_set_option(name.encode(), int(value)), "csx_set_option")
    if name == "tri.host_chains":
        _HOST_CHAINS[0] = bool(value)


def _cholsol_list_on_host(plan, b, n):
    """cs_cholsol's solve sequence for a LIST b by csx_cholsol_solve_list ("tri.host_chains"); True when it was taken"""
    if not _HOST_CHAINS[0] or isinstance(b, dvec):
        return False
    buf = _csx.f64(b[:n])
    taken = _csx.C.c_int(0)
    _csx.check(_csx.lib().csx_cholsol_solve_list(plan, _csx.pd(buf), taken), "csx_cholsol_solve_list")
    if taken.value:
        b[:n] = buf.tolist() if isinstance(b, list) else buf
    return bool(taken.value)


def cs_lsolve(L, x):
    """Solve L x = b in place, diagonal first in each column (csparse.py:1330-1345)."""
    return _trisolve(L, x, TRI_L)


def cs_ltsolve(L, x):
    """Solve L' x = b in place (csparse.py:1348-1365)."""
    return _trisolve(L, x, TRI_LT)


def cs_usolve(U, x):
    """Solve U x = b in place, diagonal last in each column (csparse.py:2368-2385)."""
    return _trisolve(U, x, TRI_U)


def cs_utsolve(U, x):
    """Solve U' x = b in place (csparse.py:2460-2475)."""
    return _trisolve(U, x, TRI_UT)


def _perm_handle(p, n):
    if p is None:
        return _csx.H(0), None
    a = _csx.i32(p[:n])
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_ivec_upload(_csx.pi(a), n, h), "csx_ivec_upload")
    return h, h


def _permute(p, b, x, n, inverse):
    if x is None or b is None:
        return False
    if isinstance(b, dvec) and isinstance(x, dvec):
        h, tmp = _perm_handle(p, n)
        try:
            _csx.check(_csx.lib().csx_permute_vec(h, b.handle, x.handle, n, b.k, inverse), "csx_permute_vec")
        finally:
            _csx.free(tmp)
        return True
    # a single host list: the reference's own loop is the whole job
    if inverse:
        for k in range(n):
            x[p[k] if p is not None else k] = b[k]
    else:
        for k in range(n):
            x[k] = b[p[k] if p is not None else k]
    return True


def cs_ipvec(p, b, x, n):
    """x(p) = b (csparse.py:1264-1277); p None is the identity."""
    return _permute(p, b, x, n, 1)


def cs_pvec(p, b, x, n):
    """x = b(p) (csparse.py:1779-1792); p None is the identity."""
    return _permute(p, b, x, n, 0)


# ------------------------------------------------------------- Cholesky ----

def _pattern_np(A):
    """Column pointers and row indices of A as int32 arrays: straight from the device copy when there is one (a pinned
    or device-made matrix: that copy is the matrix), else from the lists."""
    n = A.n
    if A._dev is not None:
        m_, n_, nnz, hv = A._dev.info()
        p = np.empty(n + 1, dtype=np.int32)
        i = np.empty(max(nnz, 1), dtype=np.int32)
        _csx.check(_csx.lib().csx_csc_download(A._dev.handle, _csx.pi(p), _csx.pi(i), None), "csx_csc_download")
        return p, i[:nnz]
    p = _csx.i32(A.p[:n + 1])
    return p, _csx.i32(A.i[:int(p[n])])


def _amd_np(order, A):
    """Permutation (int32 array of n entries) for order 1 (A + A', square A), 2 (S'S with S = A less its dense rows) or
    3 (A'A), or None: a nested dissection of that graph (csx_order_nd_host)."""
    if not CS_CSC(A) or order not in (1, 2, 3):
        return None
    n = A.n
    if order == 1 and A.m == n:
        p, i = _pattern_np(A)                                   # the graph of A + A' is formed by the ordering itself
    else:
        # the pattern of A'A (csparse.py:236-256); order 2 first drops the dense rows of A (columns of A')
        Ap, Ai = _pattern_np(A)
        m = A.m
        P = cs_spalloc(m, n, max(len(Ai), 1), False, False)
        P.p, P.i, P.x = Ap.tolist(), Ai.tolist() if len(Ai) else [0], None
        AT = cs_transpose(P, False)
        if order == 2:
            dense = min(n - 2, max(16, int(10 * sqrt(n))))
            cs_fkeep(AT, lambda i, j, a, cnt: cnt[j] <= dense, np.diff(np.asarray(AT.p)).tolist())
        C = cs_multiply(AT, P)
        if C is None:
            return None
        p, i = _csx.i32(C.p[:n + 1]), _csx.i32(C.i[:C.p[n]])
    perm = np.empty(max(n, 1), dtype=np.int32)
    if _csx.load().csx_order_nd_host(n, _csx.pi(p), _csx.pi(i), _csx.pi(perm)) != _csx.OK:
        return None
    return perm[:n]


def cs_amd(order, A):
    """Fill-reducing ordering p (csparse.py:214-556): order 1 = for Cholesky / LU of a matrix with a symmetric pattern
    (graph of A + A'), 2 = for LU (graph of S'S, S = A without its dense rows), 3 = for QR (graph of A'A).
    The reference's implementation does not run, so there is no permutation to match: this is a nested
    dissection of the same graphs (breadth-first level separators, host C++), which gives the device a bushy
    elimination tree.  None for order 0 or bad input, like the reference."""
    perm = _amd_np(order, A)
    return None if perm is None else perm.tolist()


def cs_schol(order, A, _arrays=False):
    """Symbolic Cholesky analysis (csparse.py:2051-2072): ordering, etree, column counts.  order 0 =
    natural; order 1 = cs_amd (here a nested dissection).  The tree is built by host C++ inside libcsx,
    the column counts on the device when A is resident there.  (_arrays: internal -- S.parent / S.cp / S.pinv stay
    int32 arrays instead of becoming lists; cs_cholsol and cholsol_factor, which keep S to themselves, use it to skip
    half a dozen list conversions of length n.)"""
    if not CS_CSC(A) or order not in (0, 1):
        return None
    if order == 1:
        P = _amd_np(1, A)
        if P is None:
            return None
        pinv = np.empty(A.n, dtype=np.int32)
        pinv[P] = np.arange(A.n, dtype=np.int32)          # cs_pinv (csparse.py:1696-1708)
        C = cs_symperm(A, pinv, False)
        S = cs_schol(0, C, _arrays)
        if S is not None:
            S.pinv = pinv if _arrays else pinv.tolist()
        return S
    n = A.n
    parent = np.empty(max(n, 1), dtype=np.int32)
    cp = np.empty(n + 1, dtype=np.int32)
    if A._dev is not None and A.m == A.n:
        # device-resident matrix: tree on the host, column counts from the device's row-subtree walks
        st = _csx.lib().csx_schol(A._dev.handle, _csx.pi(parent), _csx.pi(cp))
    else:
        p = _csx.i32(A.p[:n + 1])
        i = _csx.i32(A.i[:int(p[n])])
        st = _csx.load().csx_schol_host(n, _csx.pi(p), _csx.pi(i), _csx.pi(parent), _csx.pi(cp))
    if st != _csx.OK:
        return None
    S = css()
    S.pinv = None
    S.q = None
    S.parent = parent[:n] if _arrays else parent[:n].tolist()
    S.cp = cp if _arrays else cp.tolist()
    S.unz = S.lnz = int(cp[n])
    return S


def cs_chol(A, S):
    """Numeric Cholesky L L' = P A P' (csparse.py:561-619); None if A is not
    positive definite.  The returned csn holds L as a device-backed `cs`."""
    if not CS_CSC(A) or S is None or S.cp is None or S.parent is None:
        return None
    n = A.n
    parent = _csx.i32(S.parent)
    cp = _csx.i32(S.cp)
    pinv = None if S.pinv is None else _csx.i32(S.pinv)
    with _Resident(A) as dA:
        h = _csx.new_handle()
        st = _csx.lib().csx_chol(dA.handle, _csx.pi(parent), _csx.pi(cp), _csx.pi(pinv), h)
    if st == _csx.ENOTSPD:
        return None
    _csx.check(st, "csx_chol")
    N = csn()
    N.L = _from_device(h, lambda nnz: max(nnz, 1))
    N.U = None
    N.pinv = None
    N.B = None
    return N


def spsolve_columns(G, B, pinv=None, lo=True, values=True):
    """cs_spsolve (csparse.py:2078-2113) for every column of B in one device call: a CSC matrix X whose column k
    lists the reach of B(:,k) in the reference's xi[top..n-1] order (cs_reach :1939-1958, cs_dfs :789-829) with the
    solution of G x = B(:,k) beside it, bit-identical to the reference called column by column.  G lower (lo) or
    upper triangular; pinv as in cs_lu (negative = no column yet).  values=False: the reaches alone.  None on bad
    input.  The list-level cs_spsolve / cs_reach / cs_dfs (one column, caller-owned work arrays) stay host functions."""
    if not CS_CSC(G) or not CS_CSC(B) or G.m != G.n or B.m != G.n:
        return None
    pv = None if pinv is None else _csx.i32(pinv[:G.n])
    with _Resident(G) as dG, _Resident(B) as dB:
        h = _csx.new_handle()
        st = _csx.lib().csx_spsolve(dG.handle, dB.handle, None if pv is None else _csx.pi(pv), 1 if lo else 0,
                                    1 if values else 0, h)
        if st == _csx.EINVAL:
            raise IndexError("list index out of range")
        _csx.check(st, "csx_spsolve")
    X = _from_device(h, lambda nnz: max(nnz, 1))
    if not (G._pinned and B._pinned):
        X._materialise()
        X._dev = None
        X._pinned = False
    return X


def reach_columns(G, B, pinv=None):
    """cs_reach (csparse.py:1939-1958) for every column of B: column k of the result = xi[top..n-1]."""
    return spsolve_columns(G, B, pinv, True, False)


def cs_updown(L, sigma, C, parent):
    """Sparse Cholesky rank-1 update (sigma = +1) / downdate (-1): L L' + sigma w w' with w = the one column of
    C, in place (csparse.py:2318-2365).  True on success; False on bad input or when the downdate is not positive
    definite (L is then changed exactly as far as the reference's loop gets).  L.x is bit-identical to the
    reference's.  A list-backed L is updated in its own list objects; a device-backed L stays on the device."""
    if not CS_CSC(L) or not CS_CSC(C) or parent is None:
        return False
    if not _meta(L)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    cnz = C.p[1] - C.p[0]
    if cnz <= 0:
        return True
    ci = _csx.i32(C.i[C.p[0]:C.p[1]])
    cx = _csx.f64(C.x[C.p[0]:C.p[1]])
    par = _csx.i32(parent[:L.n])
    ok = _csx.C.c_int(0)
    lazy = L._lazy
    with _Resident(L) as dL:
        for h in dL.plans.values():          # triangular-solve plans hold copies of the old values
            _csx.free(h)
        dL.plans.clear()
        dL.version += 1                      # cholsol_factor solvers built on this factor re-plan at their next solve
        st = _csx.lib().csx_updown(dL.handle, int(sigma), cnz, _csx.pi(ci), _csx.pd(cx), _csx.pi(par), ok)
        if st == _csx.EINVAL:
            raise IndexError("list index out of range")
        _csx.check(st, "csx_updown")
        if not lazy:                         # the caller holds L.x: update that list in place, like the reference
            m, n, nnz, hv = dL.info()
            x = np.empty(max(nnz, 1), dtype=np.float64)
            _csx.check(_csx.lib().csx_csc_download(dL.handle, None, None, _csx.pd(x)), "csx_csc_download")
            L._x[:nnz] = x[:nnz].tolist()
    return bool(ok.value)


_UPDOWN_INFO = [None]


def _updown_sigma(sigma, k):
    """+1, -1 or k values each +1 / -1 -> int32 array of k; ValueError otherwise"""
    if isinstance(sigma, (int, float, np.integer, np.floating)):
        sg = np.full(k, int(sigma) if sigma in (1, -1) else 0, dtype=np.int32)
        bad = sigma not in (1, -1)
    else:
        v = np.asarray(sigma, dtype=np.float64).ravel()
        bad = len(v) != k or not np.all((v == 1.0) | (v == -1.0))
        sg = v.astype(np.int32) if not bad else None
    if bad:
        raise ValueError("updown_block: sigma must be +1, -1 or a sequence of %d values, each +1 or -1" % k)
    return sg


def _updown_block_call(L, sg, C, parent, flags):
    """csx_updown_block on L (in place, as cs_updown: plans freed, version bumped, host lists updated) -> applied"""
    n = L.n
    par = None
    if parent is not None:
        if len(parent) < n:
            raise ValueError("updown_block: parent is not the elimination tree of L")
        par = _csx.i32(parent[:n])
    applied = _csx.C.c_int32(0)
    t0 = time.perf_counter()
    lazy = L._lazy
    with _Resident(L) as dL, _Resident(C) as dC:
        st = _csx.lib().csx_updown_block(dL.handle, dC.handle, _csx.pi(sg), None if par is None else _csx.pi(par), flags, applied)
        if st == _csx.EINVAL:
            raise IndexError("list index out of range")
        _csx.check(st, "csx_updown_block")
        a = applied.value
        if a == -2:
            raise ValueError("updown_block: parent is not the elimination tree of L")
        changed = a > 0 or (0 <= a < C.n and not flags & 1)
        if changed:
            for h in dL.plans.values():          # triangular-solve plans hold copies of the old values
                _csx.free(h)
            dL.plans.clear()
            dL.version += 1                      # cholsol_factor solvers built on this factor re-plan at their next solve
            if not lazy and L._x is not None:    # the caller holds L.x: update that list in place, like the reference
                _, _, nnz, _ = dL.info()
                x = np.empty(max(nnz, 1), dtype=np.float64)
                _csx.check(_csx.lib().csx_csc_download(dL.handle, None, None, _csx.pd(x)), "csx_csc_download")
                L._x[:nnz] = x[:nnz].tolist()
    ch, uc, gr, ms = _csx.C.c_int32(0), _csx.C.c_int32(0), _csx.C.c_int32(0), _csx.C.c_double(0.0)
    _csx.check(_csx.lib().csx_updown_block_info(ch, uc, gr, ms), "csx_updown_block_info")
    cl, rp = (_csx.C.c_int32 * 4)(), _csx.C.c_int32(0)
    _csx.check(_csx.lib().csx_updown_block_classes(cl, rp), "csx_updown_block_classes")
    _UPDOWN_INFO[0] = {"columns": C.n, "applied": a, "chunks": ch.value, "union_columns": uc.value, "groups": gr.value,
                       "kernel_ms": ms.value, "wall_ms": 1e3 * (time.perf_counter() - t0), "classes": list(cl),
                       "replayed": rp.value}
    return a


def updown_block(L, sigma, C, parent=None):
    """k rank-1 updates / downdates at once: L L' + sum_t sigma_t w_t w_t', w_t = column t of the n-by-k CSC C, read as cs_updown
    (csparse.py:2318-2365) reads its C (a later duplicate row wins; rows off the path of f_t = min row of C(:,t) never read).
    L (cs_chol's: diagonal first, rows ascending; list-backed or on the device) is changed in place exactly as
        for t in range(k):
            if not cs_updown(L, sigma[t], C[:, t], parent): break
    changes it, byte for byte, in ONE device pass over the union of the terms' elimination-tree paths.
    sigma: +1, -1, or k values each +1 / -1.  parent: None (read from L on the device) or L's elimination tree (checked).
    Returns the number of columns applied in full: k on success, t when the downdate of column t is not positive definite (L
    is then the loop's partial state).  An empty column is a success that changes nothing.  IndexError for a row out of range;
    ValueError for a bad sigma, C.m != L.n or a parent that is not L's tree (L unchanged).  updown_info(): the last call's
    columns, chunks, union columns, groups, kernel ms and wall ms."""
    if not CS_CSC(L) or not CS_CSC(C):
        raise ValueError("updown_block: L and C must be CSC matrices")
    if not _meta(L)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    if C.m != L.n or L.m != L.n:
        raise ValueError("updown_block: C has %d rows, L has %d columns" % (C.m, L.n))
    k = C.n
    sg = _updown_sigma(sigma, k)
    if k == 0:
        _UPDOWN_INFO[0] = {"columns": 0, "applied": 0, "chunks": 0, "union_columns": 0, "groups": 0, "kernel_ms": 0.0,
                           "wall_ms": 0.0, "classes": [0, 0, 0, 0], "replayed": 0}
        return 0
    if not _meta(C)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    return _updown_block_call(L, sg, C, parent, 0)


def updown_info():
    """the last updown_block's (or cholsol_factor update / downdate's) columns, applied, chunks, union columns, groups,
    kernel ms and wall ms; classes[(block == 256) + 2 * (W in LDS)] = the groups its first pass launched in each launch
    class, replayed = 1 when a failing downdate made the chunks run again"""
    return dict(_UPDOWN_INFO[0]) if _UPDOWN_INFO[0] is not None else None


_SPARSEINV_INFO = [None]


def _last_error():
    return _csx.lib().csx_last_error().decode("utf-8", "replace")


def sparseinv(L):
    """Z = inv(L L') on the pattern of the Cholesky factor L (cs_chol's: diagonal first and positive, rows ascending;
    list-backed or on the device), by the Takahashi recurrence: a device-backed `cs` with L's p and i whose x
    holds the lower triangle of the symmetric inverse at those positions, byte-equal to
        for j = n-1 .. 0, d = L(j,j), S = rows of column j below the diagonal in storage order:
            for i in S: Z(i,j) = (-sum_{k in S} L(k,j) * Zs(i,k)) / d          (Zs(a,b) = the stored Z(max(a,b), min(a,b)))
            Z(j,j) = (1/d - sum_{k in S} L(k,j) * Z(k,j)) / d
    with every product and sum rounded on its own.  L is not changed.  ValueError with the library's message for a matrix that
    is not such a factor (rectangular, no values, an empty column, a diagonal that is not first, positive and finite, rows out
    of order, a pattern that is not a Cholesky pattern).  sparseinv_info(): the last call's depths, widest depth, terms and
    kernel ms."""
    if not CS_CSC(L):
        raise ValueError("sparseinv: L must be a CSC matrix")
    t0 = time.perf_counter()
    h = _csx.new_handle()
    with _Resident(L) as dL:
        st = _csx.lib().csx_chol_inverse(dL.handle, h)
    if st == _csx.EINVAL:
        raise ValueError("sparseinv: " + _last_error())
    _csx.check(st, "csx_chol_inverse")
    _sparseinv_note("chol", L.n, t0)
    return _from_device(h, lambda nnz: max(nnz, 1))


def _sparseinv_note(kind, n, t0):
    d, w, t, ms = _csx.C.c_int32(0), _csx.C.c_int32(0), _csx.C.c_int64(0), _csx.C.c_double(0.0)
    _csx.check(_csx.lib().csx_chol_inverse_info(d, w, t, ms), "csx_chol_inverse_info")
    _SPARSEINV_INFO[0] = {"kind": kind, "n": n, "depths": d.value, "widest": w.value, "terms": t.value, "kernel_ms": ms.value,
                          "wall_ms": 1e3 * (time.perf_counter() - t0)}


def sparseinv_info():
    """the last sparseinv / sparseinv_ldl / sparseinv_lu's (or a solver's inverse / inverse_diag / inverse_at / inverse_entries')
    kind ("chol", "ldl" or "lu"), n, depths of the elimination forest (= launches unless runs of one-column depths were
    walked), columns in the widest depth, terms (sum of |S_j|^2), kernel ms and wall ms"""
    return dict(_SPARSEINV_INFO[0]) if _SPARSEINV_INFO[0] is not None else None


def sparseinv_ldl(L, d):
    """Z = inv(L D L') on the pattern of L: L unit lower triangular on a Cholesky pattern (diagonal first and
    stored, never read; rows ascending; list-backed or on the device), d the n pivots (a dvec, numpy array or list), every one
    finite and non-zero, of either sign.  A device-backed `cs` with L's p and i whose x holds the lower triangle of the
    symmetric inverse, byte-equal to
        for j = n-1 .. 0, S = rows of column j below the diagonal in storage order:
            for i in S: Z(i,j) = -sum_{k in S} L(k,j) * Zs(i,k)                (Zs(a,b) = the stored Z(max(a,b), min(a,b)))
            Z(j,j) = 1/d[j] - sum_{k in S} L(k,j) * Z(k,j)
    with every product and sum rounded on its own.  Nothing is changed.  ValueError with the library's message for input that
    is no such factor (sparseinv's cases; a zero, non-finite or short d).  A factor with static pivots is not backward stable
    and the recurrence inherits its growth: a large max |L| (ldlsol_factor(...).info()["max_abs_l"]) says when to distrust Z."""
    if not CS_CSC(L):
        raise ValueError("sparseinv_ldl: L must be a CSC matrix")
    t0 = time.perf_counter()
    dv = d if isinstance(d, dvec) else dvec(np.asarray(d, dtype=np.float64).ravel())
    h = _csx.new_handle()
    with _Resident(L) as dL:
        st = _csx.lib().csx_ldl_inverse(dL.handle, dv.handle, h)
    if st == _csx.EINVAL:
        raise ValueError("sparseinv_ldl: " + _last_error())
    _csx.check(st, "csx_ldl_inverse")
    _sparseinv_note("ldl", L.n, t0)
    return _from_device(h, lambda nnz: max(nnz, 1))


def sparseinv_lu(L, Ut):
    """Z = inv(L U), U = Ut', on the one pattern of L and Ut: L unit lower triangular on a Cholesky pattern, Ut
    on the same p and i with column j = row j of U, the pivot Ut(j,j) first, finite and non-zero (slusol_factor's factors).
    -> (ZL, ZUt), two device-backed `cs` on that pattern: ZL(i,j) = Z(i,j) and ZUt(i,j) = Z(j,i) for i >= j (the diagonal in
    both), byte-equal to
        for j = n-1 .. 0, d = Ut(j,j), S = rows of column j below the diagonal in storage order:
            for i in S: ZL(i,j) = -sum_{k in S} L(k,j) * Z(i,k);   ZUt(i,j) = (-sum_{k in S} Ut(k,j) * Z(k,i)) / d
            ZL(j,j) = ZUt(j,j) = 1/d - sum_{k in S} L(k,j) * ZUt(k,j)
    with every product and sum rounded on its own.  Nothing is changed.  ValueError with the library's message for input that
    is no such pair (sparseinv's cases; a Ut on another pattern; a zero or non-finite pivot).  A factor with static pivots is
    not backward stable and the recurrence inherits its growth: large max |L|, max |U| / min |d|
    (slusol_factor(...).info()["max_abs_l"]) say when to distrust Z."""
    if not CS_CSC(L) or not CS_CSC(Ut):
        raise ValueError("sparseinv_lu: L and Ut must be CSC matrices")
    t0 = time.perf_counter()
    hl, hu = _csx.new_handle(), _csx.new_handle()
    with _Resident(L) as dL, _Resident(Ut) as dU:
        st = _csx.lib().csx_slu_inverse(dL.handle, dU.handle, hl, hu)
    if st == _csx.EINVAL:
        raise ValueError("sparseinv_lu: " + _last_error())
    _csx.check(st, "csx_slu_inverse")
    _sparseinv_note("lu", L.n, t0)
    return _from_device(hl, lambda nnz: max(nnz, 1)), _from_device(hu, lambda nnz: max(nnz, 1))


def _inverse_at(who, ZL, ZUt, hrmap, hcmap, rows, cols):
    """Z(rmap[rows[t]], cmap[cols[t]]) for every t as a numpy array, read off the pattern of the device-backed ZL (and ZUt for
    the entries above the diagonal; None: Z symmetric) by csx_inverse_at; hrmap, hcmap: int-vector handles or H(0).
    ValueError naming how many pairs are not on the pattern, or for an index out of range."""
    rows, cols = _csx.i32(np.asarray(rows).ravel()), _csx.i32(np.asarray(cols).ravel())
    if rows.size != cols.size:
        raise ValueError("%s: rows and cols differ in length (%d, %d)" % (who, rows.size, cols.size))
    out = dvec(max(rows.size, 1))
    missing = _csx.C.c_int64(0)
    st = _csx.lib().csx_inverse_at(ZL._dev.handle, ZUt._dev.handle if ZUt is not None else _csx.H(0), hrmap, hcmap, rows.size,
                                   _csx.pi(rows), _csx.pi(cols), out.handle, missing)
    if st == _csx.EINVAL:
        raise ValueError("%s: %s" % (who, _last_error()))
    _csx.check(st, "csx_inverse_at")
    if missing.value:
        raise ValueError("%s: %d of %d pairs are not on the pattern of the factor" % (who, missing.value, rows.size))
    return out.numpy()[:rows.size]


def _entries_np(A):
    """(row, column) of every stored entry of A in storage order, as int32 arrays"""
    p, i = _pattern_np(A)
    return i, np.repeat(np.arange(A.n, dtype=np.int32), np.diff(p))


def _first_entries(M):
    """value of the first entry of every column of a device-backed matrix (csx_csc_diag) as a numpy array"""
    out = dvec(M.n)
    st = _csx.lib().csx_csc_diag(M._dev.handle, out.handle)
    if st == _csx.EINVAL:
        raise ValueError(_last_error())
    _csx.check(st, "csx_csc_diag")
    return out.numpy()


def _solve_blocks_sharded(comm, b, nrhs, rows_in, rows_out, solve_block):
    """A batch of right-hand sides sharded by column block over the ranks of `comm` (independent units, no
    collective inside a block's solve).  The root (rank 0) passes b, a dvec rows_in-by-K block (or a list: K = 1); the
    other ranks pass None and nrhs = K.  Rank r gets columns [r k, (r + 1) k), k = ceil(K / world), of b
    (csx_block_cols + csx_comm_scatter_blocks), solve_block(block: dvec rows_in-by-k) returns its dvec rows_out-by-k
    solutions (the same object when the solve is in place), which return to the root (csx_comm_gather_blocks).
    Returns on the root the rows_out-by-K block (b itself, overwritten, when rows_in == rows_out; a new dvec otherwise)
    and the host list to write back to, if b was one; (None, None) elsewhere.  Every column has the bits of the
    unsharded solve: a sharded solve IS the unsharded one column by column."""
    lib = _csx.lib()
    root = comm.rank == 0
    K = comm.broadcast_object((b.k if isinstance(b, dvec) else 1) if root else None, 0)
    if nrhs is not None and nrhs != K:
        raise ValueError("solve: nrhs does not match the root's block")
    db = bhost = None
    if root:
        db, bhost = _vec_in(b, rows_in, "b")
    k = (K + comm.world - 1) // comm.world
    mine = dvec(rows_in, k)
    packed = dvec(rows_in * k * comm.world) if root else None     # world blocks of rows_in x k, rank order; pad columns = 0

    def _slot(buf, rows, r):
        h = _csx.new_handle()
        _csx.check(lib.csx_vec_wrap(_csx.C.c_void_p(buf.device_ptr() + 8 * rows * k * r), rows * k, h), "csx_vec_wrap")
        return h

    if root:
        for r in range(comm.world):
            c0 = r * k
            kk = max(0, min(k, K - c0))
            if kk <= 0:
                continue
            # columns [c0, c0 + kk) of B -> block r of `packed` (its first kk columns when the last block is short)
            tmp = dvec(rows_in, kk)
            _csx.check(lib.csx_block_cols(db.handle, rows_in, K, c0, kk, tmp.handle, 0), "csx_block_cols")
            slot = _slot(packed, rows_in, r)
            _csx.check(lib.csx_block_cols(slot, rows_in, k, 0, kk, tmp.handle, 1), "csx_block_cols")
            _csx.free(slot)
    comm.scatter_vec_blocks(packed.handle if root else None, mine.handle, rows_in * k, 0)
    sol = solve_block(mine)
    back = packed if rows_out == rows_in else (dvec(rows_out * k * comm.world) if root else None)
    comm.gather_vec_blocks(sol.handle, back.handle if root else None, rows_out * k, 0)
    if not root:
        return None, None
    out = db if rows_out == rows_in else dvec(rows_out, K)
    for r in range(comm.world):
        c0 = r * k
        kk = max(0, min(k, K - c0))
        if kk <= 0:
            continue
        slot = _slot(back, rows_out, r)
        tmp = dvec(rows_out, kk)
        _csx.check(lib.csx_block_cols(slot, rows_out, k, 0, kk, tmp.handle, 0), "csx_block_cols")
        _csx.check(lib.csx_block_cols(out.handle, rows_out, K, c0, kk, tmp.handle, 1), "csx_block_cols")
        _csx.free(slot)
    return out, bhost


def cs_cholsol(order, A, b):
    """Solve A x = b, A symmetric positive definite, upper triangle used; b is
    overwritten (csparse.py:622-644).  b may be a list (one system) or a dvec
    n-by-k block (k systems, factor once)."""
    if not CS_CSC(A) or b is None:
        return False
    n = A.n
    if order == 0 and A.m == n and _meta(A)[1]:
        # natural order: S = cs_schol, N = cs_chol and the solve plan in one library call, S never leaving the device
        # (csx_cholsol_factor); the reference's driver is always exact
        fused = _cholsol_factor_fused(A, True)
        if fused is None:
            return False
        L, plan = fused
        try:
            if _cholsol_list_on_host(plan, b, n):
                return True
            db, bhost = _vec_in(b, n, "b")
            _csx.check(_csx.lib().csx_cholsol_solve(plan, db.handle, db.k), "csx_cholsol_solve")
        finally:
            _csx.free(plan)
        _write_back(bhost, db, n * db.k)
        return True
    S = cs_schol(order, A, _arrays=True)
    N = cs_chol(A, S) if S is not None else None
    if S is None or N is None:
        return False
    pinv = None if S.pinv is None else _csx.i32(S.pinv)
    plan = _csx.new_handle()
    with _Resident(N.L) as dL:
        _csx.check(_csx.lib().csx_cholsol_plan(dL.handle, _csx.pi(pinv), plan), "csx_cholsol_plan")
        try:
            if _cholsol_list_on_host(plan, b, n):
                return True
            db, bhost = _vec_in(b, n, "b")
            _csx.check(_csx.lib().csx_cholsol_solve(plan, db.handle, db.k), "csx_cholsol_solve")
        finally:
            _csx.free(plan)
    _write_back(bhost, db, n * db.k)
    return True


def _cholsol_factor_fused(A, exact):
    """csx_cholsol_factor: (L as a device-backed cs, plan handle), or None when A is not positive definite."""
    hL, hP = _csx.new_handle(), _csx.new_handle()
    with _Resident(A) as dA:
        st = _csx.lib().csx_cholsol_factor(dA.handle, 1 if exact else 0, hL, hP)
    if st in (_csx.ENOTSPD, _csx.EINVAL):        # not positive definite; an index out of range (cs_schol gives None for it)
        return None
    _csx.check(st, "csx_cholsol_factor")
    return _from_device(hL, lambda nnz: max(nnz, 1)), hP


def _symbolic_of_factor(L):
    """cs_schol(0, A)'s result read off the factor: S.cp = L.p; S.parent[j] = the first row below the diagonal of column j of L
    (csparse.py:1136-1169 builds the same tree from A); as int32 arrays."""
    dev = L._dev
    m, n, nnz, hv = dev.info()
    p = np.empty(n + 1, dtype=np.int32)
    i = np.empty(max(nnz, 1), dtype=np.int32)
    _csx.check(_csx.lib().csx_csc_download(dev.handle, _csx.pi(p), _csx.pi(i), None), "csx_csc_download")
    parent = np.full(n, -1, dtype=np.int32)
    has = np.diff(p) > 1
    parent[has] = i[p[:-1][has] + 1]
    S = css()
    S.pinv = None
    S.q = None
    S.parent = parent
    S.cp = p
    S.unz = S.lnz = int(p[n])
    return S


def cholsol_factor(A, order=0, exact=None):
    """Factor once for many solves: returns a solver `solve(b)` where b is a list or a
    dvec n-by-k block (overwritten).  The batched form of cs_cholsol (csparse.py:622-644).
    The order of a solve's operations:
    exact=None (default): by the kind of right-hand side.  A LIST -- the reference's data model, the drop-in contract --
      is solved with the reference's operations in the reference's order: bit-identical to cs_lsolve + cs_ltsolve on
      the same L.  A dvec BLOCK -- the caller has left the reference's data model for the batched one -- is solved in the
      rounding-equal order, inside the 1e-10 that BASELINE.json's north_star grants x[]: dense blocks go to the matrix
      cores (blocked TRSM with explicit tile inverses, refused when an inverse is large), a big elimination tree to the
      supernodal schedule.  (G-spd, 128 right-hand sides: 2.4 ms against 4.8; bcsstk16: 0.4 ms against 6.6.)
    exact=True: every solve, blocks too, bit-identical to the reference's order.   exact=False: every solve rounding-equal.
    cs_cholsol, the reference's own driver, is always exact.
    refactor(A2): new values on A's pattern with the analysis kept: L.x becomes the factor of A2, byte-equal to a
    fresh cholsol_factor(A2, order, exact)'s (to rounding only under "chol.exact" = 0 with exact other than True); False, and nothing changed, when A2 is not positive definite; ValueError for
    another pattern.  refactor_info(): the last refactor's route, launch counts and times.
    backward_error(x, b, A=None), refine(b, maxit=5, A=None), condest(A=None), operator_info(): the componentwise backward
    error of x, iterative refinement and a 1-norm condition estimate against the SYMMETRIC matrix in the upper triangle of the
    operator (_Refinable): the factored matrix or the last refactor's values, or A= for any other square matrix
    of order n -- a stale factor against a new matrix, or the matrix after update().  See the methods."""
    if not CS_CSC(A) or A.m != A.n:
        return None
    first_plan = None
    if order == 0 and A.m == A.n and _meta(A)[1]:
        # natural order: analysis, factorisation and plan in ONE library call, S never leaving the device (csx_cholsol_factor:
        # round 4's flow handed 40 MB of parent / cp to the host, back again, and re-read L twice to re-arrange it).  The plan
        # starts in the order blocks are solved in unless every solve is to be exact; a list switches it (a flag: the exact
        # kernel of a forest of equal blocks reads L.x itself).
        fused = _cholsol_factor_fused(A, exact is True)
        if fused is None:
            return None
        N = csn()
        N.L, first_plan = fused
        N.U, N.pinv, N.B = None, None, None
        S = None                                 # read off the factor when `symbolic` is asked for
        pinv = None
    else:
        S = cs_schol(order, A, _arrays=True)
        N = cs_chol(A, S) if S is not None else None
        if N is None:
            return None
        pinv = None if S.pinv is None else _csx.i32(S.pinv)
    # (the solver exposes S with lists, as cs_schol returns them -- made when `symbolic` is first read: at 5M columns the
    # three conversions take 0.3 s, sixty times the analysis itself)
    # The C plan BORROWS L's device arrays (CholPlan::L is not owned; the L' plan reads L.p / L.i / L.x directly),
    # so the factor must stay on the device for as long as the solver lives: N.L is pinned (reading F.L.p / .i / .x
    # copies to the host but keeps the device matrix), and the solver holds the _DevMatrix itself.
    cs_pin(N.L)
    dev = N.L._dev
    n = A.n
    start_exact = exact is True if first_plan is not None else exact is not False

    def _build():
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_cholsol_plan(dev.handle, _csx.pi(pinv), h), "csx_cholsol_plan")
        if not start_exact:
            _csx.check(_csx.lib().csx_cholsol_set_order(h, 0), "csx_cholsol_set_order")
        return h

    class _Solver(_SymRefinable):
        L = N.L

        @property
        def symbolic(self):
            nonlocal S
            if S is None:
                S = _symbolic_of_factor(N.L)
            return _symbolic_lists(S)

        def __init__(self):
            self._dev = dev                      # keeps the device factor alive (see above)
            self._built = dev.version
            self.plan_handle = first_plan if first_plan is not None else _build()
            self._exact_now = start_exact            # the order the plan is in
            self._box = [self.plan_handle]
            self._fin = weakref.finalize(self, lambda box: _csx.free(box[0]), self._box)
            self._rplan, self._rinfo = None, None    # refactor(): made by its first call
            self._A2 = A                             # the matrix the factor stands for: A, or the last refactor's A2
            self._stands = dev.version               # ... while the factor's version is this one (update / downdate move it)
            self._source = None                      # operator_info(): what the last measurement was taken against
            self._refine_init(A, n)

        def _solve_block(self, blk, trans, from_list):
            _csx.check(_csx.lib().csx_cholsol_solve(self._plan_for(not from_list), blk.handle, blk.k), "csx_cholsol_solve")
            return blk

        def _current(self):
            """The plan copies part of L's values (forward gather arrays, fragments): after cs_updown(F.L, ...) changed
            the factor in place it is rebuilt from the factor as it now stands."""
            if self._built != dev.version:
                _csx.free(self.plan_handle)
                self.plan_handle = self._box[0] = _build()
                self._exact_now = start_exact
                self._built = dev.version
            return self.plan_handle

        def _plan_for(self, block):
            """The plan in the order this right-hand side is solved in (see cholsol_factor): switching is a flag; the
            rounding-equal order's operands (tile inverses, supernodal schedule) are built the first time it is asked for."""
            h = self._current()
            want_exact = exact if exact is not None else not block
            if want_exact != self._exact_now:
                _csx.check(_csx.lib().csx_cholsol_set_order(h, 1 if want_exact else 0), "csx_cholsol_set_order")
                self._exact_now = want_exact
            return h

        def info(self):
            a, b, c = _csx.C.c_int32(), _csx.C.c_int32(), _csx.C.c_int32()
            _csx.check(_csx.lib().csx_cholsol_info(self._current(), a, b, c), "csx_cholsol_info")
            return {"fused_local": a.value in (1, 2, 3, 5), "dense_block": c.value if a.value in (2, 3) else 0,  # dense kernels in use
                    "matrix_cores": a.value in (3, 5), "trees": b.value, "max_nodes": c.value}

        def solve(self, b, comm=None, nrhs=None):
            """b: a list (one system) or a dvec n-by-k block, overwritten with the solutions.
            comm (a shard.Comm of more than one rank, every rank holding this same factor -- factored redundantly or
            shipped with comm.bcast_csc): the batch is sharded by right-hand-side block.  The root (rank 0)
            passes the n-by-K block, the other ranks pass None and nrhs = K; rank r solves columns [r k, (r + 1) k),
            k = ceil(K / world): blocks leave the root (csx_comm_scatter_blocks), every rank runs the sequence of
            csparse.py:640-643 on its block with no communication, the solutions return (csx_comm_gather_blocks) and
            the root's block is overwritten.  Every column has the bits of the unsharded solve."""
            if comm is not None and comm.world > 1:
                return self._solve_sharded(b, comm, nrhs)
            if not isinstance(b, dvec) and (exact is None or exact) and _cholsol_list_on_host(self._plan_for(False), b, n):
                return True
            db, bhost = _vec_in(b, n, "b")
            _csx.check(_csx.lib().csx_cholsol_solve(self._plan_for(isinstance(b, dvec)), db.handle, db.k), "csx_cholsol_solve")
            _write_back(bhost, db, n * db.k)
            return True

        def _updown(self, C, sigma):
            if not CS_CSC(C) or C.m != n:
                raise ValueError("update / downdate: C must be a CSC matrix with %d rows" % n)
            if pinv is not None and C.n > 0:      # L L' = P A P': rows of A are rows pinv[i] of L
                with _Resident(C) as dC:
                    h = _csx.new_handle()
                    st = _csx.lib().csx_permute(dC.handle, _csx.pi(pinv), None, 1, h)
                if st == _csx.EINVAL:
                    raise IndexError("list index out of range")
                _csx.check(st, "csx_permute")
                C = _from_device(h, lambda nnz: max(nnz, 1))
            sg = np.full(C.n, sigma, dtype=np.int32)
            if C.n == 0:
                _UPDOWN_INFO[0] = {"columns": 0, "applied": 0, "chunks": 0, "union_columns": 0, "groups": 0,
                                   "kernel_ms": 0.0, "wall_ms": 0.0}
                return True
            a = _updown_block_call(N.L, sg, C, None, 3)
            if a == -1:
                raise ValueError("update / downdate: a column of C reaches outside the pattern of L(:, f)")
            return a == C.n

        def update(self, C):
            """L L' + C C' in place (C: n-by-k CSC in A's row numbering; rows through pinv for order >= 1), in one pass
            (updown_block).  Every row of C(:,t) must lie in the pattern of L(:, f_t), f_t its first row in L's numbering
            (the factor's pattern does not change): ValueError otherwise, nothing changed.  True.  The plans are rebuilt
            from the new values at the next solve; updown_info() reports the call."""
            return self._updown(C, 1)

        def downdate(self, C):
            """L L' - C C' in place, as update(C).  All or nothing: False when a downdate is not positive definite, and then
            L.x and the solves are exactly as before."""
            return self._updown(C, -1)

        def updown_info(self):
            return updown_info()

        def inverse(self):
            """Z = inv(L L') on the pattern of L (sparseinv): a device-backed `cs` in L's numbering -- for order >= 1 its rows
            and columns are those of P A P' (symbolic.pinv maps A's).  Computed from the factor as it stands (after update /
            downdate / cs_updown: the new values); nothing is kept between calls."""
            return sparseinv(N.L)

        def inverse_diag(self):
            """diag(inv(A)) as a numpy array, entry i = inv(A)(i,i) in A's numbering"""
            d = _first_entries(self.inverse())
            return d if pinv is None else d[pinv]

        def logdet(self):
            """log det A = 2 sum_j log L(j,j), the sum correctly rounded (math.fsum)"""
            return 2.0 * math.fsum(np.log(_first_entries(N.L)).tolist())

        def refactor(self, A2):
            """New values on the kept analysis: A2 a CSC `cs` with A's exact pattern, or nnz(A) values in A's
            storage order (numpy, list or dvec), in A's own numbering whatever the order; ValueError for another pattern or
            length.  L.x becomes the factor of A2, byte-equal to a fresh cholsol_factor(A2, order, exact)'s under the options
            in force (under "chol.exact" = 0 with exact other than True: equal to rounding, the fresh factor's block kernel
            being the emitting one); L.p, L.i and the ordering stay.  True on success; False when A2 is not positive
            definite, and then L and the solves are exactly as before.  The first call makes the plan (a solver never
            refactored carries nothing of it); the solve plans are rebuilt from the new values at the next solve, as after
            update().  Legal after update / downdate / cs_updown: the refactor overwrites L from A2."""
            t0 = time.perf_counter()
            A2 = _refactor_input(A, A2)
            if self._rplan is None:
                h = _csx.new_handle()
                with _Resident(A) as dA:
                    _csx.check(_csx.lib().csx_chol_refactor_plan(dA.handle, dev.handle, _csx.pi(pinv), h),
                               "csx_chol_refactor_plan")
                self._rplan = h
                weakref.finalize(self, lambda hp, keep: _csx.free(hp), h, dev)   # (the plan borrows L: freed before dev can go)
            ok, info = _csx.C.c_int(0), np.zeros(8, dtype=np.int32)
            _refactor_call(A2, lambda h2: _csx.lib().csx_chol_refactor(self._rplan, h2, ok, _csx.pi(info)), ok)
            if ok.value:
                _refactored(N.L, dev)
                self._A2, self._stands, self._source = A2, dev.version, None
                self._operator_changed()
            num, call = _csx.C.c_double(0.0), _csx.C.c_double(0.0)
            _csx.check(_csx.lib().csx_chol_refactor_info(num, call), "csx_chol_refactor_info")
            self._rinfo = {"ok": bool(ok.value), "route": "forest" if info[0] else "general", "levels": int(info[1]),
                           "supernodes": int(info[2]), "trees": int(info[3]), "dense_trees": int(info[4]), "band": int(info[5]),
                           "first": bool(info[6]), "numeric_ms": num.value, "ms": 1e3 * (time.perf_counter() - t0)}
            win = _csx.C.c_int32(0)
            _csx.check(_csx.lib().csx_chol_refactor_window(self._rplan, win), "csx_chol_refactor_window")
            self._rwindow = int(win.value)
            return bool(ok.value)

        def refactor_info(self, window=False):
            """None before the first refactor; else the last one's ok, route ("general" / "forest"), levels (launches of the
            level walk), supernodes, trees, dense_trees, band (0 none, 1 register window, 2 blocked dense band), first (this
            call made the plan's scratch), numeric_ms (HIP events around the numeric kernels) and ms (the whole call).
            window=True adds "window": the register-window instance that refactor launched (48, 80, 112, 144 or 176; 0: none)."""
            if self._rinfo is None:
                return None
            return dict(self._rinfo, window=self._rwindow) if window else dict(self._rinfo)

        def _solve_sharded(self, b, comm, nrhs):
            # every rank solves in the order the ROOT's right-hand side asks for
            plan = self._plan_for(comm.broadcast_object(isinstance(b, dvec) if comm.rank == 0 else None, 0))

            def block(mine):
                _csx.check(_csx.lib().csx_cholsol_solve(plan, mine.handle, mine.k), "csx_cholsol_solve")
                return mine

            out, bhost = _solve_blocks_sharded(comm, b, nrhs, n, n, block)
            if out is not None:
                _write_back(bhost, out, n * out.k)
            return True

    return _Solver()


# ------------------------------------- what the static-pivot solvers share ----

def _symbolic_lists(S):
    """S with parent / cp / pinv as lists, as cs_schol returns them -- made when a solver's `symbolic` is first read: at 5M
    columns the three conversions take 0.3 s, sixty times the analysis itself"""
    for name in ("parent", "cp", "pinv"):
        v = getattr(S, name)
        if v is not None and not isinstance(v, list):
            setattr(S, name, v.tolist())
    return S


def _perturb_tau(perturb, norm, dev, values=None):
    """tau = perturb |M|_1 by the library's `norm` (csx_norm1_sym, csx_norm1), 0.0 for perturb == 0: M the device matrix dev, or
    its pattern with `values` (a dvec in its storage order; nothing is copied)"""
    if perturb == 0.0:
        return 0.0
    out = _csx.C.c_double(0.0)
    h = dev.handle if values is None else _wrap_values(dev, values)
    try:
        _csx.check(norm(h, out), norm.__name__)
    finally:
        if values is not None:
            _csx.free(h)
    return perturb * out.value


def _refactor_tau(perturb, norm, A, A2):
    """_perturb_tau of the operand of a refactor (_refactor_input's A2) of a factor of A"""
    if perturb == 0.0:
        return 0.0
    if isinstance(A2, cs):
        with _Resident(A2) as d2:
            return _perturb_tau(perturb, norm, d2)
    with _Resident(A) as dA:
        return _perturb_tau(perturb, norm, dA, A2)


def _adopt_factor(hF, hL, mats=(), vecs=()):
    """Python faces of the parts that a device factor hF lends out (its *_parts call): the wrappers free the plans cached on the
    matrices and the factor, never a part.  hL: the matrix whose wrapper frees the factor, after its plans; mats: further matrix
    handles, vecs: (handle, n, k) of dense parts -- both keep hL's wrapper alive.  -> [pinned `cs` of hL and of mats], [dvec]"""
    def pinned(h):
        M = cs_pin(_from_device(h, lambda nnz: max(nnz, 1)))
        M._dev._fin.detach()
        return M

    L = pinned(hL)
    dev = L._dev
    dev._fin = weakref.finalize(dev, lambda plans, h: (_DevMatrix._release(None, plans), _csx.free(h)), dev.plans, hF)
    Ms, vs = [L], []
    for h in mats:
        M = pinned(h)
        M._dev._fin = weakref.finalize(M._dev, _DevMatrix._release, None, M._dev.plans)
        M._dev._keep = dev
        Ms.append(M)
    for h, n, k in vecs:
        v = dvec(n, k, _handle=h)
        v._fin.detach()
        v._keep = dev
        vs.append(v)
    return Ms, vs


def _in_order(plans, in_exact_order, sweeps):
    """sweeps() with the triangular-solve plans in the reference's order (1) or the rounding-equal one (0); order 1 is put back
    whatever happens: the plans are shared with the list-level cs_lsolve / cs_ltsolve / cs_usolve / cs_utsolve on the same factors"""
    lib = _csx.lib()
    try:
        for plan in plans:
            _csx.check(lib.csx_tri_set_order(plan, 1 if in_exact_order else 0), "csx_tri_set_order")
        return sweeps()
    finally:
        for plan in plans:
            lib.csx_tri_set_order(plan, 1)


def _factor_info(hF, info_call, names, stats_call, stat_names, **more):
    """info() of ldlsol / schur / slusol / hqrsol_factor: the integers `names` of info_call, then the doubles stat_names of
    stats_call (both in the library's order), then `more`"""
    lib = _csx.lib()
    raw = (_csx.C.c_int64 * len(names))()
    st = (_csx.C.c_double * len(stat_names))()
    _csx.check(getattr(lib, info_call)(hF, raw), info_call)
    _csx.check(getattr(lib, stats_call)(hF, st), stats_call)
    out = {name: int(v) for name, v in zip(names, raw)}
    out.update(zip(stat_names, st))
    out.update(more)
    return out


class _LdlSolver(object):
    """What the solvers of ldlsol_factor and schur_factor share: both stand on one partial LDL' in the library (DESIGN.md §22, §25:
    the LDL' factor is the partial one with nothing kept).  The solver calls _ldl_init and names its entry points: _INFO, the
    names of the info[] layout, and _CALLS, the library's refactor / info / stats functions.  _after_refactor(A2): its own
    bookkeeping after a successful refactor."""

    _INFO, _CALLS = (), ()

    def _ldl_init(self, A, S, perturb, hF, N, dev):
        self._A, self._S, self._perturb, self._hF = A, S, perturb, hF
        self.factors = N
        self._dev = dev                              # keeps the parts and the factor alive

    @property
    def symbolic(self):
        return _symbolic_lists(self._S)

    def _after_refactor(self, A2):
        pass

    def refactor(self, A2):
        lib = _csx.lib()
        A2 = _refactor_input(self._A, A2)
        ok = _csx.C.c_int(0)
        tau = _refactor_tau(self._perturb, lib.csx_norm1_sym, self._A, A2)     # |S|_1 of the operand
        fn = getattr(lib, self._CALLS[0])
        _refactor_call(A2, lambda h2: fn(self._hF, h2, tau, ok), ok)
        if ok.value == 1:
            _refactored(self.factors.L, self._dev)
            self._after_refactor(A2)
        return ok.value == 1

    def info(self):
        return _factor_info(self._hF, self._CALLS[1], self._INFO, self._CALLS[2], ("min_abs_d", "max_abs_d", "max_abs_l"))

    def inertia(self):
        """(positive, negative) pivots of the committed factor (of A11 for a partial one)"""
        i = self.info()
        return i["pos"], i["neg"]

    def logdet(self):
        """(sign, log |det A|) (of A11 for a partial factor): the sign of the product of the pivots, and sum_j log |d_j|
        correctly rounded (math.fsum)"""
        d = self.factors.D.numpy().reshape(-1)
        sign = -1.0 if int(np.sum(d < 0.0)) % 2 else 1.0
        return sign, math.fsum(np.log(np.abs(d)).tolist())


# ------------------------------------------------------------------- LDL' ----

_LDL_INFO =("n", "lnz", "levels", "launches", "pos", "neg", "perturbed", "breakdown", "kernel_us", "level_launches",
             "run_launches", "long_columns", "window")


def ldlsol_factor(A, order=0, perturb=0.0, exact=None):
    """Factor a symmetric INDEFINITE matrix once for many solves: L D L' = P A P' with unit lower triangular L on the pattern
    of the Cholesky factor and diagonal D, 1x1 pivots in the static order of `order` (0 natural, 1 nested dissection), no
    pivot search.  A is read as cs_chol reads it: the stored entries with row <= column, of duplicates the
    last.  K - sigma M with sigma inside the spectrum, quasi-definite KKT systems: the route that today goes through
    lusol_factor.  Static pivoting is not backward stable by itself: follow solve() with refine() and read backward_error().
    perturb: a pivot with |d| < tau = perturb |S|_1 (csx_norm1_sym) is replaced by copysign(tau, d) and counted
    (info()["perturbed"]); 0.0 (default): none, and a zero or non-finite pivot is a breakdown.
    None for a non-CSC or non-square A, and None on breakdown.  Otherwise a solver:
    solve(b): b a list (one system) or a dvec n-by-k block, overwritten: cs_ipvec(pinv), cs_lsolve(L), X[i,:] /= d[i]
      (csx_block_div_rows), cs_ltsolve(L), cs_pvec(pinv), the two sweeps under lusol_factor's rule for `exact`: a list in the
      reference's order, a block in the rounding-equal order, True / False force one order for both.
    refactor(A2): new values on the kept analysis, A2 as for cholsol_factor's refactor: True; False with L, D and the solves
      exactly as before on breakdown; ValueError for another pattern or length.  L.x and d are byte-equal to a fresh
      ldlsol_factor(A2, order, perturb)'s.
    batch(values, perturb=None): B symmetric value sets on A's pattern factored together in one walk of the levels, with batched
      solves, the inertia and the log-determinant of every member (_LdlBatch): a shift or parameter sweep on one
      pattern; this factor is left as it is.
    backward_error(x, b, A=None), refine(b, maxit=5, A=None), condest(A=None), operator_info(): as on cholsol_factor (_SymRefinable).
    inertia(): (positive, negative) pivots = eigenvalues of A by Sylvester's law (exact arithmetic; perturbed pivots keep the
      sign they had).  logdet(): (sign, log |det A|), the sum correctly rounded.  info(): n, lnz, levels (height levels of the
      elimination tree), launches (numeric launches of the last run: level_launches of the wave-per-column kernel +
      run_launches of the one-workgroup walker of narrow levels), pos, neg, perturbed, breakdown (smallest broken column of the
      last run, -1 none), kernel_us, long_columns (columns of the last run that the kernels updated in place: longer than the LDS `window`), min_abs_d,
      max_abs_d, max_abs_l.  factors: .L (a pinned `cs`, unit diagonal stored) and .D (a dvec); symbolic: S.
    inverse(), inverse_at(rows, cols), inverse_diag(), inverse_entries(): entries of inv(A) on the pattern of L (sparseinv_ldl,
      DESIGN.md §26), computed from the factor as it stands.  A static-pivot factor is not backward stable and the recurrence
      inherits its growth, as solve() without refine() does: info()["max_abs_l"] says when to distrust them."""
    if not CS_CSC(A) or A.m != A.n:
        return None
    perturb = float(perturb)
    if not perturb >= 0.0:
        raise ValueError("ldlsol_factor: perturb must be >= 0")
    S = cs_schol(order, A, _arrays=True)
    if S is None:
        return None
    n = A.n
    pinv = None if S.pinv is None else _csx.i32(S.pinv)
    lib = _csx.lib()
    hF, ok = _csx.new_handle(), _csx.C.c_int(0)
    with _Resident(A) as dA:
        _csx.check(lib.csx_ldl_factor(dA.handle, _csx.pi(_csx.i32(S.parent)), _csx.pi(_csx.i32(S.cp)), _csx.pi(pinv),
                                      _perturb_tau(perturb, lib.csx_norm1_sym, dA), hF, ok), "csx_ldl_factor")
    if not ok.value:
        return None
    hL, hd = _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_ldl_parts(hF, hL, hd), "csx_ldl_parts")
    N = csn()
    (N.L,), (N.D,) = _adopt_factor(hF, hL, vecs=[(hd, n, 1)])
    dev = N.L._dev
    N.U, N.pinv, N.B = None, None, None
    hp, keep_p = _perm_handle(pinv, n)
    perturb_of_factor = perturb

    class _Solver(_LdlSolver, _SymRefinable):
        _INFO, _CALLS = _LDL_INFO, ("csx_ldl_refactor", "csx_ldl_info", "csx_ldl_stats")

        def __init__(self):
            self._ldl_init(A, S, perturb, hF, N, dev)
            self._fin = weakref.finalize(self, _csx.free, keep_p)
            self._A2, self._stands, self._source = A, dev.version, None
            self._refine_init(A, n)

        def _solve_block(self, blk, trans, from_list):
            return self._block(blk, exact if exact is not None else from_list)

        def _block(self, blk, in_exact_order):
            k = blk.k
            x = blk
            if pinv is not None:
                x = dvec(n, k)
                _csx.check(lib.csx_permute_vec(hp, blk.handle, x.handle, n, k, 1), "csx_permute_vec")
            p1, p2 = _plan(dev, TRI_L), _plan(dev, TRI_LT)

            def sweeps():
                _csx.check(lib.csx_tri_solve(p1, x.handle, k), "csx_tri_solve")
                _csx.check(lib.csx_block_div_rows(x.handle, hd, n, k), "csx_block_div_rows")
                _csx.check(lib.csx_tri_solve(p2, x.handle, k), "csx_tri_solve")

            _in_order((p1, p2), in_exact_order, sweeps)
            if pinv is not None:
                _csx.check(lib.csx_permute_vec(hp, x.handle, blk.handle, n, k, 0), "csx_permute_vec")
            return blk

        def solve(self, b):
            db, bhost = _vec_in(b, n, "b")
            self._block(db, exact if exact is not None else not isinstance(b, dvec))
            _write_back(bhost, db, n * db.k)
            return True

        def _after_refactor(self, A2):
            self._A2, self._stands, self._source = A2, dev.version, None
            self._operator_changed()

        def batch(self, values, perturb=None):
            """B value sets on A's pattern factored together on this factor's analysis -> an _LdlBatch (its docstring has the
            rest).  values: a dvec of nnz x B (read, not kept), a 2-D numpy array of that shape, or a list of B value arrays
            (copied), each in A's storage order and read as A is (entries with row <= column, of duplicates the last); perturb:
            defaults to this factor's.  ValueError for another row count, B = 0 or B over the limit.  This factor is not changed
            and goes on working; it must not be freed before the batch, which holds on to it."""
            pb = perturb_of_factor if perturb is None else float(perturb)
            if not pb >= 0.0:
                raise ValueError("ldlsol_factor.batch: perturb must be >= 0")
            return _LdlBatch(self, hF, _meta(A)[0], n, pb, values)

        # Entries of inv(A) on the pattern of L (sparseinv_ldl).  Each call reads the factor as it stands (after
        # refactor: the new values; after a refactor that broke down: the old ones) and keeps nothing.  Static pivoting is not
        # backward stable and the recurrence inherits the factor's growth, as solve() without refine() does: info()["max_abs_l"]
        # says when to distrust the entries.

        def inverse(self):
            """Z = inv(L D L') on the pattern of L: a device-backed `cs` in L's numbering (symbolic.pinv maps A's)"""
            return sparseinv_ldl(N.L, N.D)

        def inverse_at(self, rows, cols):
            """inv(A)(rows[t], cols[t]) in A's numbering as a numpy array; ValueError naming how many pairs are not on the
            pattern of L + L'"""
            return _inverse_at("ldlsol_factor.inverse_at", self.inverse(), None, hp, hp, rows, cols)

        def inverse_diag(self):
            """diag(inv(A)) as a numpy array, entry i = inv(A)(i,i) in A's numbering"""
            d = _first_entries(self.inverse())
            return d if pinv is None else d[pinv]

        def inverse_entries(self):
            """one value per stored entry q of A: inv(A)(row_q, col_q) (entries below the diagonal and duplicates get their
            symmetric or shared value); always on the pattern"""
            return self.inverse_at(*_entries_np(A))

    return _Solver()


# ------------------------------------------------- Schur complement ----

_SCHUR_INFO = ("n", "n1", "ns", "lnz", "levels", "launches", "level_launches", "run_launches", "schur_launches", "schur_chunks",
               "pos", "neg", "perturbed", "breakdown", "kernel_us", "long_columns", "window")


def _schur_order(A, keep, order):
    """perm (int32, new -> old): the interior indices first -- ascending (order 0) or by a nested dissection of the pattern of
    A(interior, interior) (order 1) -- then `keep` in the caller's order"""
    n = A.n
    inside = np.ones(n, dtype=bool)
    inside[keep] = False
    interior = np.flatnonzero(inside).astype(np.int32)
    n1 = len(interior)
    if order == 1 and n1 > 0:
        p, i = _pattern_np(A)
        cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(p))
        rows = i.astype(np.int64)
        both = inside[rows] & inside[cols]
        local = np.cumsum(inside) - 1                          # old index -> index among the interior
        sp = np.zeros(n1 + 1, dtype=np.int32)
        sp[1:] = np.cumsum(np.bincount(local[cols[both]], minlength=n1))
        si = _csx.i32(local[rows[both]])                       # (entries stay in column order: `local` is monotone)
        perm = np.empty(n1, dtype=np.int32)
        if _csx.load().csx_order_nd_host(n1, _csx.pi(sp), _csx.pi(si), _csx.pi(perm)) != _csx.OK:
            return None
        interior = interior[perm]
    return np.concatenate([interior, np.asarray(keep, dtype=np.int32)]).astype(np.int32)


def schur_factor(A, keep, order=0, perturb=0.0, exact=None):
    """Eliminate all of a symmetric matrix but the indices `keep` and return what is left: the partial L D L' of P A P' with the
    Schur complement S = A22 - A21 inv(A11) A12 of the kept set on the device.  A is read as cs_chol reads it
    (stored entries with row <= column, of duplicates the last).  keep: ns distinct indices; P numbers the n1 = n - ns interior
    indices first (order 0: ascending; 1: nested dissection of the pattern of A(interior, interior)), then keep in the caller's
    order.  P A P' = Lp blockdiag(D1, S) Lp' with Lp unit lower triangular -- its first n1 columns those of the LDL' of P A P',
    rows >= n1 included, its last ns columns those of the identity -- 1x1 pivots in that static order, no pivot search.
    perturb: as for ldlsol_factor, on the interior pivots.  Only an interior pivot can break down: a zero or non-finite diagonal
    of S is data.  None for a non-CSC or non-square A and on an interior breakdown; ValueError for duplicate or out-of-range
    keep or perturb < 0.  Otherwise a solver:
    schur: the ns-by-ns dvec S (symmetric, both triangles the same bytes).  factors: .L = Lp (a pinned `cs`), .D (dvec of n1).
    symbolic: the analysis of P A P' with .pinv.  keep: the list.
    condense(b): b a list of n or an n-by-k dvec, not modified -> (g, state): state an n-by-k dvec in the permuted order holding
      [inv(D1) inv(L11) b1; g], g = b2 - L21 inv(L11) b1 the right-hand side of S x2 = g (ns-by-k: a list for a list b, a dvec
      for a block): cs_ipvec(pinv), cs_lsolve(Lp), csx_block_div_rows on the first n1 rows.
    expand(state, x2): x2 ns-by-k (list, numpy or dvec) -> x in A's numbering (a list for a list x2, else an n-by-k dvec): rows
      >= n1 of a copy of state become x2, cs_ltsolve(Lp), cs_pvec(pinv).
    solve(b, interface): condense, x2 = interface(g as numpy ns-by-k), expand; b overwritten; True.  No dense solver is added:
      `interface` is the caller's solve of S x2 = g.
    The two sweeps follow lusol_factor's rule for `exact`: a list in the reference's order, a block in the rounding-equal order,
    True / False force one order for both.
    refactor(A2): new values on the kept analysis, as on ldlsol_factor: True; False with Lp, D, S and the solves exactly as before
      on an interior breakdown; ValueError for another pattern or length.
    inertia(): (positive, negative) pivots of A11; with the inertia of S it is A's (Haynsworth).  logdet(): (sign, log |det A11|).
    info(): n, n1, ns, lnz (of Lp), levels (of the interior tree), launches, level_launches, run_launches (the walker, cut at
      256 levels), schur_launches, schur_chunks ((column, chunk of `window` rows) pairs of the trailing-column kernel), pos, neg,
      perturbed, breakdown, kernel_us, long_columns, window, min_abs_d, max_abs_d, max_abs_l."""
    if not CS_CSC(A) or A.m != A.n:
        return None
    perturb = float(perturb)
    if not perturb >= 0.0:
        raise ValueError("schur_factor: perturb must be >= 0")
    if order not in (0, 1):
        return None
    n = A.n
    keep = [int(v) for v in keep]
    if any(v < 0 or v >= n for v in keep) or len(set(keep)) != len(keep):
        raise ValueError("schur_factor: keep must hold distinct indices of A")
    ns = len(keep)
    n1 = n - ns
    perm = _schur_order(A, keep, order)
    if perm is None:
        return None
    pinv = np.empty(n, dtype=np.int32)
    pinv[perm] = np.arange(n, dtype=np.int32)
    S = cs_schol(0, cs_symperm(A, pinv, False), _arrays=True)
    if S is None:
        return None
    S.pinv = pinv
    lib = _csx.lib()
    hF, ok = _csx.new_handle(), _csx.C.c_int(0)
    with _Resident(A) as dA:
        _csx.check(lib.csx_schur_factor(dA.handle, _csx.pi(_csx.i32(S.parent)), _csx.pi(_csx.i32(S.cp)), _csx.pi(pinv), n1,
                                        _perturb_tau(perturb, lib.csx_norm1_sym, dA), hF, ok), "csx_schur_factor")
    if not ok.value:
        return None
    hL, hd, hS = _csx.new_handle(), _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_schur_parts(hF, hL, hd, hS), "csx_schur_parts")
    N = csn()
    (N.L,), (N.D, Sd) = _adopt_factor(hF, hL, vecs=[(hd, n1, 1), (hS, ns, max(ns, 1))])
    dev = N.L._dev
    N.U, N.pinv, N.B = None, None, None
    hp, keep_p = _perm_handle(pinv, n)

    def tail(x, k):
        """a NEW handle (the caller frees it) of rows n1 .. n - 1 of the n-by-k block x: nothing is copied"""
        h = _csx.new_handle()
        _csx.check(lib.csx_vec_wrap(_csx.C.c_void_p(x.device_ptr() + 8 * n1 * k), ns * k, h), "csx_vec_wrap")
        return h

    class _Solver(_LdlSolver):
        _INFO, _CALLS = _SCHUR_INFO, ("csx_schur_refactor", "csx_schur_info", "csx_schur_stats")
        schur = Sd

        def __init__(self):
            self._ldl_init(A, S, perturb, hF, N, dev)
            self._fin = weakref.finalize(self, _csx.free, keep_p)
            self.keep = list(keep)

        def _sweep(self, kind, x, k, in_exact_order):
            plan = _plan(dev, kind)
            _in_order((plan,), in_exact_order, lambda: _csx.check(lib.csx_tri_solve(plan, x.handle, k), "csx_tri_solve"))

        def _condense(self, blk, in_exact_order):
            k = blk.k
            x = dvec(n, k)
            _csx.check(lib.csx_permute_vec(hp, blk.handle, x.handle, n, k, 1), "csx_permute_vec")
            self._sweep(TRI_L, x, k, in_exact_order)
            _csx.check(lib.csx_block_div_rows(x.handle, hd, n1, k), "csx_block_div_rows")
            g = dvec(ns, k)
            if ns:
                h = tail(x, k)
                try:
                    _csx.check(lib.csx_vec_copy(h, g.handle), "csx_vec_copy")
                finally:
                    _csx.free(h)
            return g, x

        def _expand(self, state, x2, in_exact_order, out=None):
            if not isinstance(state, dvec) or state.n != n:
                raise ValueError("expand: state is not a condense() of this factor")
            k = state.k
            x = state.copy()
            if ns:
                h = tail(x, k)
                try:
                    if isinstance(x2, dvec):
                        if x2.n * x2.k != ns * k:
                            raise ValueError("expand: x2 is not ns-by-k")
                        _csx.check(lib.csx_vec_copy(x2.handle, h), "csx_vec_copy")
                    else:
                        a = np.ascontiguousarray(np.asarray(x2, dtype=np.float64)).reshape(-1)
                        if a.size != ns * k:
                            raise ValueError("expand: x2 is not ns-by-k")
                        _csx.check(lib.csx_vec_write(h, _csx.pd(a), a.size), "csx_vec_write")
                finally:
                    _csx.free(h)
            self._sweep(TRI_LT, x, k, in_exact_order)
            out = dvec(n, k) if out is None else out
            _csx.check(lib.csx_permute_vec(hp, x.handle, out.handle, n, k, 0), "csx_permute_vec")
            return out

        def condense(self, b):
            from_list = not isinstance(b, dvec)
            db, _ = _vec_in(b, n, "b")
            g, state = self._condense(db, exact if exact is not None else from_list)
            return (g.numpy().reshape(-1).tolist() if from_list else g), state

        def expand(self, state, x2):
            from_list = isinstance(x2, list)
            x = self._expand(state, x2, exact if exact is not None else from_list)
            return x.numpy().reshape(-1).tolist() if from_list else x

        def solve(self, b, interface):
            from_list = not isinstance(b, dvec)
            in_exact_order = exact if exact is not None else from_list
            db, bhost = _vec_in(b, n, "b")
            g, state = self._condense(db, in_exact_order)
            x2 = np.asarray(interface(g.numpy().reshape(ns, db.k)), dtype=np.float64)
            self._expand(state, x2, in_exact_order, out=db)
            _write_back(bhost, db, n * db.k)
            return True

    return _Solver()


# -------------------------------------------------------------------- LU ----

def _cs_from_arrays(m, n, p, i, x):
    C = cs_spalloc(m, n, len(i), True, False)
    C.p, C.i, C.x = p, i if i else [0], x if x else [0.0]
    C.nzmax = max(len(i), 1) if i else 0
    return C


def cs_lu(A, S, tol):
    """Sparse LU with threshold partial pivoting, P A = L U (csparse.py:1370-1451).
    Host C++ (csx_lu_host): pivot search is serial and data dependent.  L has its unit
    diagonal first in every column, U its diagonal last -- what cs_lsolve / cs_usolve need."""
    if not CS_CSC(A) or S is None:
        return None
    if not _meta(A)[1]:        # asked of the device for a device-made A: no download, the device copy stays
        raise TypeError("'NoneType' object is not subscriptable")
    n = A.n
    if A.m != n:
        raise IndexError("list index out of range")
    if S.q is not None:
        # column k of the factorisation is column q[k] of A (csparse.py:1405): the same as factoring A Q in natural order
        Sq = css()
        Sq.q, Sq.pinv, Sq.lnz, Sq.unz = None, None, S.lnz, S.unz
        return cs_lu(cs_permute(A, None, S.q, True), Sq, tol)
    if n >= 4096 or A._dev is not None:
        # a batch of small independent blocks (block-diagonal up to a symmetric permutation) factors on the device,
        # one workgroup per block; anything else comes back with done = 0 and takes the host code below
        pinv = np.empty(max(n, 1), dtype=np.int32)
        hL, hU, done = _csx.new_handle(), _csx.new_handle(), _csx.C.c_int(0)
        with _Resident(A) as dA:             # ONE residency for both device attempts (an unpinned A is uploaded once)
            st = _csx.lib().csx_lu_blocks(dA.handle, float(tol), hL, hU, _csx.pi(pinv), done)
            if st == _csx.ENOTSPD:
                return None
            _csx.check(st, "csx_lu_blocks")
            if not done.value:
                # one connected matrix: columns scheduled by the column elimination tree, a lane per column (csx_lu_etree);
                # done = 0 again for anything but a shallow tree with short columns, which stays with the host loop
                st = _csx.lib().csx_lu_etree(dA.handle, float(tol), hL, hU, _csx.pi(pinv), done)
                if st == _csx.ENOTSPD:
                    return None
                _csx.check(st, "csx_lu_etree")
        if done.value:
            N = csn()
            N.L = _from_device(hL, lambda nnz: max(nnz, 1))
            N.U = _from_device(hU, lambda nnz: max(nnz, 1))
            N.pinv = pinv[:n].tolist()
            N.B = None
            return N
    p = _csx.i32(A.p[:n + 1])
    nnz = int(p[n])
    i, x = _csx.i32(A.i[:nnz]), _csx.f64(A.x[:nnz])
    C = _csx.C
    out = [C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(),
           C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()]
    pinv = np.empty(max(n, 1), dtype=np.int32)
    lib = _csx.load()
    st = lib.csx_lu_host(n, _csx.pi(p), _csx.pi(i), _csx.pd(x), float(tol), *[C.byref(o) for o in out], _csx.pi(pinv))
    if st == _csx.ENOTSPD:
        return None
    _csx.check(st, "csx_lu_host")
    try:
        Lp = np.ctypeslib.as_array(out[0], shape=(n + 1,)).tolist()
        Up = np.ctypeslib.as_array(out[3], shape=(n + 1,)).tolist()
        lnz, unz = Lp[n], Up[n]
        Li = np.ctypeslib.as_array(out[1], shape=(max(lnz, 1),))[:lnz].tolist()
        Lx = np.ctypeslib.as_array(out[2], shape=(max(lnz, 1),))[:lnz].tolist()
        Ui = np.ctypeslib.as_array(out[4], shape=(max(unz, 1),))[:unz].tolist()
        Ux = np.ctypeslib.as_array(out[5], shape=(max(unz, 1),))[:unz].tolist()
    finally:
        for o in out:
            lib.csx_host_free(C.cast(o, C.c_void_p))
    N = csn()
    N.L = _cs_from_arrays(n, n, Lp, Li, Lx)
    N.U = _cs_from_arrays(n, n, Up, Ui, Ux)
    N.pinv = pinv[:n].tolist()
    N.B = None
    return N


def cs_lusol(order, A, b, tol):
    """Solve A x = b by LU; b is overwritten (csparse.py:1456-1478): host factorisation, then
    x = b(p); L\\x; U\\x; b(q) = x with the triangular solves on the device."""
    if not CS_CSC(A) or b is None:
        return False
    n = A.n
    S = cs_sqr(order, A, False)
    N = cs_lu(A, S, tol) if S is not None else None
    if S is None or N is None:
        return False
    x = dvec(n, b.k) if isinstance(b, dvec) else xalloc(n)      # b: a list (one system) or a dvec n-by-k block (k systems)
    cs_ipvec(N.pinv, b, x, n)
    cs_lsolve(N.L, x)
    cs_usolve(N.U, x)
    cs_ipvec(S.q, x, b, n)
    return True


def _condest(norm_a, solve, n):
    """cond_1(A) = |A|_1 |A^-1|_1 estimated with |A|_1 = norm_a and Hager-Higham's estimator of |A^-1|_1 as LAPACK's dlacn2
    runs it (Higham 1988, ITMAX = 5): solve(v, trans) returns A^-1 v (trans False) or A^-T v (trans True) for a numpy
    n-vector.  sign(0) = +1; ties of the largest |z_j| go to the lowest j.  0.0 for n = 0."""
    if n == 0:
        return 0.0

    def sgn(v):
        return np.where(v >= 0.0, 1.0, -1.0)

    y = solve(np.full(n, 1.0 / n), False)
    if n == 1:
        return float(norm_a) * abs(float(y[0]))
    est = float(np.sum(np.abs(y)))
    xi = sgn(y)
    j = int(np.argmax(np.abs(solve(xi, True))))
    it = 2
    while True:
        e = np.zeros(n)
        e[j] = 1.0
        y = solve(e, False)
        est_old, est = est, float(np.sum(np.abs(y)))
        s = sgn(y)
        if np.array_equal(s, xi) or est <= est_old:      # repeated sign vector: converged; no increase: cycling
            break
        xi = s
        z = solve(xi, True)
        j_last, j = j, int(np.argmax(np.abs(z)))
        if z[j_last] != abs(z[j]) and it < 5:
            it += 1
            continue
        break
    alt = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + np.arange(n) / (n - 1.0))
    temp = 2.0 * (float(np.sum(np.abs(solve(alt, False)))) / (3.0 * n))
    return float(norm_a) * max(est, temp)


def _refactor_input(A, A2):
    """A2 of a refactor of a factor of A: a CSC `cs` with A's m, n and entry count (its pattern is compared with A's on the
    device) or nnz(A) values in A's storage order (numpy, list or dvec; copied).  ValueError otherwise."""
    nnz = _meta(A)[0]
    if isinstance(A2, cs):
        if not CS_CSC(A2) or A2.m != A.m or A2.n != A.n or _meta(A2) != (nnz, True):
            raise ValueError("refactor: A2 does not have the pattern of the factored matrix")
        return A2
    v = A2.copy() if isinstance(A2, dvec) else dvec(np.asarray(A2, dtype=np.float64).ravel())
    if v.n * v.k != nnz:
        raise ValueError("refactor: %d values given, the factored matrix has %d entries" % (v.n * v.k, nnz))
    return v


def _refactor_call(A2, fn, ok):
    """fn(handle of A2) -> status; ok = -1 after it: A2's pattern or length is not A's -> ValueError"""
    if isinstance(A2, dvec):
        st = fn(A2.handle)
    else:
        with _Resident(A2) as d:
            st = fn(d.handle)
    _csx.check(st, "refactor")
    if ok.value == -1:
        raise ValueError("refactor: A2 does not have the pattern of the factored matrix")


def _refactored(M, dev):
    """The values behind `cs` M (device copy dev) were replaced by a refactor: the triangular-solve plans cached on it hold the
    old ones and go (solvers re-plan), and host lists already read from it are updated in place, as cs_updown does."""
    for h in dev.plans.values():
        _csx.free(h)
    dev.plans.clear()
    dev.version += 1
    if not M._lazy and M._x is not None:
        _, _, nnz, _ = dev.info()
        x = np.empty(max(nnz, 1), dtype=np.float64)
        _csx.check(_csx.lib().csx_csc_download(dev.handle, None, None, _csx.pd(x)), "csx_csc_download")
        M._x[:nnz] = x[:nnz].tolist()


def _wrap_values(dev, values):
    """a NEW handle (the caller frees it) of the pattern of the device matrix dev with the values of the dvec `values` in its
    storage order: nothing is copied, dev and values must outlive it"""
    C = _csx.C
    m, n, nnz, _ = dev.info()
    dp, di, dx = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _csx.check(_csx.lib().csx_csc_ptrs(dev.handle, dp, di, dx), "csx_csc_ptrs")
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_wrap(m, n, nnz, dp, di, C.c_void_p(values.device_ptr()), h), "csx_csc_wrap")
    return h


def _refactor_norm(A, A2):
    """cs_norm of the matrix a refactor installed, for condest(): A2 when it is a `cs`; else A's pattern with the values A2
    (a dvec in A's storage order) -- column sums on the device over A's pattern, nothing copied to the host"""
    if isinstance(A2, cs):
        return cs_norm(A2)
    with _Resident(A) as dA:
        h = _wrap_values(dA, A2)
        try:
            out = _csx.C.c_double(0.0)
            _csx.check(_csx.lib().csx_norm1(h, out), "csx_norm1")
        finally:
            _csx.free(h)
    return out.value


class _Refinable(object):
    """backward_error() and refine() of the solvers of lusol_factor and btf_factor, measured against the matrix
    the solver stands for: A, or the values of the last successful refactor() on A's pattern (self._A2).  The solver calls
    _refine_init(A, n), gives _solve_block(blk, trans, from_list) -- its own solve of a dvec block under its own order rule --
    and calls _operator_changed() after a successful refactor.  _residual_into(hA, dX, dB, dR, k, trans) -> (omega, rnorm) is
    the residual of that operator: csx_residual_block here; the cholsol solver, whose operator is the symmetric matrix in the
    upper triangle, gives csx_residual_sym_block."""

    EPS = 2.0 ** -52
    _residual_into = staticmethod(_residual_into)

    def _refine_init(self, A, n):
        self._rA, self._rn = A, n
        self._op = {"handle": None, "keep": None}     # A's pattern wrapped with the refactor's values (a dvec), while they hold
        self._operator_builds = 0
        weakref.finalize(self, lambda op: _csx.free(op["handle"]), self._op)

    def _operator_changed(self):
        _csx.free(self._op["handle"])
        self._op["handle"], self._op["keep"] = None, None

    @contextlib.contextmanager
    def _operator(self):
        """the handle of the matrix the solver stands for"""
        A2 = self._A2
        if isinstance(A2, cs):
            with _Resident(A2) as d:
                yield d.handle
            return
        if self._op["handle"] is None:
            # kept until the next successful refactor: the row gather cached on it is built once per set of values
            A = self._rA
            dev = A._dev if A._dev is not None else _DevMatrix(_upload(A))
            self._op["handle"], self._op["keep"] = _wrap_values(dev, A2), (dev, A2)
            self._operator_builds += 1
        yield self._op["handle"].value

    def backward_error(self, x, b, trans=False):
        """omega of x as a solution of A x = b (trans: A' x = b) per column, a float for one host vector"""
        return self._backward_error(x, b, trans, self._operator())

    def _backward_error(self, x, b, trans, operator):
        n = self._rn
        X, xrows, k = _block_shape(x)
        B, brows, kb = _block_shape(b)
        if k != kb or k < 1:
            raise ValueError("backward_error: x and b have different numbers of columns")
        if xrows < n or brows < n:
            raise IndexError("list index out of range")
        single = not isinstance(x, dvec) and X.ndim == 1
        dX = X if isinstance(X, dvec) else dvec(X)
        dB = B if isinstance(B, dvec) else dvec(B)
        with operator as hA:
            omega, _ = self._residual_into(hA, dX, dB, None, k, trans)
        return float(omega[0]) if single else omega

    def refine(self, b, maxit=5, trans=False):
        """solve, then at most maxit steps of iterative refinement on the columns whose backward error is above 2^-52; b is
        overwritten with x.  A step is kept only where it lowers the column's omega (strictly), and a column stops once a
        step fails to halve it: omega <= omega0 always, a rejected step leaves the column bit for bit as it was."""
        return self._refine(b, maxit, trans, self._operator())

    def _refine(self, b, maxit, trans, operator):
        n, eps, trans = self._rn, self.EPS, bool(trans)
        db, bhost = _vec_in(b, n, "b")
        k = db.k
        from_list = not isinstance(b, dvec)
        lib = _csx.lib()

        def mask(v):
            return _csx.pi(_csx.i32(v))

        B = db.copy()
        X = db
        with operator as hA, np.errstate(invalid="ignore"):
            self._solve_block(X, trans, from_list)
            R = dvec(n, k)
            w, rn = self._residual_into(hA, X, B, R, k, trans)
            w0 = w.copy()
            steps, solves = np.zeros(k, dtype=np.int64), 1
            live = w > eps                                   # a NaN column is never live
            Xc = Rc = D = None
            for _ in range(int(maxit)):
                if not live.any():
                    break
                if Xc is None:
                    Xc, Rc, D = dvec(n, k), dvec(n, k), dvec(n, k)
                _csx.check(lib.csx_vec_copy(R.handle, D.handle), "csx_vec_copy")
                self._solve_block(D, trans, from_list)
                solves += 1
                _csx.check(lib.csx_block_add_cols(X.handle, D.handle, Xc.handle, n, k, mask(live)), "csx_block_add_cols")
                wc, rnc = self._residual_into(hA, Xc, B, Rc, k, trans)
                accept = live & (wc < w)
                if accept.any():
                    _csx.check(lib.csx_block_select_cols(Xc.handle, X.handle, n, k, mask(accept)), "csx_block_select_cols")
                    _csx.check(lib.csx_block_select_cols(Rc.handle, R.handle, n, k, mask(accept)), "csx_block_select_cols")
                steps += accept
                live = accept & (wc > eps) & (2.0 * wc <= w)
                w, rn = np.where(accept, wc, w), np.where(accept, rnc, rn)
        _write_back(bhost, db, n * k)
        return {"omega0": w0, "omega": w, "rnorm": rn, "steps": steps, "solves": solves}

    def solve_grad(self, x, gx, trans=False, refine=0):
        """(gb, gA): the gradient of a scalar loss through x = A^-1 b (trans: A'^-1 b) with respect to b and to the stored
        entries of A.  x: the solution block solve() gave; gx: the loss gradient with respect to x, same
        shape, not modified.  gb = Lambda, the adjoint solution A' Lambda = gx (trans: A Lambda = gx), a NEW dvec block made by
        one solve of this solver in the other direction, in the order a solve of gx would take (refine > 0: by
        refine(maxit=refine) in that direction instead).  gA: a NEW dvec of nnz doubles on the pattern of the factored matrix,
        in its storage order -- what refactor(values) takes --, gA[q] = -sum_c Lambda[i_q, c] x[j_q, c] (trans: -sum_c x[i_q, c]
        Lambda[j_q, c]) by outer_on_pattern.  One host vector in gives 1-D numpy arrays out.  ValueError for unequal k,
        IndexError for short blocks."""
        return self._solve_grad(x, gx, bool(trans), refine, self._rA, self._operator, False)

    def _solve_grad(self, x, gx, trans, refine, pattern, operator, sym):
        """pattern: the `cs` whose stored entries gA is about; operator: a callable that gives the context manager of the
        operator's handle (taken only by refine > 0)"""
        n = self._rn
        X, xrows, k = _block_shape(x)
        G, grows, kg = _block_shape(gx)
        if k != kg or k < 1:
            raise ValueError("solve_grad: x and gx have different numbers of columns")
        if xrows < n or grows < n:
            raise IndexError("list index out of range")
        single = not isinstance(x, dvec) and not isinstance(gx, dvec) and X.ndim == 1 and G.ndim == 1
        gb = gx.copy() if isinstance(gx, dvec) else dvec(G[:n])
        adjoint = False if sym else not trans          # S = S': the symmetric solvers have one direction
        if int(refine) > 0:
            self._refine(gb, int(refine), adjoint, operator())
        else:
            self._solve_block(gb, adjoint, not isinstance(gx, dvec))
        dX = X if isinstance(X, dvec) else dvec(X)
        U, V = (dX, gb) if trans else (gb, dX)
        gA = outer_on_pattern(pattern, U, V, alpha=-1.0, sym=sym)
        return (gb.numpy().reshape(-1)[:n], gA.numpy()) if single else (gb, gA)

    def gmres(self, b, restart=16, maxit=64, inner_tol=2.0 ** -26, trans=False):
        """solve, then restarted GMRES with this factor as the preconditioner on the columns whose backward error is above
        2^-52; b is overwritten with x.  Where refine() needs the factor to contract, this needs only a Krylov
        space that holds the correction: a factor that differs from A by rank p ends in p + 1 inner steps.  Every column is its
        own system.  restart: inner steps of a cycle (the basis takes restart blocks of b's size on the device; MemoryError
        with the byte count when they cannot be had); maxit: inner steps per column at most (0: solve() and the backward
        error); inner_tol: a column leaves its cycle once the Arnoldi estimate of its residual is below inner_tol times the
        cycle's first residual.  The true residual is recomputed after every cycle and the cycle is kept only where it lowers
        the column's omega (strictly): omega <= omega0 always, a refused cycle leaves the column bit for bit as it was and
        stops it.  refine()'s dict, and iters (inner steps per column), cycles (accepted cycles per column; steps is the same
        array), resid_est (the last Arnoldi estimate over the cycle's first residual; 1.0 before any step).  ValueError for
        restart < 1, maxit < 0, or inner_tol outside (0, 1)."""
        return self._gmres(b, restart, maxit, inner_tol, trans, self._operator)

    def _gmres(self, b, restart, maxit, inner_tol, trans, operator):
        """operator: a callable that gives the context manager of the operator's handle (taken after the arguments are
        checked)"""
        m, maxit, tol = int(restart), int(maxit), float(inner_tol)
        if m < 1 or m > 0x7FFFFFFE:
            raise ValueError("gmres: restart must be at least 1 (and a 32-bit count of blocks)")
        if maxit < 0:
            raise ValueError("gmres: maxit must not be negative")
        if not 0.0 < tol < 1.0:
            raise ValueError("gmres: inner_tol must lie in (0, 1)")
        n, eps, trans = self._rn, self.EPS, bool(trans)
        db, bhost = _vec_in(b, n, "b")
        k = db.k
        from_list = not isinstance(b, dvec)
        lib = _csx.lib()

        def mask(v):
            return _csx.pi(_csx.i32(v))

        B = db.copy()
        X = db
        with operator() as hA, np.errstate(all="ignore"):
            self._solve_block(X, trans, from_list)
            R = dvec(n, k)
            w, rn = self._residual_into(hA, X, B, R, k, trans)
            w0 = w.copy()
            iters, cycles, solves = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64), 1
            est = np.ones(k)
            live = w > eps                                   # a NaN column is never live
            space = None
            while (live & (iters < maxit)).any():
                if space is None:
                    space = _GmresSpace(n, k, m)
                V, Vj, work, Z, Wb, Zero, Xc, Rc = space.blocks
                cyc = live & (iters < maxit)
                # beta = sqrt(ordered sum r r);  V_0 = r / beta
                _csx.check(lib.csx_block_select_cols(R.handle, Vj[0].handle, n, k, mask(cyc)), "csx_block_select_cols")
                beta = np.full(k, np.nan)
                _csx.check(lib.csx_gs_project(V.handle, 1, R.handle, work.handle, n, k, mask(cyc), 0, _csx.pd(beta)),
                           "csx_gs_project")
                beta = np.sqrt(beta)
                cyc &= np.isfinite(beta) & (beta > 0.0)      # r r under- or overflowed: the column stops
                live &= cyc
                if not cyc.any():
                    break
                _csx.check(lib.csx_gs_scale(R.handle, V.handle, 0, work.handle, n, k, mask(cyc), _csx.pd(beta)), "csx_gs_scale")
                arn = [_Arnoldi(m, float(beta[c])) if cyc[c] else None for c in range(k)]
                act = cyc.copy()
                for j in range(m):
                    if not act.any():
                        break
                    # Z = M^-1 V_j;  Wb = 0 - A Z (exactly -(A Z): the two calls that read it first take the sign up)
                    _csx.check(lib.csx_vec_copy(Vj[j].handle, Z.handle), "csx_vec_copy")
                    self._solve_block(Z, trans, from_list)
                    solves += 1
                    self._residual_into(hA, Z, Zero, Wb, k, trans)
                    nv, am = j + 1, mask(act)
                    h1, h2, nrm2 = np.zeros((nv, k)), np.zeros((nv, k)), np.zeros(k)
                    _csx.check(lib.csx_gs_project(V.handle, nv, Wb.handle, work.handle, n, k, am, 1, _csx.pd(h1)), "csx_gs_project")
                    _csx.check(lib.csx_gs_update(V.handle, nv, Wb.handle, work.handle, n, k, am, 1, _csx.pd(h1), _csx.pd(nrm2)),
                               "csx_gs_update")
                    _csx.check(lib.csx_gs_project(V.handle, nv, Wb.handle, work.handle, n, k, am, 0, _csx.pd(h2)), "csx_gs_project")
                    _csx.check(lib.csx_gs_update(V.handle, nv, Wb.handle, work.handle, n, k, am, 0, _csx.pd(h2), _csx.pd(nrm2)),
                               "csx_gs_update")
                    hnext = np.sqrt(nrm2)
                    stay = act.copy()
                    for c in np.flatnonzero(act):
                        iters[c] += 1
                        left = arn[c].step(h1[:, c] + h2[:, c], float(hnext[c]), tol)
                        est[c] = arn[c].estimate
                        stay[c] = not (left or iters[c] >= maxit)
                    if j + 1 < m and stay.any():
                        _csx.check(lib.csx_gs_scale(Wb.handle, V.handle, j + 1, work.handle, n, k, mask(stay), _csx.pd(hnext)),
                                   "csx_gs_scale")
                    act = stay
                # U = V y;  D = M^-1 U;  the candidate, its true residual, and the acceptance rule of refine()
                length = np.array([a.length if a is not None else 0 for a in arn], dtype=np.int32)
                y = np.zeros((int(length.max()), k))
                for c in np.flatnonzero(cyc):
                    y[:length[c], c] = arn[c].solution()
                _csx.check(lib.csx_gs_combine(V.handle, y.shape[0], Z.handle, work.handle, n, k, mask(cyc), _csx.pd(y),
                                              _csx.pi(length)), "csx_gs_combine")
                self._solve_block(Z, trans, from_list)
                solves += 1
                _csx.check(lib.csx_block_add_cols(X.handle, Z.handle, Xc.handle, n, k, mask(cyc)), "csx_block_add_cols")
                wc, rnc = self._residual_into(hA, Xc, B, Rc, k, trans)
                accept = cyc & (wc < w)
                if accept.any():
                    _csx.check(lib.csx_block_select_cols(Xc.handle, X.handle, n, k, mask(accept)), "csx_block_select_cols")
                    _csx.check(lib.csx_block_select_cols(Rc.handle, R.handle, n, k, mask(accept)), "csx_block_select_cols")
                cycles += accept
                live = accept & (wc > eps)
                w, rn = np.where(accept, wc, w), np.where(accept, rnc, rn)
        _write_back(bhost, db, n * k)
        return {"omega0": w0, "omega": w, "rnorm": rn, "steps": cycles, "cycles": cycles, "iters": iters, "solves": solves,
                "resid_est": est}


class _Arnoldi(object):
    """one column's Hessenberg matrix under its Givens rotations, in plain double operations: column j comes in
    as (h[0 .. j], hnext); the rotations so far are applied to it, a new one (c, s) = (a, b) / sqrt(a a + b b) (no hypot;
    (1, 0) when both are zero) clears hnext and turns g; |g[j + 1]| estimates the residual"""

    def __init__(self, m, beta):
        self.R = np.zeros((m, m))
        self.cs, self.sn = np.zeros(m), np.zeros(m)
        self.g = np.zeros(m + 1)
        self.g[0] = self.beta = beta
        self.length, self.estimate = 0, 1.0

    def step(self, h, hnext, tol):
        """-> whether the column leaves its cycle: the estimate is at most tol beta, or hnext is zero (or no number)"""
        j, R, g = self.length, self.R, self.g
        col = np.array(h, dtype=np.float64)
        for i in range(j):
            a, b2 = col[i], col[i + 1]
            col[i] = self.cs[i] * a + self.sn[i] * b2
            col[i + 1] = self.cs[i] * b2 - self.sn[i] * a
        a, b2 = col[j], hnext
        d = np.sqrt(a * a + b2 * b2)
        c, s = (1.0, 0.0) if d == 0.0 else (a / d, b2 / d)
        col[j] = c * a + s * b2
        g[j + 1] = -(s * g[j])
        g[j] = c * g[j]
        self.cs[j], self.sn[j] = c, s
        R[:j + 1, j] = col
        self.length = j + 1
        self.estimate = abs(g[j + 1]) / self.beta
        return bool(abs(g[j + 1]) <= tol * self.beta) or not hnext > 0.0

    def solution(self):
        """y of the rotated triangle: back substitution, the terms of a row subtracted in ascending order"""
        jl, R = self.length, self.R
        y = np.zeros(jl)
        for i in range(jl - 1, -1, -1):
            s = self.g[i]
            for l in range(i + 1, jl):
                s = s - R[i, l] * y[l]
            y[i] = s / R[i, i]
        return y


class _GmresSpace(object):
    """the device blocks of one gmres() call, allocated once: the basis (one vector of `restart` blocks, and a view of every
    block), the work vector of the csx_gs_* calls, Z (the block a solve runs in), Wb (the product), a zero right-hand side, the
    candidate and its residual"""

    def __init__(self, n, k, m):
        count = n * k
        nbytes = 8 * (count * (m + 5) + _csx.gs_work_len(n, k, m))
        try:
            V = dvec(count * m)
            base = V.device_ptr() or 0
            views = []
            for j in range(m):
                h = _csx.new_handle()
                _csx.check(_csx.lib().csx_vec_wrap(base + 8 * count * j, count, h), "csx_vec_wrap")
                views.append(dvec(n, k, _handle=h))
            work = dvec(_csx.gs_work_len(n, k, m))
            rest = [dvec(n, k) for _ in range(5)]
        except _csx.CsxError as e:
            raise MemoryError("gmres: cannot allocate the basis of %d blocks and its work space, %d bytes (%s)" % (m, nbytes, e))
        self.blocks = [V, views, work] + rest


EIG_PIVOT = 2.0 ** -20     # a pivot of the scaled Cholesky factor below this in the first pass: the block is dependent (§29)


def _eig_dense(what, *args):
    """The small dense steps of eigsh(), in numpy on the host; the restated loop of the tests calls this very
    function, so the two runs differ in the block operations alone.
    "cholqr", G (b x b, the Gram matrix of a block in the M inner product), first (the first of the two passes)
        -> (R, inv(R)) with R'R = G, or None on breakdown: G is taken as its upper triangle mirrored and scaled to a unit
        diagonal by d = 1 / sqrt(diag G); L = cholesky; R = L' diag(1 / d).  Breakdown: a diagonal entry of G that is not
        positive or not finite, a Cholesky factorisation that fails, or (first pass) a pivot of L below EIG_PIVOT.
    "ritz", T (m x m, block upper triangle filled), B (the sub-diagonal block that follows T, or None after a breakdown)
        -> (theta, S, estimate): eigh of T's upper triangle mirrored, ordered by descending |theta| (stable);
        estimate[c] = |B S[last rows, c]|_2 / |theta[c]| (0 with no B)."""
    with np.errstate(all="ignore"):
        if what == "cholqr":
            G, first = np.asarray(args[0], dtype=np.float64), bool(args[1])
            G = np.triu(G) + np.triu(G, 1).T
            d0 = np.diag(G).copy()
            if not (np.isfinite(d0).all() and (d0 > 0.0).all()):
                return None
            d = 1.0 / np.sqrt(d0)
            Gs = G * d[:, None] * d[None, :]
            if not np.isfinite(Gs).all():
                return None
            try:
                L = np.linalg.cholesky(Gs)
            except np.linalg.LinAlgError:
                return None
            piv = np.diag(L)
            if not np.isfinite(L).all() or not (piv > 0.0).all() or (first and piv.min() < EIG_PIVOT):
                return None
            R = L.T * (1.0 / d)[None, :]
            Rinv = np.linalg.solve(R, np.eye(R.shape[0]))
            return np.ascontiguousarray(R), np.ascontiguousarray(np.triu(Rinv))
        if what == "ritz":
            T = np.asarray(args[0], dtype=np.float64)
            B = args[1]
            T = np.triu(T) + np.triu(T, 1).T
            theta, S = np.linalg.eigh(T)
            order = np.argsort(-np.abs(theta), kind="stable")
            theta, S = theta[order], np.ascontiguousarray(S[:, order])
            if B is None:
                est = np.zeros(len(theta))
            else:
                b = B.shape[0]
                est = np.sqrt(((B @ S[-b:, :]) ** 2).sum(axis=0)) / np.abs(theta)
            return theta, S, est
    raise ValueError("_eig_dense: " + repr(what))


class _EigSpace(object):
    """the device blocks of one eigsh() call, allocated once: the bases Q and P (one vector of `blocks` n x b blocks each and a
    view of every block; P is Q itself without a mass matrix), the work vector of the csx_bgs_* / csx_gs_* calls, and six working
    blocks of n x wide doubles with an n x b and n x k view of each"""

    def __init__(self, n, b, blocks, wide, mass):
        count = n * b
        nwork = max(_csx.bgs_work_len(n, b, wide, blocks), _csx.bgs_work_len(n, wide, wide, 1), _csx.gs_work_len(n, wide, 1))
        self.nbytes = 8 * (count * blocks * (2 if mass else 1) + 6 * n * wide + nwork)
        self.n, self.b = n, b
        try:
            self.Q, self.Qj = self._basis(n, b, blocks)
            self.P, self.Pj = self._basis(n, b, blocks) if mass else (self.Q, self.Qj)
            self.work = dvec(nwork)
            self._flat = [dvec(n * wide) for _ in range(6)]
        except _csx.CsxError as e:
            raise MemoryError("eigsh: cannot allocate the bases of %d blocks and the working blocks, %d bytes (%s)"
                              % (blocks, self.nbytes, e))
        self._views = {}
        self._flat[5].fill(0.0)

    @staticmethod
    def _view(base, n, k):
        h = _csx.new_handle()
        _csx.check(_csx.lib().csx_vec_wrap(base, n * k, h), "csx_vec_wrap")
        return dvec(n, k, _handle=h)

    def _basis(self, n, b, blocks):
        V = dvec(n * b * blocks)
        base = V.device_ptr() or 0
        return V, [self._view(base + 8 * n * b * j, n, b) for j in range(blocks)]

    def blocks(self, k):
        """the six working blocks as n x k: W, S (the first pass's block; X at a verification), N (a product, negated), B, R and
        the zero right-hand side"""
        if k not in self._views:
            self._views[k] = [self._view(f.device_ptr() or 0, self.n, k) for f in self._flat]
        return self._views[k]


class _SymRefinable(_Refinable):
    """backward_error / refine / condest / operator_info of the solvers of a SYMMETRIC matrix held in the upper triangle
    (cholsol_factor, ldlsol_factor), measured with csx_residual_sym_block against the factored matrix, the
    last refactor's values, or A=.  The solver sets, beside _refine_init(A, n): _dev (the factor's _DevMatrix: its version moves
    when the values change in place), _A2 (the matrix the factor stands for), _stands (the version at which it does) and
    _source (None), and gives solve(list)."""

    _residual_into = staticmethod(_residual_sym_into)

    def _operator_for(self, A_given):
        """the context manager of the operator's handle: A_given's, or the factored / refactored matrix's"""
        if A_given is not None:
            if not CS_CSC(A_given) or A_given.m != self._rn or A_given.n != self._rn:
                raise ValueError("A= must be a square CSC matrix of order %d" % self._rn)
            if not _meta(A_given)[1]:
                raise TypeError("A= is a pattern-only matrix")
            self._source = "given"
            return _resident_handle(A_given)
        if self._stands != self._dev.version:
            raise RuntimeError("the factor was changed in place (update / downdate / cs_updown) and no longer stands for "
                               "the factored matrix: pass the matrix it stands for now as A=, or refactor()")
        self._source = "factored" if self._A2 is self._rA else "refactored"
        return self._operator()

    def backward_error(self, x, b, A=None):
        """omega of x as a solution of S x = b per column (a float for one host vector), S the symmetric matrix in the
        upper triangle of the operator: the factored matrix, or the values of the last successful refactor(), in A's own
        numbering whatever the order; or A=, a square CSC matrix of order n with values (ValueError for another shape,
        TypeError for a pattern-only one) -- pin it (cs_pin) to keep its row gather between calls.  RuntimeError for
        A=None after update / downdate / cs_updown changed the factor: it stands for another matrix then, until the
        next successful refactor()."""
        return self._backward_error(x, b, False, self._operator_for(A))

    def refine(self, b, maxit=5, A=None):
        """solve, then at most maxit steps of iterative refinement against the operator (see backward_error) on the
        columns whose backward error is above 2^-52; b is overwritten with x.  With A= a nearby matrix this is the
        stale-factor iteration: the factor preconditions, A is solved.  _Refinable.refine's loop and result."""
        return self._refine(b, maxit, False, self._operator_for(A))

    def gmres(self, b, restart=16, maxit=64, inner_tol=2.0 ** -26, A=None):
        """solve, then restarted GMRES against the operator (see backward_error) with this factor as the preconditioner;
        b is overwritten with x.  With A= a nearby matrix the stale factor preconditions and A is solved: a matrix that differs
        from the factored one in r rows ends in r + 1 inner steps, however far apart the two are.  _Refinable.gmres's loop,
        arguments and result."""
        return self._gmres(b, restart, maxit, inner_tol, False, lambda: self._operator_for(A))

    def solve_grad(self, x, gx, refine=0, A=None):
        """(gb, gA) as _Refinable.solve_grad for S x = b, S the symmetric matrix in the upper triangle of the operator (see
        backward_error): gb = S^-1 gx by this factor's solve (refine > 0: refine(maxit=refine, A=A)), gA on the pattern of the
        factored matrix -- or of A=, of which only the pattern is read unless refine > 0 -- in sym mode: an entry above the
        diagonal stands at two places of S and takes -sum_c (gb[i, c] x[j, c] + gb[j, c] x[i, c]), a diagonal entry
        -sum_c gb[i, c] x[i, c], an entry below the diagonal +0.0.  RuntimeError for A=None after update / downdate /
        cs_updown changed the factor, as backward_error."""
        if A is not None:
            if not CS_CSC(A) or A.m != self._rn or A.n != self._rn:
                raise ValueError("A= must be a square CSC matrix of order %d" % self._rn)
        elif self._stands != self._dev.version:
            self._operator_for(None)        # raises the RuntimeError of backward_error
        return self._solve_grad(x, gx, False, refine, A if A is not None else self._rA, lambda: self._operator_for(A), True)

    def eigsh(self, nev, M=None, sigma=0.0, block=None, maxblocks=32, tol=2.0 ** -30, seed=0, v0=None, A=None):
        """The nev eigenpairs of K x = lambda M x nearest sigma, by unrestarted shift-invert block Lanczos with full
        reorthogonalisation on this factor.  The factor stands for A = K - sigma M: every step is one block
        solve with it; the operator (see backward_error; A=) is what the residuals are measured against.  M: an SPD matrix in
        the upper triangle of a square CSC `cs`, or None for the identity.  sigma is only added back into the values.
        block: columns of a basis block, 1 .. BGS_MAXW (default min(BGS_MAXW, max(nev, 8)) rounded up to even); capped by n.
        maxblocks: a memory cap -- two bases of maxblocks blocks (one without M) and six working blocks, all allocated before
        the loop; MemoryError with the byte count when they cannot be had.  Running out of blocks returns what there is with
        converged False.  tol: a pair has converged when |M x / theta - A x|_2 <= tol |M x / theta|_2, theta = 1 / (lambda -
        sigma).  v0: an n x block starting block (default numpy.random.default_rng(seed).random((n, block)) - 0.5).
        A dict: values (sigma + mu by ascending |mu|), vectors (a dvec n x nev, M-orthonormal to rounding), resid, omega,
        estimate, converged (one entry per pair), blocks (basis blocks of the Ritz space), solves, products, breakdown (the
        space became invariant to working precision: the pairs are final; fewer than nev are returned if it held fewer), and on
        ldlsol_factor below: the negative pivots of inertia(), the number of eigenvalues under sigma (None when a pivot was
        perturbed).  ValueError for nev < 1, nev > (maxblocks - 1) block, block outside 1 .. BGS_MAXW, tol outside (0, 1), an M or
        v0 of another shape, or a v0 with dependent columns; TypeError for a pattern-only M."""
        n, maxw = self._rn, _csx.bgs_limits()["BGS_MAXW"]
        nev, nb, tol, sigma = int(nev), int(maxblocks), float(tol), float(sigma)
        if nev < 1:
            raise ValueError("eigsh: nev must be at least 1")
        if block is None:
            b = min(maxw, max(nev, 8))
            b = min(maxw, b + (b & 1))
        else:
            b = int(block)
            if b < 1 or b > maxw:
                raise ValueError("eigsh: block must lie in 1 .. %d (BGS_MAXW)" % maxw)
        b = min(b, n)
        nb = min(nb, max(2, n // max(b, 1)))           # a basis holds n vectors at the most
        if not 0.0 < tol < 1.0:
            raise ValueError("eigsh: tol must lie in (0, 1)")
        if b < 1 or nev > (nb - 1) * b or nb > 0x7FFFFFFE:
            raise ValueError("eigsh: nev must be at most (maxblocks - 1) * block = %d" % (max(nb - 1, 0) * max(b, 0)))
        mass = M is not None
        if mass:
            if not CS_CSC(M) or M.m != n or M.n != n:
                raise ValueError("eigsh: M must be a square CSC matrix of order %d" % n)
            if not _meta(M)[1]:
                raise TypeError("eigsh: M is a pattern-only matrix")
        if v0 is None:
            start = np.random.default_rng(seed).random((n, b)) - 0.5
        else:
            start = np.ascontiguousarray(v0, dtype=np.float64)
            if start.shape != (n, b):
                raise ValueError("eigsh: v0 must be an n x block array, %d x %d" % (n, b))
        operator = self._operator_for(A)
        lib = _csx.lib()
        wide = max(b, min(nev, maxw))
        chunks = [(c0, min(c0 + maxw, nev)) for c0 in range(0, nev, maxw)]
        sgn = -1.0 if mass else 1.0                    # W holds sgn times the vector: the products come out negated (below)
        count = {"solves": 0, "products": 0}

        def gram(V, nv, Y, q, negate):
            out = np.empty((nv * b, q))
            _csx.check(lib.csx_bgs_gram(V.handle, nv, b, Y.handle, q, space.work.handle, n, negate, _csx.pd(out)), "csx_bgs_gram")
            return out

        def update(V, nv, X, H):
            _csx.check(lib.csx_bgs_update(V.handle, nv, b, X.handle, b, space.work.handle, n, _csx.pd(_csx.f64(H))),
                       "csx_bgs_update")

        def combine(V, nv, U, q, S):
            _csx.check(lib.csx_bgs_combine(V.handle, nv, b, U.handle, q, space.work.handle, n, _csx.pd(_csx.f64(S))),
                       "csx_bgs_combine")

        def product(X, out, k):
            """out = 0 - M X: exactly -(M X); every reader takes the sign up"""
            self._residual_into(hM, X, space.blocks(k)[5], out, k, False)
            count["products"] += 1

        def orthonormalise(src, s, dst):
            """dst = the block src (held as s times itself) made M-orthonormal by two Cholesky-QR passes -> R2 R1, or None"""
            R = []
            for first, blk, sign, to in ((True, src, s, S1), (False, S1, 1.0, dst)):
                if mass:
                    product(blk, N, b)
                    G = gram(blk, 1, N, b, 1)
                else:
                    G = gram(blk, 1, blk, b, 0)
                r = _eig_dense("cholqr", G, first)
                if r is None:
                    return None
                R.append(r[0])
                combine(blk, 1, to, b, sign * r[1])
            return R[1] @ R[0]

        with operator as hA, (_resident_handle(M) if mass else contextlib.nullcontext(0)) as hM, np.errstate(all="ignore"):
            space = _EigSpace(n, b, nb, wide, mass)
            Q, Qj, P, Pj = space.Q, space.Qj, space.P, space.Pj
            W, S1, N, _, _, _ = space.blocks(b)
            for c0, c1 in chunks:
                space.blocks(c1 - c0)
            ones = _csx.i32(np.ones(maxw))
            T = np.zeros((nb * b, nb * b))
            W.assign(start)
            if orthonormalise(W, 1.0, Qj[0]) is None:
                raise ValueError("eigsh: the columns of the starting block are dependent")
            if mass:
                product(Qj[0], Pj[0], b)
            breakdown, done, j = False, False, 0
            while not done:
                nv = j + 1
                _csx.check(lib.csx_vec_copy(Pj[j].handle, W.handle), "csx_vec_copy")
                self._solve_block(W, False, False)
                count["solves"] += 1
                H1 = gram(P, nv, W, b, 0)
                update(Q, nv, W, sgn * H1)
                H2 = gram(P, nv, W, b, 0)
                update(Q, nv, W, sgn * H2)
                T[:nv * b, j * b:nv * b] = H1 + H2
                Bsub = orthonormalise(W, sgn, Qj[j + 1])
                if Bsub is None:
                    breakdown = True
                elif mass:
                    product(Qj[j + 1], Pj[j + 1], b)
                m = nv * b
                theta, S, est = _eig_dense("ritz", T[:m, :m], Bsub)
                last = breakdown or j + 2 >= nb
                kk = min(nev, m)
                if last or (kk == nev and (est[:nev] <= tol).all()):
                    resid, omega, host = np.empty(kk), np.empty(kk), []
                    for c0, c1 in chunks:
                        c1 = min(c1, kk)
                        if c1 <= c0:
                            break
                        q = c1 - c0
                        Wq, X, Nq, Bq, Rq, _ = space.blocks(q)
                        th, mk = _csx.f64(theta[c0:c1]), _csx.pi(ones)
                        combine(Q, nv, X, q, S[:, c0:c1])
                        if mass:
                            product(X, Nq, q)
                            _csx.check(lib.csx_gs_scale(Nq.handle, Bq.handle, 0, space.work.handle, n, q, mk, _csx.pd(-th)),
                                       "csx_gs_scale")
                        else:
                            _csx.check(lib.csx_gs_scale(X.handle, Bq.handle, 0, space.work.handle, n, q, mk, _csx.pd(th)),
                                       "csx_gs_scale")
                        omega[c0:c1], _ = self._residual_into(hA, X, Bq, Rq, q, False)
                        norms = []
                        for blk in (Rq, Bq):
                            s2 = np.empty(q)
                            _csx.check(lib.csx_vec_copy(blk.handle, Wq.handle), "csx_vec_copy")
                            _csx.check(lib.csx_gs_project(Wq.handle, 1, blk.handle, space.work.handle, n, q, mk, 0, _csx.pd(s2)),
                                       "csx_gs_project")
                            norms.append(np.sqrt(s2))
                        resid[c0:c1] = norms[0] / norms[1]
                        if len(chunks) > 1:
                            host.append(X.numpy().reshape(n, q))
                    done = last or bool((resid <= tol).all())
                j += 1
            vectors = dvec(np.hstack(host)) if len(chunks) > 1 else space.blocks(kk)[1].copy()
        out = {"values": sigma + 1.0 / theta[:kk], "vectors": vectors, "resid": resid, "omega": omega, "estimate": est[:kk].copy(),
               "converged": resid <= tol, "blocks": j, "solves": count["solves"], "products": count["products"],
               "breakdown": breakdown}
        if isinstance(self, _LdlSolver):
            info = self.info()
            out["below"] = None if info["perturbed"] else int(info["neg"])
        return out

    def condest(self, A=None):
        """an estimate of cond_1(S) = |S|_1 |S^-1|_1 of the operator (see backward_error): csx_norm1_sym times
        Hager-Higham's estimate of the inverse's norm from single right-hand-side solves on this factor.  The estimate
        is a lower bound, and no condition number is below 1: the result is never below 1.0 (0.0 for n = 0) -- a solve
        divides by every pivot twice, so for a well-conditioned matrix the product can round to just under 1"""
        with self._operator_for(A) as hA:
            out = _csx.C.c_double(0.0)
            _csx.check(_csx.lib().csx_norm1_sym(hA, out), "csx_norm1_sym")

        def one(v, t):
            x = v.tolist()
            self.solve(x)
            return np.asarray(x, dtype=np.float64)

        n = self._rn
        est = _condest(out.value, one, n)
        return est if n == 0 else max(est, 1.0)     # (a NaN stays a NaN)

    def operator_info(self):
        """source: what the last backward_error / refine / condest measured against ("factored", "refactored" or "given";
        before the first, what A=None would take); builds: how often the refactor's values were wrapped over A's pattern
        (once per set of values given as values rather than as a matrix)"""
        src = self._source or ("factored" if self._A2 is self._rA else "refactored")
        return {"source": src, "builds": self._operator_builds}


def lusol_factor(A, order=0, tol=1.0, exact=None):
    """Factor once for many solves -- the batched form of cs_lusol (csparse.py:1456-1478): cs_sqr + cs_lu once, then
    solve(b) runs the reference's sequence x = b(p); L \\ x; U \\ x; b(q) = x (:1474-1477) on the device for a list (one
    system) or a dvec n-by-k block (k systems, overwritten): csx_permute_vec, csx_tri_solve on L and on U,
    csx_permute_vec.  The order of a solve's operations follows cholsol_factor's rule: exact=None (default): a LIST is
    solved in the reference's order, bit-identical to cs_lusol; a dvec BLOCK in the rounding-equal order (x[] within the
    1e-10 of BASELINE.json's north_star) -- which differs from the exact one only where the factors fall into many small
    independent components of at most 80 rows (config 3's W: 1 493 of 67), solved densely on the matrix cores then
    (csx_tri_set_order; refused when an inverse of a diagonal tile is large); exact=True: every solve bit-identical to
    cs_lusol on that column; exact=False: every solve rounding-equal.  cs_lusol, the reference's driver, is always exact.
    solve(b, comm=..., nrhs=K) shards the block by right-hand-side block over the ranks of a shard.Comm, every rank
    holding this factor; see cholsol_factor.
    solve(b, trans=True) solves A' x = b on the same factors (L U = A(p, q)): y = b(q) (cs_pvec), U' y = y
    (cs_utsolve), L' y = y (cs_ltsolve), x = y(pinv) (cs_pvec) -- the exact order is that sequence operation for operation,
    under the same rule for lists, blocks and `exact`; through comm= as well.
    condest(): an estimate of cond_1(A) = |A|_1 |A^-1|_1: cs_norm(A) (cached) times Hager-Higham's estimate of |A^-1|_1
    (LAPACK dlacn2's iteration) from exact-order single right-hand-side solves, forward and transposed.
    refactor(A2): new values, the same pivots: A2 a CSC `cs` with A's exact pattern, or nnz(A) values in A's
    storage order (numpy, list or dvec); ValueError for another pattern or length.  L and U get the values cs_lu's own loop
    gives with this pinv (byte-equal to cs_lu(A2) whenever it would pivot the same), on the device for connected components
    of at most 96 rows, on the host for the rest.  True on success; False when a kept pivot is 0 or not finite, and then
    nothing changes.  The triangular-solve plans hold copies of the values: they are rebuilt by the next solve.
    refactor_info(): the last refactor's pivot_ratio (min over the columns of |u_kk| / the largest candidate of its column),
    device_columns, host_columns and ms.
    backward_error(x, b, trans=False): the componentwise backward error of x per column, against A or the last refactor's values;
    refine(b, maxit=5, trans=False): solve, then iterative refinement while it lowers that error; b is overwritten with x
    (_Refinable).
    None when A is not square CSC or singular."""
    if not CS_CSC(A) or A.m != A.n:
        return None
    S = cs_sqr(order, A, False)
    N = cs_lu(A, S, tol) if S is not None else None
    if N is None:
        return None
    n = A.n
    L, U = cs_pin(N.L), cs_pin(N.U)
    hp, keep_p = _perm_handle(N.pinv, n)
    hq, keep_q = _perm_handle(S.q, n)

    class _Solver(_Refinable):
        factors, symbolic = N, S

        def __init__(self):
            self._fin = weakref.finalize(self, lambda hs: [_csx.free(h) for h in hs if h is not None], [keep_p, keep_q])
            self._A2, self._norm = A, None         # the matrix condest() is about: A, or the last refactor's A2
            self._rplan, self._rinfo = None, None
            self._refine_init(A, n)

        def _solve_block(self, blk, trans, from_list):
            return self._block(blk, exact if exact is not None else from_list, trans)

        def _block(self, blk, in_exact_order=True, trans=False):
            # x(pinv) = b, L x = x, U x = x, b(q) = x (csparse.py:1470-1473) as ONE library call: in the rounding-equal order on
            # forests of small components the two permutations ride on the two sweeps (csx_lusol_solve); trans: y = b(q),
            # U' y = y, L' y = y, x = y(pinv) (csx_lusol_solve_trans)
            lib = _csx.lib()
            x = dvec(n, blk.k)
            with _Resident(L) as dL, _Resident(U) as dU:
                # (shared with the list-level cs_lsolve / cs_usolve / cs_ltsolve / cs_utsolve on this factor: the order is set per solve)
                if trans:
                    p1, p2, fn, name = _plan(dU, TRI_UT), _plan(dL, TRI_LT), lib.csx_lusol_solve_trans, "csx_lusol_solve_trans"
                else:
                    p1, p2, fn, name = _plan(dL, TRI_L), _plan(dU, TRI_U), lib.csx_lusol_solve, "csx_lusol_solve"
                fused = _csx.C.c_int(0)
                _in_order((p1, p2), in_exact_order,
                          lambda: _csx.check(fn(p1, p2, hp, hq, blk.handle, x.handle, blk.k, _csx.C.byref(fused)), name))
            self.last_fused = bool(fused.value)
            return blk

        def info(self):
            """which of the two triangular solves run on the matrix cores in the rounding-equal order, and the guard's measure"""
            out = {}
            for name, M, kind in (("L", L, TRI_L), ("U", U, TRI_U)):
                with _Resident(M) as dM:
                    mc, g = _csx.C.c_int32(0), _csx.C.c_double(0.0)
                    plan = _plan(dM, kind)
                    _csx.check(_csx.lib().csx_tri_set_order(plan, 0), "csx_tri_set_order")
                    _csx.check(_csx.lib().csx_tri_order_info(plan, mc, g), "csx_tri_order_info")
                    _csx.lib().csx_tri_set_order(plan, 1)
                    out[name] = {"matrix_cores": bool(mc.value), "growth": g.value}
            return out

        def solve(self, b, comm=None, nrhs=None, trans=False):
            trans = bool(trans)
            if comm is not None and comm.world > 1:
                # every rank solves in the order the ROOT's right-hand side asks for
                ex = comm.broadcast_object((exact if exact is not None else not isinstance(b, dvec)) if comm.rank == 0 else None, 0)
                out, bhost = _solve_blocks_sharded(comm, b, nrhs, n, n, lambda blk: self._block(blk, ex, trans))
                if out is not None:
                    _write_back(bhost, out, n * out.k)
                return True
            db, bhost = _vec_in(b, n, "b")
            self._block(db, exact if exact is not None else not isinstance(b, dvec), trans)
            _write_back(bhost, db, n * db.k)
            return True

        def condest(self):
            if self._norm is None:
                self._norm = _refactor_norm(A, self._A2)
            return _condest(self._norm, lambda v, t: self._block(dvec(v), True, t).numpy(), n)

        def refactor(self, A2):
            t0 = time.perf_counter()
            A2 = _refactor_input(A, A2)
            if self._rplan is None:
                # the refactor's schedule and maps, on the first call only: nothing of it exists for a solver never refactored
                h = _csx.new_handle()
                q = None if S.q is None else _csx.i32(S.q)
                with _Resident(L) as dL, _Resident(U) as dU, _Resident(A) as dA:
                    _csx.check(_csx.lib().csx_lu_refactor_plan(dL.handle, dU.handle, dA.handle,
                                                               None if q is None else _csx.pi(q), _csx.pi(_csx.i32(N.pinv)), h),
                               "csx_lu_refactor_plan")
                self._rplan = h
                weakref.finalize(self, _csx.free, h)
            ok, ratio, cols = _csx.C.c_int(0), _csx.C.c_double(0.0), (_csx.C.c_int64 * 2)()
            _refactor_call(A2, lambda h: _csx.lib().csx_lu_refactor(self._rplan, h, ok, ratio, cols), ok)
            if ok.value:
                for M in (L, U):
                    _refactored(M, M._dev)
                self._A2, self._norm = A2, None
                self._operator_changed()
            self._rinfo = {"ok": bool(ok.value), "pivot_ratio": ratio.value, "device_columns": int(cols[0]),
                           "host_columns": int(cols[1]), "ms": 1e3 * (time.perf_counter() - t0)}
            return bool(ok.value)

        def refactor_info(self):
            return dict(self._rinfo) if self._rinfo is not None else None

    return _Solver()


# ------------------------------------------------------ LU, static pivots ----

_SLU_INFO = ("n", "lnz", "levels", "launches", "level_launches", "run_launches", "perturbed", "breakdown", "kernel_us",
             "long_columns", "window", "run_levels", "pos", "neg")


_SLU_BATCH_SHARED = ("n", "lnz", "levels", "launches", "level_launches", "run_launches", "kernel_us", "B")
_SLU_BATCH_MEMBER = ("perturbed", "breakdown", "long_columns", "pos", "neg")
_SLU_BATCH_STATS = ("min_abs_d", "max_abs_d", "max_abs_l", "max_abs_u")


class _ValueBatch(object):
    """What _SluBatch, _LdlBatch and _HqrBatch share: the intake of the values, the thresholds, the run, the solve's block and
    info().  A batch class names its texts' prefix (_NAME), the prefix of its library calls (_CALLS), its limits, its statistics
    and the integers of its info() (_SHARED of the whole run, _MEMBER per member)."""

    _NAME, _CALLS, _STATS = "", "", ()
    _SHARED, _MEMBER = _SLU_BATCH_SHARED, _SLU_BATCH_MEMBER
    _limits = staticmethod(lambda: {})

    def __init__(self, solver, hF, nnz, n, perturb, values):
        self._solver, self._hF, self._nnz, self._n, self._perturb = solver, hF, nnz, n, perturb     # (the solver keeps the factor alive)
        V, self.B = self._values(values, None)
        h, ok = _csx.new_handle(), (_csx.C.c_int * self.B)()
        _csx.check(self._call("factor")(hF, V.handle, self.B, *(self._run_args(V) + (h, ok))), self._CALLS + "_factor")
        self._h = h
        self._fin = weakref.finalize(self, _csx.free, h)
        self.ok = np.array(ok[:], dtype=bool)

    def _call(self, name):
        return getattr(_csx.lib(), self._CALLS + "_" + name)

    def _values(self, values, B):
        """(dvec of nnz x B, B) of the caller's values; B: the members it must have, or None"""
        a = None
        if isinstance(values, dvec):
            rows, k = values.n, values.k
        else:
            a = values if isinstance(values, np.ndarray) else np.asarray([np.asarray(v, dtype=np.float64).ravel() for v in values]).T
            a = np.asarray(a, dtype=np.float64)
            if a.ndim != 2 or a.shape[1] < 1:
                raise ValueError("%s: values must be an nnz x B block or a list of B value arrays, B >= 1" % self._NAME)
            rows, k = a.shape
        if rows != self._nnz:
            raise ValueError("%s: %d rows of values given, the factored matrix has %d entries" % (self._NAME, rows, self._nnz))
        if B is not None and k != B:
            raise ValueError("%s: %d members given, the batch has %d" % (self._NAME, k, B))
        most = self._limits()["MAX_MEMBERS"]
        if k > most:
            raise ValueError("%s: %d members, a batch holds at most %d: split the family" % (self._NAME, k, most))
        return (self._device_rows(values, k) if a is None else dvec(self._host_rows(a))), k

    def _host_rows(self, a):
        """the nnz x B numpy block in the storage order of the factored matrix (here: as given)"""
        return a

    def _device_rows(self, V, k):
        return V

    def _run_args(self, V):
        """what a run takes between the values and its results: the members' thresholds (a factorisation without one: nothing)"""
        return (_csx.pd(self._tau(V)),)

    def _tau(self, V):
        if self._perturb == 0.0:
            return None
        out = np.zeros(self.B)
        _csx.check(self._call("norm1")(self._hF, V.handle, self.B, _csx.pd(out)), self._CALLS + "_norm1")
        return self._perturb * out

    def refactor(self, values):
        V, _ = self._values(values, self.B)
        ok = (_csx.C.c_int * self.B)()
        _csx.check(self._call("refactor")(self._h, V.handle, *(self._run_args(V) + (ok,))), self._CALLS + "_refactor")
        self.ok = np.array(ok[:], dtype=bool)
        return self.ok

    def _solve(self, X, *more):
        if isinstance(X, dvec):
            d, host = X, None
        else:
            host = X
            d = dvec(np.asarray(X, dtype=np.float64))
        if d.n != self._n or d.k < self.B or d.k % self.B:
            raise ValueError("%s.solve: X must be n x (B r) = %d x (%d r)" % (self._NAME, self._n, self.B))
        _csx.check(self._call("solve")(self._h, d.handle, d.k // self.B, *more), self._CALLS + "_solve")
        if host is not None:
            if not isinstance(host, np.ndarray):
                raise ValueError("%s.solve: X must be a dvec or a numpy array" % self._NAME)
            host[...] = d.numpy().reshape(host.shape)
        return True

    def _member(self, m, second):
        """(L.x, the member's second array of `second`(info) doubles) of member m"""
        m = int(m)
        if not 0 <= m < self.B:
            raise ValueError("%s.member: member %d of %d" % (self._NAME, m, self.B))
        i = self.info()
        lnz, cnt = i["lnz"], second(i)
        Lx, other = np.empty(max(lnz, 1)), np.empty(max(cnt, 1))
        _csx.check(self._call("member")(self._h, m, _csx.pd(Lx), _csx.pd(other)), self._CALLS + "_member")
        return Lx[:lnz], other[:cnt]

    def info(self):
        C = _csx.C
        shared = (C.c_int64 * len(self._SHARED))()
        per = np.zeros((self.B, len(self._MEMBER)), dtype=np.int64)
        st = np.zeros((self.B, len(self._STATS)))
        _csx.check(self._call("info")(self._h, shared, per.ctypes.data_as(C.POINTER(C.c_int64))), self._CALLS + "_info")
        _csx.check(self._call("stats")(self._h, _csx.pd(st)), self._CALLS + "_stats")
        out = {name: int(v) for name, v in zip(self._SHARED, shared)}
        out.update((name, per[:, k].copy()) for k, name in enumerate(self._MEMBER))
        out.update((name, st[:, k].copy()) for k, name in enumerate(self._STATS))
        return out


class _SluBatch(_ValueBatch):
    """B value sets on the pattern of one slusol_factor, factored together (slusol_factor(...).batch(values)): the
    members share the factor's analysis, matching, order and launch schedule, and go through every launch of it at once.
    Every member's factor is byte-equal to slusol_factor of that member alone under the same matching and order.
    B: the members.  ok: a numpy bool array, False where a member broke down -- there is no commit for a batch, so such a
      member's values mean nothing (until a refactor mends it) and the others are untouched.
    refactor(values): new values for all B members (B is fixed) -> the new ok.
    solve(X, trans=False): X an n x (B r) block (dvec, overwritten; or a 2-D numpy array, overwritten), columns m r .. m r + r - 1
      belong to member m; always in the exact order: every column has the bytes of
      slusol_factor(A_m, exact=True).solve(...).  The columns of a failed member come back NaN.
    member(m) -> (Lx, Utx) as numpy arrays; info(): n, lnz, levels, launches, level_launches, run_launches, kernel_us and B of the
      whole run, and numpy arrays per member: perturbed, breakdown, long_columns, pos, neg, min_abs_d, max_abs_d, max_abs_l,
      max_abs_u.
    Deliberately NOT here: refine, gmres, condest, inverse, solve_grad.  The route to them is the single factor:
    F.refactor(values[:, m])."""

    _NAME, _CALLS, _STATS = "slusol_factor.batch", "csx_slu_batch", _SLU_BATCH_STATS
    _limits = staticmethod(_csx.slu_batch_limits)

    def solve(self, X, trans=False):
        return self._solve(X, 1 if trans else 0)

    def member(self, m):
        return self._member(m, lambda i: i["lnz"])


class _LdlBatch(_ValueBatch):
    """B symmetric value sets on the pattern of one ldlsol_factor, factored together (ldlsol_factor(...).batch(values); DESIGN.md
    §36): K - sigma_j M over shifts, quasi-definite KKT systems over scenarios.  The members share the factor's analysis, order
    and launch schedule and go through every launch of it at once; every member's L.x and d are byte-equal to ldlsol_factor of
    that member alone under the same order.  Half the factor storage of the route through slusol_factor(...).batch, and the
    inertia of every member.
    B: the members.  ok: a numpy bool array, False where a member broke down -- there is no commit for a batch, so such a
      member's values mean nothing (until a refactor mends it) and the others are untouched.
    refactor(values): new values for all B members (B is fixed) -> the new ok.
    solve(X): X an n x (B r) block (dvec, overwritten; or a 2-D numpy array, overwritten), columns m r .. m r + r - 1 belong to
      member m; always in the exact order, the division by D fused into the backward sweep: every column has the bytes of
      ldlsol_factor(A_m, exact=True).solve(...).  The columns of a failed member come back NaN.
    member(m) -> (Lx, d) as numpy arrays.  inertia() -> (pos, neg), numpy arrays per member: neg[m] of K - sigma_m M counts the
      eigenvalues below sigma_m (exact arithmetic; perturbed pivots keep their sign).  logdet() -> (signs, logs) per member, the
      sum of log |d| correctly rounded (math.fsum) as the single solver's; NaN for a failed member.
    info(): n, lnz, levels, launches, level_launches, run_launches, kernel_us and B of the whole run, and numpy arrays per
      member: perturbed, breakdown, long_columns, pos, neg, min_abs_d, max_abs_d, max_abs_l.
    Deliberately NOT here: refine, gmres, condest, inverse, solve_grad, eigsh.  The route to them is the single factor:
    F.refactor(values[:, m])."""

    _NAME, _CALLS, _STATS = "ldlsol_factor.batch", "csx_ldl_batch", ("min_abs_d", "max_abs_d", "max_abs_l")
    _limits = staticmethod(_csx.ldl_batch_limits)

    def solve(self, X):
        return self._solve(X)

    def member(self, m):
        return self._member(m, lambda i: i["n"])

    def inertia(self):
        i = self.info()
        return i["pos"], i["neg"]

    def logdet(self):
        d = np.empty(max(self.B * self._n, 1))
        _csx.check(self._call("d")(self._h, _csx.pd(d)), "csx_ldl_batch_d")
        d = d[:self.B * self._n].reshape(self.B, self._n)
        signs, logs = np.full(self.B, np.nan), np.full(self.B, np.nan)
        for m in np.flatnonzero(self.ok):
            signs[m] = -1.0 if int(np.sum(d[m] < 0.0)) % 2 else 1.0
            logs[m] = math.fsum(np.log(np.abs(d[m])).tolist())
        return signs, logs


_HQR_BATCH_SHARED = ("m", "n", "m2", "vnz", "rnz", "levels", "launches", "level_launches", "run_launches", "kernel_us", "B",
                     "solve_launches")
_HQR_BATCH_MEMBER = ("breakdown", "long_columns", "zero_diagonals")


class _HqrBatch(_ValueBatch):
    """B value sets on the pattern of one hqrsol_factor, factored together (hqrsol_factor(...).batch(values)):
    reweighted least squares W_j A, Gauss-Newton Jacobians over scenarios, regularisation sweeps on a stacked [A; lambda_j I].
    The members share the factor's analysis, column order and launch schedule and go through every launch of it at once; every
    member's V.x, R.x and beta are byte-equal to csx_hqr_host, that is to hqrsol_factor of that member alone.
    B: the members.  ok: a numpy bool array, False where a diagonal of a member's R came out non-finite -- there is no commit
      for a batch, so such a member's values mean nothing (until a refactor mends it) and the others are untouched.
    refactor(values): new values for all B members (B is fixed) -> the new ok.
    solve(X, trans=False): X a dvec or a 2-D numpy array of rows_in x (B r), columns m r .. m r + r - 1 belonging to member m ->
      a NEW dvec / array of rows_out x (B r), X left as it was; the single solver's sequences (first: m >= n, rows m -> n;
      second: m < n, or trans=True on a square A, rows n -> m of the factored matrix) in the reference's operation order: every
      column has the bytes of hqrsol_factor(A_m).solve(...) on a list.  The columns of a failed member come back NaN; an exact
      zero on R's diagonal is no breakdown (ok stays True, info()["zero_diagonals"] counts it) and gives what the single solver
      gives: ZeroDivisionError, as the reference's division does.  trans=True on a rectangular A: ValueError.
    member(m) -> (Vx, Rx, beta) as numpy arrays.  logabsdet() -> a numpy array per member, the sum of log |r_kk| correctly
      rounded (math.fsum) as the single solver's, NaN for a failed member; ValueError for a rectangular A.
    info(): m, n, m2, vnz, rnz, levels, launches, level_launches, run_launches, kernel_us, B of the whole run and solve_launches of
      the last solve, and numpy arrays per member: breakdown, long_columns, zero_diagonals, min_abs_r, max_abs_r.
    Deliberately NOT here: refine, gmres, condest, solve_grad.  The route to them is the single factor:
    F.refactor(values[:, m])."""

    _NAME, _CALLS, _STATS = "hqrsol_factor.batch", "csx_hqr_batch", ("min_abs_r", "max_abs_r")
    _SHARED, _MEMBER = _HQR_BATCH_SHARED, _HQR_BATCH_MEMBER
    _limits = staticmethod(_csx.hqr_batch_limits)

    def __init__(self, solver, hF, nnz, shape, storage_map, values):
        self._shape, self._storage_map = shape, storage_map      # (A's m and n; None, or the maker of A's order -> A''s)
        _ValueBatch.__init__(self, solver, hF, nnz, None, 0.0, values)

    def _run_args(self, V):
        return ()

    # a wide A: the factored matrix is A', and the rows of the value block go into ITS storage order

    def _host_rows(self, a):
        return a if self._storage_map is None else np.ascontiguousarray(a[self._storage_map()])

    def _device_rows(self, V, k):
        if self._storage_map is None:
            return V
        out = dvec(self._nnz, k)
        h, keep = _perm_handle(self._storage_map(), self._nnz)
        try:
            _csx.check(_csx.lib().csx_permute_vec(h, V.handle, out.handle, self._nnz, k, 0), "csx_permute_vec")
        finally:
            _csx.free(keep)
        return out

    def solve(self, X, trans=False):
        am, an = self._shape
        if trans and am != an:
            raise ValueError("hqrsol_factor: trans=True needs a square matrix")
        second = bool(trans) or am < an
        fm, fn = max(am, an), min(am, an)            # the factored matrix: A, or A' for a wide A
        rows_in, rows_out = (fn, fm) if second else (fm, fn)
        host = not isinstance(X, dvec)
        if host and not (isinstance(X, np.ndarray) and X.ndim == 2):
            raise ValueError("%s.solve: X must be a dvec or a 2-D numpy array" % self._NAME)
        d = dvec(np.asarray(X, dtype=np.float64)) if host else X
        if d.n != rows_in or d.k < self.B or d.k % self.B:
            raise ValueError("%s.solve: X must be %d x (B r) = %d x (%d r)" % (self._NAME, rows_in, rows_in, self.B))
        out = dvec(rows_out, d.k)
        _csx.check(self._call("solve")(self._h, d.handle, out.handle, d.k // self.B, 1 if second else 0), self._CALLS + "_solve")
        return out.numpy().reshape(rows_out, d.k) if host else out

    def member(self, m):
        m = int(m)
        if not 0 <= m < self.B:
            raise ValueError("%s.member: member %d of %d" % (self._NAME, m, self.B))
        i = self.info()
        Vx, Rx, beta = np.empty(max(i["vnz"], 1)), np.empty(max(i["rnz"], 1)), np.empty(max(i["n"], 1))
        _csx.check(self._call("member")(self._h, m, _csx.pd(Vx), _csx.pd(Rx), _csx.pd(beta)), self._CALLS + "_member")
        return Vx[:i["vnz"]], Rx[:i["rnz"]], beta[:i["n"]]

    def logabsdet(self):
        am, an = self._shape
        if am != an:
            raise ValueError("hqrsol_factor: logabsdet needs a square matrix (least-squares refinement is not offered)")
        d = np.empty(max(self.B * an, 1))
        _csx.check(self._call("r_diag")(self._h, _csx.pd(d)), self._CALLS + "_r_diag")
        d = d[:self.B * an].reshape(self.B, an)
        logs = np.full(self.B, np.nan)
        with np.errstate(divide="ignore"):
            for m in np.flatnonzero(self.ok):
                logs[m] = math.fsum(np.log(np.abs(d[m])).tolist())
        return logs


def _perm_parity(p):
    """+1.0 / -1.0: the sign of the permutation p (a sequence of 0..n-1), from its cycles"""
    p = np.asarray(p, dtype=np.int64)
    seen = np.zeros(len(p), dtype=bool)
    even = True
    for s in range(len(p)):
        k, length = s, 0
        while not seen[k]:
            seen[k] = True
            k = int(p[k])
            length += 1
        if length and length % 2 == 0:
            even = not even
    return 1.0 if even else -1.0


def slusol_factor(A, order=0, perturb=0.0, match=None, seed=0, exact=None):
    """Factor a general UNSYMMETRIC matrix in one connected piece once for many solves, on the device, without a pivot search
    (DESIGN.md §23): L U = P A(prow, :) P' with L unit lower triangular and U = Ut' upper triangular, both on the Cholesky pattern
    of the pattern of A1 + A1', A1 = A(prow, :).
    match: a maximum matching (maxtrans_array(A, seed): the row matched to column j becomes row j) puts a zero-free diagonal in
      place: None (default) matches only when some diagonal entry of A is not stored, True always, False never.  None is
      returned for a structurally singular A.  The matching is unweighted: it knows nothing of the values.
    order: 0 natural, 1 nested dissection of A1 + A1' (cs_schol's), applied symmetrically.
    perturb: a pivot with |d| < tau = perturb |A|_1 is replaced by copysign(tau, d) and counted (info()["perturbed"]).  It is
      RELATIVE TO |A|_1 AND NOT A DEFAULT: 0.0 (default) perturbs nothing, and a zero or non-finite pivot is a breakdown.  On a
      badly scaled matrix (fs_183_1: |A|_1 = 8e8) 1e-10 perturbs half the pivots and refinement does not recover.
    Static pivoting is not backward stable by itself: follow solve() with refine() and read backward_error().  Of duplicate
    entries the factorisation takes the last (as cs_lu does) while a residual sums them: sum them first (cs_dupl).
    None for a non-CSC or non-square A, and None on breakdown.  Otherwise a solver:
    solve(b, trans=False): b a list (one system) or a dvec n-by-k block, overwritten: x(pinv o prow^-1) = b, cs_lsolve(L),
      cs_ltsolve(Ut), x = x(pinv); trans=True (A' x = b): x(pinv) = b, cs_lsolve(Ut), cs_ltsolve(L), x = x(pinv o prow^-1).  The
      sweeps follow lusol_factor's rule for `exact`.
    refactor(A2): new values on the kept analysis (and the kept matching), A2 as for lusol_factor's refactor: True; False with
      L, Ut and the solves exactly as before on breakdown; ValueError for another pattern or length.  L.x and Ut.x are byte-equal
      to a fresh factor's under the same prow and order.
    batch(values, perturb=None): B value sets on A's pattern factored together in one walk of the levels (_SluBatch, DESIGN.md
      §32): a parameter sweep on one pattern; this factor is left as it is.
    backward_error(x, b, trans=False), refine(b, maxit=5, trans=False): _Refinable's; condest(): cond_1(A) estimated from
      exact-order solves; logdet(): (sign, log |det A|), the sign with both permutations' parities; info(): n, lnz, levels,
      launches = level_launches + run_launches of the last run, perturbed, breakdown, kernel_us, long_columns (updated in place:
      longer than the LDS `window`), run_levels (levels per walker launch), pos, neg (pivot signs), min_abs_d, max_abs_d,
      max_abs_l, max_abs_u, matched.  factors: .L, .U (= Ut: column k is row k of U, the pivot first), .prow, .pinv.
    inverse() -> (ZL, ZUt), inverse_at(rows, cols), inverse_entries() (entry (r, c) of A -> inv(A)(c, r), the gradient of
      log|det A|), inverse_diag(): entries of inv(A) on the pattern of the factors (sparseinv_lu), computed from the
      factor as it stands.  A static-pivot factor is not backward stable and the recurrence inherits its growth, as solve()
      without refine() does: info()["max_abs_l"] says when to distrust them."""
    if not CS_CSC(A) or A.m != A.n:
        return None
    perturb = float(perturb)
    if not perturb >= 0.0:
        raise ValueError("slusol_factor: perturb must be >= 0")
    n = A.n
    if not _meta(A)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    if match is None:
        p, i = _pattern_np(A)
        cols = np.repeat(np.arange(n, dtype=np.int32), np.diff(p))
        match = int(np.unique(cols[i[:len(cols)] == cols]).size) < n
    prow = None
    if match:
        prow = maxtrans_array(A, seed)[n:]
        if n and int(prow.min()) < 0:
            return None                              # structurally singular
        prow = np.ascontiguousarray(prow, dtype=np.int32)
    # B: the pattern of A1 + A1' (the values do not matter), for the ordering and the counts
    A1 = A
    if prow is not None:
        prinv = np.empty(n, dtype=np.int32)
        prinv[prow] = np.arange(n, dtype=np.int32)
        A1 = cs_permute(A, prinv, None, False)
    B = cs_add(A1, cs_transpose(A1, False), 1.0, 1.0)
    S = cs_schol(order, B, _arrays=True) if B is not None else None
    if S is None:
        return None
    pinv = None if S.pinv is None else _csx.i32(S.pinv)
    lib = _csx.lib()
    hF, ok = _csx.new_handle(), _csx.C.c_int(0)
    with _Resident(A) as dA:
        _csx.check(lib.csx_slu_factor(dA.handle, _csx.pi(_csx.i32(S.parent)), _csx.pi(_csx.i32(S.cp)), _csx.pi(prow), _csx.pi(pinv),
                                      _perturb_tau(perturb, lib.csx_norm1, dA), hF, ok), "csx_slu_factor")
    if not ok.value:
        return None
    hL, hU = _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_slu_parts(hF, hL, hU), "csx_slu_parts")
    N = csn()
    (N.L, N.U), _ = _adopt_factor(hF, hL, mats=[hU])     # (Ut lives in the factor that L's wrapper frees)
    devL, devU = N.L._dev, N.U._dev
    N.prow = None if prow is None else prow.tolist()
    N.pinv, N.B = None if pinv is None else pinv.tolist(), None
    # the two permutations of a solve: x(comb) = b before the forward sweeps, x = x(pinv) after them (swapped for A')
    comb = pinv
    if prow is not None:
        comb = prinv if pinv is None else pinv[prinv]
    hc, keep_c = _perm_handle(comb, n)
    hp, keep_p = _perm_handle(pinv, n)
    sign_perm = (_perm_parity(prow) if prow is not None else 1.0)    # (P C P' keeps the determinant)
    perturb_of_factor = perturb

    class _Solver(_Refinable):
        factors = N

        symbolic = property(lambda self: _symbolic_lists(S))

        def __init__(self):
            self._devs = (devL, devU)                # keep L, Ut and the factor alive
            self._fin = weakref.finalize(self, lambda hs: [_csx.free(h) for h in hs if h is not None], [keep_c, keep_p])
            self._A2, self._norm = A, None
            self._refine_init(A, n)

        def _solve_block(self, blk, trans, from_list):
            return self._block(blk, exact if exact is not None else from_list, trans)

        def _block(self, blk, in_exact_order=True, trans=False):
            k = blk.k
            (h_in, p_in), (h_out, p_out) = ((hp, pinv), (hc, comb)) if trans else ((hc, comb), (hp, pinv))
            x = blk
            if p_in is not None:
                x = dvec(n, k)
                _csx.check(lib.csx_permute_vec(h_in, blk.handle, x.handle, n, k, 1), "csx_permute_vec")
            p1, p2 = (_plan(devU, TRI_L), _plan(devL, TRI_LT)) if trans else (_plan(devL, TRI_L), _plan(devU, TRI_LT))

            def sweeps():
                _csx.check(lib.csx_tri_solve(p1, x.handle, k), "csx_tri_solve")
                _csx.check(lib.csx_tri_solve(p2, x.handle, k), "csx_tri_solve")

            _in_order((p1, p2), in_exact_order, sweeps)
            if p_out is not None:
                y = blk if x is not blk else dvec(n, k)
                _csx.check(lib.csx_permute_vec(h_out, x.handle, y.handle, n, k, 0), "csx_permute_vec")
                if y is not blk:
                    _csx.check(lib.csx_vec_copy(y.handle, blk.handle), "csx_vec_copy")
            elif x is not blk:
                _csx.check(lib.csx_vec_copy(x.handle, blk.handle), "csx_vec_copy")
            return blk

        def solve(self, b, trans=False):
            db, bhost = _vec_in(b, n, "b")
            self._block(db, exact if exact is not None else not isinstance(b, dvec), bool(trans))
            _write_back(bhost, db, n * db.k)
            return True

        def refactor(self, A2):
            A2 = _refactor_input(A, A2)
            ok = _csx.C.c_int(0)
            tau = _refactor_tau(perturb, lib.csx_norm1, A, A2)
            _refactor_call(A2, lambda h2: lib.csx_slu_refactor(hF, h2, tau, ok), ok)
            if ok.value == 1:
                _refactored(N.L, devL)
                _refactored(N.U, devU)
                self._A2, self._norm = A2, None
                self._operator_changed()
            return ok.value == 1

        def batch(self, values, perturb=None):
            """B value sets on A's pattern factored together on this factor's analysis -> a _SluBatch (its docstring has the
            rest).  values: a dvec of nnz x B (read, not kept), a 2-D numpy array of that shape, or a list of B value arrays
            (copied), each in A's storage order; perturb: defaults to this factor's.  ValueError for another row count or B = 0.
            This factor is not changed and goes on working; it must not be freed before the batch, which holds on to it."""
            pb = perturb_of_factor if perturb is None else float(perturb)
            if not pb >= 0.0:
                raise ValueError("slusol_factor.batch: perturb must be >= 0")
            return _SluBatch(self, hF, _meta(A)[0], n, pb, values)

        def condest(self):
            if self._norm is None:
                self._norm = _refactor_norm(A, self._A2)
            return _condest(self._norm, lambda v, t: self._block(dvec(v), True, t).numpy(), n)

        def info(self):
            return _factor_info(hF, "csx_slu_info", _SLU_INFO, "csx_slu_stats", ("min_abs_d", "max_abs_d", "max_abs_l", "max_abs_u"),
                                matched=prow is not None)

        def logdet(self):
            """(sign, log |det A|): det A = det(prow) * the product of the pivots (the symmetric permutation cancels); the sum
            of log |d_j| correctly rounded (math.fsum)"""
            Lp = np.empty(n + 1, dtype=np.int32)
            x = np.empty(max(devU.info()[2], 1), dtype=np.float64)
            _csx.check(lib.csx_csc_download(devU.handle, _csx.pi(Lp), None, _csx.pd(x)), "csx_csc_download")
            d = x[Lp[:n]]
            sign = sign_perm * (-1.0 if int(np.sum(d < 0.0)) % 2 else 1.0)
            return sign, math.fsum(np.log(np.abs(d)).tolist())

        # Entries of inv(A) on the pattern of L and Ut (sparseinv_lu).  Each call reads the factor as it stands
        # (after refactor: the new values; after a refactor that broke down: the old ones) and keeps nothing.  Static pivoting
        # is not backward stable and the recurrence inherits the factor's growth, as solve() without refine() does:
        # info()["max_abs_l"] says when to distrust the entries.

        def inverse(self):
            """(ZL, ZUt): Z = inv(L U) on the pattern of the factors, in their numbering: ZL(i,j) = Z(i,j), ZUt(i,j) = Z(j,i),
            i >= j; inv(A)(x, y) = Z(pinv[x], pinv[prow^-1[y]])"""
            return sparseinv_lu(N.L, N.U)

        def inverse_at(self, rows, cols):
            """inv(A)(rows[t], cols[t]) in A's numbering as a numpy array; ValueError naming how many pairs are not on the
            pattern of the factors"""
            ZL, ZUt = self.inverse()
            return _inverse_at("slusol_factor.inverse_at", ZL, ZUt, hp, hc, rows, cols)

        def inverse_entries(self):
            """one value per stored entry q of A at (r, c): inv(A)(c, r) = d log|det A| / d A(r,c), the companion of logdet();
            always on the pattern (the slot of that entry of the factors, in the other array); duplicates share a value"""
            r, c = _entries_np(A)
            return self.inverse_at(c, r)

        def inverse_diag(self):
            """diag(inv(A)) in A's numbering as a numpy array.  With a matching in force inv(A)(i,i) is on the pattern only
            where A(i,i) is stored or filled: ValueError, as inverse_at's, when some are not"""
            k = np.arange(n, dtype=np.int32)
            return self.inverse_at(k, k)

    return _Solver()


# -------------------------------------------------------------------- QR ----
# cs_qr: host C++ (csx_qr_host), on the device for batches of small independent blocks (csx_qr_blocks); the Q' x step of
# the solve (cs_happly for every reflection) and the triangular solves on the device.

def cs_etree(A, ata):
    """Elimination tree of A (ata False; upper triangle used) or of A'A (csparse.py:1136-1169)."""
    if not CS_CSC(A):
        return None
    m, n = A.m, A.n
    Ap, Ai = A.p, A.i
    parent = [-1] * n
    anc = [-1] * n
    prev = [-1] * m if ata else None
    for k in range(n):
        for p in range(Ap[k], Ap[k + 1]):
            i = prev[Ai[p]] if ata else Ai[p]
            while i != -1 and i < k:
                up = anc[i]
                anc[i] = k
                if up == -1:
                    parent[i] = k
                i = up
            if ata:
                prev[Ai[p]] = k
    return parent


def cs_post(parent, n):
    """Postorder of a forest (csparse.py:1711-1742, :2258-2289)."""
    if parent is None:
        return None
    first_child = [-1] * n
    sibling = [-1] * n
    for j in range(n - 1, -1, -1):
        if parent[j] != -1:
            sibling[j] = first_child[parent[j]]
            first_child[parent[j]] = j
    post = []
    for root in range(n):
        if parent[root] != -1:
            continue
        stack = [root]
        while stack:
            c = first_child[stack[-1]]
            if c == -1:
                post.append(stack.pop())
            else:
                first_child[stack[-1]] = sibling[c]
                stack.append(c)
    return post


def cs_counts(A, parent, post, ata):
    """Column counts of L L' = A (ata False: the upper triangle of a square A) or L L' = A'A (ata True), given the elimination
    tree and its postorder (csparse.py:703-764; cs_leaf :1280-1304, _init_ata :677-700).  Host C++ (csx_counts_host): a symbolic
    step in front of the hot path.  None on bad input, like the reference."""
    if not CS_CSC(A) or parent is None or post is None:
        return None
    m, n = A.m, A.n
    if not ata and m != n:
        return None
    p = _csx.i32(A.p[:n + 1])
    i = _csx.i32(A.i[:int(p[n])])
    par, po = _csx.i32(parent[:n]), _csx.i32(post[:n])
    if len(par) < n or len(po) < n:
        return None
    cnt = np.empty(max(n, 1), dtype=np.int32)
    st = _csx.load().csx_counts_host(m, n, _csx.pi(p), _csx.pi(i), _csx.pi(par), _csx.pi(po), 1 if ata else 0, _csx.pi(cnt))
    if st != _csx.OK:
        return None
    return cnt[:n].tolist()


def cs_sqr(order, A, qr):
    """Symbolic ordering and analysis for QR or LU (csparse.py:2187-2217).  order 0 natural, 1 / 2 / 3 as cs_amd.
    LU: only the column ordering S.q and the reference's size guesses.  QR: the column elimination tree, the column
    counts of R and cs_vcount (leftmost, pinv, m2, entries of V) of A Q, in host C++ (csx_sqr_host)."""
    if not CS_CSC(A) or order not in (0, 1, 2, 3):
        return None
    n = A.n
    S = css()
    S.q = cs_amd(order, A)
    if order and S.q is None:
        return None
    S.pinv = None
    if not qr:
        S.unz = S.lnz = 4 * _meta(A)[0] + n
        return S
    m = A.m
    C = cs_permute(A, None, S.q, False) if order else A
    Ap = _csx.i32(C.p[:n + 1])
    nnz = int(Ap[n])
    Ai = _csx.i32(C.i[:nnz]) if nnz else np.zeros(1, np.int32)
    parent, cp = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.int32)
    pinv, leftmost = np.empty(max(m + n, 1), np.int32), np.empty(max(m, 1), np.int32)
    m2, vnz, rnz = _csx.C.c_int32(0), _csx.C.c_int64(0), _csx.C.c_int64(0)
    st = _csx.load().csx_sqr_host(m, n, _csx.pi(Ap), _csx.pi(Ai), _csx.pi(parent), _csx.pi(cp), _csx.pi(pinv),
                                  _csx.pi(leftmost), m2, vnz, rnz)
    if st == _csx.EINVAL:
        raise IndexError("list index out of range")
    _csx.check(st, "csx_sqr_host")
    S.parent, S.cp = parent[:n].tolist(), cp[:n].tolist()
    S.pinv, S.leftmost = pinv[:m + n].tolist(), leftmost[:m].tolist()
    S.m2, S.lnz, S.unz = int(m2.value), int(vnz.value), int(rnz.value)
    return S


def cs_house(x, x_offset, beta, n):
    """Householder reflection (I - beta v v') x = s e1; x is overwritten with v (csparse.py:1238-1261)."""
    if x is None or beta is None:
        return -1
    sigma = 0
    for i in range(1, n):
        sigma += x[x_offset + i] * x[x_offset + i]
    x0 = x[x_offset]
    if sigma == 0:
        s = abs(x0)
        beta[0] = 2.0 if x0 <= 0 else 0.0
        x[x_offset] = 1
    else:
        s = sqrt(x0 * x0 + sigma)
        x[x_offset] = x0 - s if x0 <= 0 else -sigma / (x0 + s)
        beta[0] = -1.0 / (s * x[x_offset])
    return s


def cs_happly(V, i, beta, x):
    """x = (I - beta v v') x with v = V(:, i) (csparse.py:1216-1235)."""
    if not CS_CSC(V) or x is None:
        return False
    Vi, Vx = V.i, V.x
    lo, hi = V.p[i], V.p[i + 1]
    tau = 0
    for p in range(lo, hi):
        tau += Vx[p] * x[Vi[p]]
    tau *= beta
    for p in range(lo, hi):
        x[Vi[p]] -= Vx[p] * tau
    return True


def cs_qr(A, S):
    """Sparse Householder QR, A = Q R (csparse.py:1797-1870).  N.L = V, N.U = R (diagonal last in
    every column), N.B = beta.  Host C++ (csx_qr_host, csx_host.cpp): column by column along the column
    elimination tree, like cs_lu a sequence of data-dependent steps -- except for a square matrix that is a batch of
    small independent blocks, which factors on the device (csx_qr_blocks: one lane per block, same results bit for bit)."""
    if not CS_CSC(A) or S is None:
        return None
    if not _meta(A)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    m, n, m2 = A.m, A.n, S.m2
    q = None if S.q is None else _csx.i32(S.q)
    parent, pinv, leftmost = _csx.i32(S.parent), _csx.i32(S.pinv), _csx.i32(S.leftmost)
    if q is None and m == n and m2 == m and (n >= 4096 or A._dev is not None):
        # a batch of small independent blocks factors on the device, one lane per block running the host code's loop
        # (csx_qr_blocks); anything else comes back with done = 0 and takes the host code below
        beta = np.zeros(max(n, 1))
        hV, hR, done = _csx.new_handle(), _csx.new_handle(), _csx.C.c_int(0)
        with _Resident(A) as dA:
            st = _csx.lib().csx_qr_blocks(dA.handle, _csx.pi(parent), _csx.pi(pinv), _csx.pi(leftmost), m2, hV, hR,
                                          _csx.pd(beta), done)
        if st == _csx.EINVAL:
            raise IndexError("list index out of range")
        _csx.check(st, "csx_qr_blocks")
        if done.value:
            N = csn()
            N.L = _from_device(hV, lambda nnz: max(nnz, 1))
            N.U = _from_device(hR, lambda nnz: max(nnz, 1))
            N.B = beta[:n].tolist()
            N.pinv = None
            return N
    Ap = _csx.i32(A.p[:n + 1])
    nnz = int(Ap[n])
    Ai, Ax = _csx.i32(A.i[:nnz]), _csx.f64(A.x[:nnz])
    vcap, rcap = max(int(S.lnz), 1), max(int(S.unz), 1)
    Vp, Rp = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    Vi, Ri = np.zeros(vcap, np.int32), np.zeros(rcap, np.int32)
    Vx, Rx, beta = np.zeros(vcap), np.zeros(rcap), np.zeros(max(n, 1))
    st = _csx.load().csx_qr_host(m, n, m2, _csx.pi(Ap), _csx.pi(Ai), _csx.pd(Ax), _csx.pi(q), _csx.pi(parent), _csx.pi(pinv),
                                 _csx.pi(leftmost), vcap, rcap, _csx.pi(Vp), _csx.pi(Vi), _csx.pd(Vx), _csx.pi(Rp),
                                 _csx.pi(Ri), _csx.pd(Rx), _csx.pd(beta))
    if st == _csx.EINVAL:
        raise IndexError("list index out of range")
    _csx.check(st, "csx_qr_host")
    N = csn()
    N.L = V = cs_spalloc(m2, n, vcap, True, False)
    N.U = R = cs_spalloc(m2, n, rcap, True, False)
    V.p, V.i, V.x = Vp.tolist(), Vi.tolist(), Vx.tolist()
    R.p, R.i, R.x = Rp.tolist(), Ri.tolist(), Rx.tolist()
    N.B = beta[:n].tolist()
    N.pinv = None
    return N


def _apply_q(N, x, transpose):
    """x <- Q' x (transpose) or Q x for the Householder vectors in N.L / N.B (csx_qr_apply_host)."""
    V = N.L
    n = V.n
    Vp = _csx.i32(V.p[:n + 1])
    vnz = int(Vp[n])
    xv = _csx.f64(x)
    _csx.check(_csx.load().csx_qr_apply_host(n, _csx.pi(Vp), _csx.pi(_csx.i32(V.i[:vnz])), _csx.pd(_csx.f64(V.x[:vnz])),
                                             _csx.pd(_csx.f64(N.B)), 1 if transpose else 0, _csx.pd(xv)), "csx_qr_apply_host")
    x[:] = xv.tolist()


def _square_view(T):
    """R from cs_qr is m2-by-n with nothing below row n: present it as n-by-n to the device solves."""
    if T.m == T.n:
        return T
    V = cs()
    V.m = V.n = T.n
    V.nz, V.nzmax = -1, T.nzmax
    V.p, V.i, V.x = T.p, T.i, T.x
    return V


def cs_qrsol(order, A, b):
    """Least squares (m >= n) or minimum-norm solution (m < n) by QR; b (size max(m, n)) is
    overwritten with x (csparse.py:1875-1912).  The factorisation and the Householder applications
    run on the host, the triangular solves cs_usolve / cs_utsolve on the device."""
    if not CS_CSC(A) or b is None:
        return False
    n, m = A.n, A.m
    if m >= n:
        S = cs_sqr(order, A, True)
        N = cs_qr(A, S) if S is not None else None
        if S is None or N is None:
            return False
        x = xalloc(S.m2)
        cs_ipvec(S.pinv, b, x, m)
        _apply_q(N, x, True)
        cs_usolve(_square_view(N.U), x)
        cs_ipvec(S.q, x, b, n)
    else:
        AT = cs_transpose(A, True)
        S = cs_sqr(order, AT, True)
        N = cs_qr(AT, S) if S is not None else None
        if AT is None or S is None or N is None:
            return False
        x = xalloc(S.m2)
        cs_pvec(S.q, b, x, m)
        cs_utsolve(_square_view(N.U), x)
        _apply_q(N, x, False)
        cs_pvec(S.pinv, x, b, n)
    return True


def apply_q(N, X, transpose=True):
    """X <- Q' X (transpose) or Q X for the Householder vectors of N = cs_qr(A, S), X a dvec block of N.L.m rows
    (cs_happly, csparse.py:1216-1235, for every reflection and every column of X, on the device: csx_happly)."""
    if not isinstance(X, dvec) or X.n < N.L.m:
        raise IndexError("list index out of range")
    beta = dvec(np.asarray(N.B, dtype=np.float64) if len(N.B) else np.zeros(1))
    with _Resident(N.L) as dV:
        _csx.check(_csx.lib().csx_happly(dV.handle, beta.handle, X.handle, X.k, 1 if transpose else 0), "csx_happly")
    return True


def qrsol_factor(A, order=0):
    """Factor once (cs_sqr + cs_qr on the host), solve least-squares problems min ||A x - b|| for blocks of right-hand
    sides on the device: the solve sequence of cs_qrsol for m >= n (csparse.py:1893-1898) -- x = P b, Q' x, solve R x,
    x(q) -- as csx_permute_vec, csx_happly, csx_tri_solve.  solve(B): B a dvec m-by-k block or a list of m entries;
    returns the n-by-k solutions as a new dvec (or overwrites the list's first n entries, like cs_qrsol).  Every column
    is bit-identical to cs_qrsol on that column."""
    if not CS_CSC(A) or A.m < A.n:
        return None
    S = cs_sqr(order, A, True)
    N = cs_qr(A, S) if S is not None else None
    if N is None:
        return None
    m, n, m2 = A.m, A.n, S.m2
    R = cs_pin(_square_view(N.U))
    cs_pin(N.L)

    class _Solver(object):
        factors, symbolic = N, S

        def _block(self, db):
            X = dvec(m2, db.k)                       # zeros: the fictitious rows stay zero
            cs_ipvec(S.pinv, db, X, m)               # x(pinv) = b
            apply_q(N, X, True)
            cs_usolve(R, X)                          # the first n rows of the block
            out = dvec(n, db.k)
            cs_ipvec(S.q, X, out, n)
            return out

        def solve(self, b, comm=None, nrhs=None):
            """comm (a shard.Comm of more than one rank, every rank holding these factors): the block is sharded by
            right-hand-side block (see cholsol_factor) -- the root passes the m-by-K block and gets the n-by-K
            solutions, the other ranks pass None and nrhs = K and get None."""
            if comm is not None and comm.world > 1:
                host = b if (comm.rank == 0 and not isinstance(b, dvec)) else None
                src = dvec(np.asarray(b[:m], dtype=np.float64)) if host is not None else b
                out, _ = _solve_blocks_sharded(comm, src, nrhs, m, n, self._block)
                if host is not None:
                    host[:n] = out.numpy().reshape(-1)[:n].tolist()
                    return True
                return out
            host = None if isinstance(b, dvec) else b
            db = b if isinstance(b, dvec) else dvec(np.asarray(b[:m], dtype=np.float64))
            if db.n < m:
                raise IndexError("list index out of range")
            out = self._block(db)
            if host is not None:
                host[:n] = out.numpy().reshape(-1)[:n].tolist()
                return True
            return out

    return _Solver()


_HQR_INFO = ("m", "n", "m2", "vnz", "rnz", "levels", "launches", "level_launches", "run_launches", "long_columns",
             "zero_diagonals", "breakdown", "kernel_us", "window", "run_levels")


def hqrsol_factor(A, order=0):
    """Factor once by sparse Householder QR ON THE DEVICE, for a matrix in one connected piece: cs_sqr on the
    host, then V, R and beta by csx_hqr_factor -- a wave per column over the height levels of the column elimination tree, on
    patterns known before a value is read.  m >= n factors A (least squares); m < n factors A' (cs_transpose on the device) and
    solves minimum-norm; order goes to cs_sqr as in qrsol_factor.  Householder QR searches for no pivot and is backward stable
    as it stands: no perturbation, no matching; the only breakdown is a non-finite diagonal of R.
    V.p, V.i, R.p, R.i are cs_qr's exactly.  V.x, R.x and beta are byte-equal to csx_hqr_host and the same on every run, but
    equal to cs_qr's ONLY TO ROUNDING: a reflection's dot product is 64 strided partial sums and a fixed tree here, entry by
    entry there.  R is stored n-by-n (nothing of cs_qr's m2-by-n R lies below row n).
    None for a non-CSC A, a failed ordering, or a breakdown.  Otherwise a solver:
    solve(b, trans=False): m >= n: cs_qrsol's first sequence, x(pinv) = b, Q' x, R \\ x, x(q) (qrsol_factor's); m < n: its second,
      x = b(q), R' \\ x, Q x, x(pinv), the minimum-norm solution; trans=True (square A only: A' x = b) is the second sequence on
      A's own factors.  b a list (overwritten with x, True returned) or a dvec block of as many rows as the system has equations
      (a new dvec of the unknowns returned); every column of a block is byte-equal to the list solve.
    refactor(A2): new values on the kept analysis, A2 as for lusol_factor's refactor: True; False with the factors and the
      solves exactly as before on breakdown; ValueError for another pattern or length.  Byte-equal to a fresh factor.
    backward_error(x, b, trans=False), refine(b, maxit=5, trans=False), condest(): _Refinable's and _condest, for a SQUARE A;
      ValueError for a rectangular one (least-squares refinement is not offered).  logabsdet(): the sum of log |r_kk| (math.fsum),
      square A.  info(): m, n, m2 of the factored matrix, vnz, rnz, levels, launches = level_launches + run_launches of the
      last run, long_columns (updated in place: more slots than the LDS `window`), run_levels, zero_diagonals, breakdown,
      kernel_us, min_abs_r, max_abs_r, transposed.  factors: .L = V, .U = R, .B = beta; symbolic: cs_sqr's S.
    batch(values): B value sets on A's pattern factored together in one walk of the levels (_HqrBatch): every
      member's V.x, R.x and beta byte-equal to this factor refactored to that member, batched solves byte-equal to solve() on a
      list, logabsdet() per member."""
    if not CS_CSC(A) or order not in (0, 1, 2, 3):
        return None
    if not _meta(A)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    tall = A.m >= A.n
    Cm = A if tall else cs_transpose(A, True)
    S = cs_sqr(order, Cm, True) if Cm is not None else None
    if S is None:
        return None
    m, n, m2 = Cm.m, Cm.n, S.m2
    square = A.m == A.n
    lib = _csx.lib()
    q = None if S.q is None else _csx.i32(S.q)
    pinv = _csx.i32(S.pinv[:m])
    hF, ok = _csx.new_handle(), _csx.C.c_int(0)
    with _Resident(Cm) as dC:
        st = lib.csx_hqr_factor(dC.handle, _csx.pi(q), _csx.pi(_csx.i32(S.parent)), _csx.pi(pinv), _csx.pi(_csx.i32(S.leftmost)),
                                m2, hF, ok)
    _csx.check(st, "csx_hqr_factor")
    if not ok.value:
        return None
    hV, hR, hB = _csx.new_handle(), _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_hqr_parts(hF, hV, hR, hB), "csx_hqr_parts")
    N = csn()
    (N.L, N.U), _ = _adopt_factor(hF, hV, mats=[hR])     # (R and beta live in the factor that V's wrapper frees)
    devV, devR = N.L._dev, N.U._dev
    N.pinv = None

    def read_beta():
        out = np.zeros(max(n, 1))
        if n:
            _csx.check(lib.csx_vec_download(hB, _csx.pd(out), n), "csx_vec_download")
        return out[:n].tolist()

    N.B = read_beta()
    hq, keep_q = _perm_handle(q, n)
    hp, keep_p = _perm_handle(pinv, m)
    tmap = []                                        # m < n: A's storage order -> A''s, made by the first refactor with values

    def storage_map():
        if not tmap:
            nnz = _meta(A)[0]
            I = cs_spalloc(A.m, A.n, nnz, True, False)
            ap, ai = _pattern_np(A)
            I.p, I.i, I.x = ap.tolist(), (ai.tolist() or [0]), (np.arange(nnz, dtype=np.float64).tolist() or [0.0])
            tmap.append(np.asarray(cs_transpose(I, True).x[:nnz], dtype=np.int64))
        return tmap[0]

    class _Solver(_Refinable):
        factors, symbolic = N, S

        def __init__(self):
            self._devs = (devV, devR)                # keep V, R and the factor alive
            self._fin = weakref.finalize(self, lambda hs: [_csx.free(h) for h in hs if h is not None], [keep_q, keep_p])
            self._A2, self._norm = A, None
            self._refine_init(A, A.n)

        def _block(self, db, second):
            """db: the right-hand sides as a dvec block; second: cs_qrsol's second sequence (R' \\ x, Q x) on these factors"""
            k = db.k
            X = dvec(m2, k)                          # zeros: the fictitious rows stay zero
            if not second:
                _csx.check(lib.csx_permute_vec(hp, db.handle, X.handle, m, k, 1), "csx_permute_vec")     # x(pinv) = b
                _csx.check(lib.csx_happly(devV.handle, hB, X.handle, k, 1), "csx_happly")
                _csx.check(lib.csx_tri_solve(_plan(devR, TRI_U), X.handle, k), "csx_tri_solve")          # the first n rows
                out = dvec(n, k)
                _csx.check(lib.csx_permute_vec(hq, X.handle, out.handle, n, k, 1), "csx_permute_vec")    # x(q) = x
            else:
                _csx.check(lib.csx_permute_vec(hq, db.handle, X.handle, n, k, 0), "csx_permute_vec")     # x = b(q)
                _csx.check(lib.csx_tri_solve(_plan(devR, TRI_UT), X.handle, k), "csx_tri_solve")
                _csx.check(lib.csx_happly(devV.handle, hB, X.handle, k, 0), "csx_happly")
                out = dvec(m, k)
                _csx.check(lib.csx_permute_vec(hp, X.handle, out.handle, m, k, 0), "csx_permute_vec")    # x = x(pinv)
            return out

        def _solve_block(self, blk, trans, from_list):
            out = self._block(blk, bool(trans))
            _csx.check(lib.csx_vec_copy(out.handle, blk.handle), "csx_vec_copy")
            return blk

        def solve(self, b, trans=False):
            if trans and not square:
                raise ValueError("hqrsol_factor: trans=True needs a square matrix")
            second = bool(trans) or not tall
            rows_in, rows_out = (n, m) if second else (m, n)
            host = None if isinstance(b, dvec) else b
            if host is not None and len(host) < rows_in:
                raise IndexError("list index out of range")
            db = b if host is None else dvec(np.asarray(b[:rows_in], dtype=np.float64))
            if db.n < rows_in:
                raise IndexError("list index out of range")
            out = self._block(db, second)
            if host is not None:
                host[:rows_out] = out.numpy().reshape(-1)[:rows_out].tolist()
                return True
            return out

        def refactor(self, A2):
            A2 = _refactor_input(A, A2)
            given = A2
            if not tall:                             # the factored matrix is A': its values in ITS storage order
                if isinstance(A2, cs):
                    given = cs_transpose(A2, True)
                else:
                    given = dvec(A2.numpy().reshape(-1)[storage_map()])
            ok = _csx.C.c_int(0)
            _refactor_call(given, lambda h2: lib.csx_hqr_refactor(hF, h2, ok), ok)
            if ok.value == 1:
                _refactored(N.L, devV)
                _refactored(N.U, devR)
                N.B[:] = read_beta()
                self._A2, self._norm = A2, None
                self._operator_changed()
            return ok.value == 1

        def batch(self, values):
            """B value sets on A's pattern factored together on this factor's analysis -> an _HqrBatch (its docstring has the
            rest).  values: a dvec of nnz x B (read, not kept), a 2-D numpy array of that shape, or a list of B value arrays
            (copied), each in A's storage order (of duplicates the last is taken).  ValueError for another row count, B = 0 or B
            over the limit.  This factor is not changed and goes on working; it must not be freed before the batch, which
            holds on to it."""
            return _HqrBatch(self, hF, _meta(A)[0], (A.m, A.n), None if tall else storage_map, values)

        def _square_only(self, what):
            if not square:
                raise ValueError("hqrsol_factor: %s needs a square matrix (least-squares refinement is not offered)" % what)

        def backward_error(self, x, b, trans=False):
            self._square_only("backward_error")
            return _Refinable.backward_error(self, x, b, trans)

        def refine(self, b, maxit=5, trans=False):
            self._square_only("refine")
            return _Refinable.refine(self, b, maxit, trans)

        def gmres(self, b, restart=16, maxit=64, inner_tol=2.0 ** -26, trans=False):
            self._square_only("gmres")
            return _Refinable.gmres(self, b, restart, maxit, inner_tol, trans)

        def solve_grad(self, x, gx, trans=False, refine=0):
            self._square_only("solve_grad")
            return _Refinable.solve_grad(self, x, gx, trans, refine)

        def condest(self):
            self._square_only("condest")
            if self._norm is None:
                self._norm = _refactor_norm(A, self._A2)
            return _condest(self._norm, lambda v, t: self._block(dvec(v), bool(t)).numpy().reshape(-1), n)

        def logabsdet(self):
            """log |det A| of a square A: the sum of log |r_kk| correctly rounded (math.fsum); -inf with a zero diagonal"""
            self._square_only("logabsdet")
            Rp = np.empty(n + 1, dtype=np.int32)
            x = np.empty(max(devR.info()[2], 1), dtype=np.float64)
            _csx.check(lib.csx_csc_download(devR.handle, _csx.pi(Rp), None, _csx.pd(x)), "csx_csc_download")
            with np.errstate(divide="ignore"):
                return math.fsum(np.log(np.abs(x[Rp[1:] - 1])).tolist())

        def info(self):
            return _factor_info(hF, "csx_hqr_info", _HQR_INFO, "csx_hqr_stats", ("min_abs_r", "max_abs_r"), transposed=not tall)

    return _Solver()


def device_name():
    return _csx.device_info()


# ----------------------------------------------- Dulmage-Mendelsohn family ----

class csd(object):
    """Output of the Dulmage-Mendelsohn decomposition (csparse.py:93-112)."""

    def __init__(self):
        self.p = []     # size m, row permutation
        self.q = []     # size n, column permutation
        self.r = []     # size nb+1, block k is rows r[k] to r[k+1]-1 in A(p,q)
        self.s = []     # size nb+1, block k is cols s[k] to s[k+1]-1 in A(p,q)
        self.nb = 0     # number of blocks in the fine decomposition
        self.rr = []    # coarse row decomposition
        self.cc = []    # coarse column decomposition


def cs_dalloc(m, n):
    """Allocate a csd (csparse.py:2443): p m, r m+6, q n, s n+6, cc and rr 5."""
    D = csd()
    D.p = ialloc(m)
    D.r = ialloc(m + 6)
    D.q = ialloc(n)
    D.s = ialloc(n + 6)
    D.cc = ialloc(5)
    D.rr = ialloc(5)
    return D


def _splitmix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def randperm_array(n, seed):
    """cs_randperm as a numpy int32 array (identity for seed 0).

    The generator: index k gets the key (h(k), k) with h(k) = the upper 32 bits of
    splitmix64(splitmix64(seed mod 2^64) + k); the permutation lists 0..n-1 by ascending key.  seed -1 gives
    n-1..0.  These keys are also the priorities with which cs_maxtrans / cs_dmperm break ties on the device."""
    n = int(n)
    if seed == 0:
        return np.arange(n, dtype=np.int32)
    if seed == -1:
        return np.arange(n - 1, -1, -1, dtype=np.int32)
    sh = _splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF))
    with np.errstate(over="ignore"):
        h = _splitmix64(sh + np.arange(n, dtype=np.uint64)) >> np.uint64(32)
    return np.argsort(h, kind="stable").astype(np.int32)


def cs_randperm(n, seed):
    """Random permutation (csparse.py:1915): None for seed 0 (identity), n-1..0 for -1, otherwise the
    permutation randperm_array documents (the reference's own draw cannot run: SURVEY.md D11)."""
    if seed == 0:
        return None
    return randperm_array(n, seed).tolist()


def maxtrans_array(A, seed=0):
    """Maximum matching as a numpy int32 array of length m + n (cs_maxtrans's jimatch); None if A is not CSC."""
    if not CS_CSC(A):
        return None
    m, n = A.m, A.n
    out = np.empty(m + n, dtype=np.int32)
    rank = _csx.C.c_int32(0)
    with _Resident(A) as dA:
        _csx.check(_csx.lib().csx_maxtrans(dA.handle, int(seed), _csx.pi(out), rank), "csx_maxtrans")
    return out


def cs_maxtrans(A, seed):
    """Maximum transversal (csparse.py:1527): jimatch, length m + n.  jimatch[i] (i < m) is the column matched to
    row i, jimatch[m + j] the row matched to column j, -1 if unmatched.  The matching has maximum cardinality
    (the structural rank) and every pair is an entry of A (stored zeros count).  Which maximum matching comes back
    depends on the seed (cs_randperm's keys set the priorities); it is the same on every call."""
    out = maxtrans_array(A, seed)
    return None if out is None else out.tolist()


def scc_arrays(A):
    """(p, r) numpy int32 arrays of cs_scc; r has nb + 1 entries.  None if A is not CSC or not square."""
    if not CS_CSC(A):
        return None
    if A.m != A.n:
        return None
    n = A.n
    p = np.empty(n, dtype=np.int32)
    r = np.zeros(n + 1, dtype=np.int32)
    nb = _csx.C.c_int32(0)
    with _Resident(A) as dA:
        _csx.check(_csx.lib().csx_scc(dA.handle, _csx.pi(p), _csx.pi(r), nb), "csx_scc")
    return p, r[:nb.value + 1].copy()


def cs_scc(A):
    """Strongly connected components of a square A (csparse.py:1992): a csd with p, r and nb.  A(p,p) is block
    upper triangular -- for every entry (i, j) the block holding row i comes no later than the block holding
    column j -- and each diagonal block r[k] .. r[k+1]-1 is strongly connected.  None if A is not CSC or not square."""
    got = scc_arrays(A)
    if got is None:
        return None
    p, r = got
    D = cs_dalloc(A.m, 0)
    D.p = p.tolist()
    D.r = r.tolist() + [0] * (A.m + 6 - len(r))
    D.nb = len(r) - 1
    return D


def dmperm_arrays(A, seed=0):
    """cs_dmperm as numpy int32 arrays: dict(p, q, r, s, rr, cc, nb) with r and s trimmed to nb + 1 entries.
    None if A is not CSC."""
    if not CS_CSC(A):
        return None
    m, n = A.m, A.n
    p = np.empty(m, dtype=np.int32)
    q = np.empty(n, dtype=np.int32)
    r = np.zeros(m + 6, dtype=np.int32)
    s = np.zeros(n + 6, dtype=np.int32)
    rr = np.zeros(5, dtype=np.int32)
    cc = np.zeros(5, dtype=np.int32)
    nb = _csx.C.c_int32(0)
    with _Resident(A) as dA:
        _csx.check(_csx.lib().csx_dmperm(dA.handle, int(seed), _csx.pi(p), _csx.pi(q), _csx.pi(r), _csx.pi(s), nb,
                                         _csx.pi(rr), _csx.pi(cc)), "csx_dmperm")
    k = nb.value
    return dict(p=p, q=q, r=r[:k + 1].copy(), s=s[:k + 1].copy(), rr=rr, cc=cc, nb=k)


def dmperm_times():
    """Device times (ms) of the last cs_dmperm / cs_maxtrans / cs_scc: initial matching, augmentation, coarse
    decomposition, fine decomposition, whole call."""
    ms = np.zeros(5)
    _csx.check(_csx.lib().csx_dmperm_times(_csx.pd(ms)), "csx_dmperm_times")
    return dict(zip(("matching", "augment", "coarse", "fine", "total"), ms.tolist()))


def dmperm_rounds():
    """Round counts of the last cs_dmperm / cs_maxtrans / cs_scc: augmentation levels (all phases), augmentation
    phases, trim rounds, colouring rounds (at most 2 (m + n + 1) in all), block order rounds."""
    r = np.zeros(5, dtype=np.int64)
    _csx.check(_csx.lib().csx_dmperm_rounds(r.ctypes.data_as(_csx.C.POINTER(_csx.C.c_int64))), "csx_dmperm_rounds")
    return dict(zip(("augment_levels", "augment_phases", "trim", "colour", "order"), r.tolist()))


def cs_dmperm(A, seed):
    """Dulmage-Mendelsohn decomposition (csparse.py:905), laid out as CSparse's: a csd with p (m), q (n), r, s
    (nb + 1 used), nb, rr[5], cc[5]; None if A is not CSC.

    cc = [0, |C0|, |C0|+|C1|, |C0|+|C1|+|C2|, n], rr = [0, |R1|, |R1|+|R2|, |R1|+|R2|+|R3|, m], the structural
    rank is rr[3].  Matched pairs lie on the shifted diagonals of A(p,q): row rr[0]+k with column cc[1]+k, rr[1]+k
    with cc[2]+k, rr[2]+k with cc[3]+k.  Fine blocks: A(R1, C0 C1) if cc[2] > 0, then the strongly connected
    components of A(R2, C2) in block upper triangular order, then A(R3 R0, C3) if rr[2] < m; A(p,q) is block upper
    triangular with respect to r and s.  The coarse sets, the row and column sets of every fine block, nb and the
    structural rank do not depend on the seed; the matching and the order inside a block do."""
    got = dmperm_arrays(A, seed)
    if got is None:
        return None
    m, n, k = A.m, A.n, got["nb"]
    D = cs_dalloc(m, n)
    D.p = got["p"].tolist()
    D.q = got["q"].tolist()
    D.r = got["r"].tolist() + [0] * (m + 6 - (k + 1))
    D.s = got["s"].tolist() + [0] * (n + 6 - (k + 1))
    D.nb = k
    D.rr = got["rr"].tolist()
    D.cc = got["cc"].tolist()
    return D


# ------------------------------------------------------------ block triangular LU --

class btfn(object):
    """Factors of btf_factor: C = A(p, q) = D + F with L U = D(pinv, :) (cs_lu of the block-diagonal part D) and F the
    strictly block upper part, both in C's column storage order.  p, q (n), r (nb + 1: block k is rows / columns r[k] .. r[k+1]-1 of C), levels (nb,
    highest first) and pinv are numpy int32 arrays; L, U, F are `cs` matrices (device-backed)."""

    def __init__(self):
        self.L = self.U = self.F = self.D = None
        self.pinv = self.p = self.q = self.r = self.levels = None


def btf_factor(A, tol=1.0, seed=0):
    """Factor a square, structurally nonsingular A through its block triangular form (KLU's scheme; CSparse's
    cs_dmsol for the square case): dmperm_arrays(A, seed) gives the strongly connected blocks, the blocks are put in
    level order (a block's level: 0 without entries outside it in its rows, else 1 + the largest level those reach;
    highest first), C = A(p, q) is split into its diagonal blocks D and the strictly block upper rest F, and
    cs_lu(D, cs_sqr(0, D, False), tol) factors the blocks (on the device when D is a batch of small blocks).

    solve(b): b a list (one system) or a dvec n-by-k block (k systems), overwritten with x; True.  Every right-hand side
    is solved in one order fixed by the factors: c = b(p); blocks from last to first, c_i -= F_ij z_j
    in cs_gaxpy's order, then the block's part of cs_ipvec(pinv), cs_lsolve(L), cs_usolve(U); x(q) = z.  Lists and
    blocks give the same bits, every run.  One launch per level for the blocks of at most 96 rows.
    solve(b, trans=True) solves A' x = b: C' w = b(q) block lower triangular, x(p) = w; blocks highest level
    first, for every column j c_j = b(q_j) - F(:, j)' w in F's column storage order, then the block's part of
    cs_utsolve(U), cs_ltsolve(L), cs_pvec(pinv).  One order here too; its programs are made on the first transposed solve.
    condest(): an estimate of cond_1(A): cs_norm(A) (cached) times Hager-Higham's estimate of |A^-1|_1 (LAPACK dlacn2).
    .factors: a btfn; .info(): the plan's counts; .factor_ms: wall-clock ms of dmperm, split, cs_lu(D), plan.
    refactor(A2): new values, the same p, q, r, levels and pivots: A2 a CSC `cs` with A's exact pattern, or
    nnz(A) values in A's storage order (numpy, list or dvec); ValueError for another pattern or length.  D and F are gathered
    from A2 as the split does, L and U get the values cs_lu's own loop gives with this pinv (byte-equal to a fresh factor's
    whenever cs_lu(D2) would pivot the same): one wave per block of at most 96 rows, the host for larger blocks.  The forward
    programs are refreshed in place; the transposed ones are made again by the next transposed solve.  True on success;
    False when a kept pivot is 0 or not finite, and then nothing changes.  The first call builds the maps and the schedule.
    refactor_info(): the last refactor's pivot_ratio, device_columns, host_columns and ms.
    backward_error(x, b, trans=False) and refine(b, maxit=5, trans=False): as on lusol_factor's solver.
    None when A is not CSC, not square, structurally singular (sprank < n), or cs_lu(D) returns None (a numerically
    singular block)."""
    if not CS_CSC(A) or A.m != A.n:
        return None
    if not _meta(A)[1]:
        raise TypeError("'NoneType' object is not subscriptable")
    n = A.n
    ms = {}
    t0 = time.perf_counter()
    d = dmperm_arrays(A, seed)
    ms["dmperm"] = 1e3 * (time.perf_counter() - t0)
    if int(d["rr"][3]) < n:
        return None
    nb = d["nb"]
    t0 = time.perf_counter()
    p, q = np.empty(n, np.int32), np.empty(n, np.int32)
    r, levels = np.zeros(nb + 1, np.int32), np.zeros(max(nb, 1), np.int32)
    nlev = _csx.C.c_int32(0)
    hD, hF = _csx.new_handle(), _csx.new_handle()
    with _Resident(A) as dA:
        _csx.check(_csx.lib().csx_btf_split(dA.handle, _csx.pi(d["p"]), _csx.pi(d["q"]), _csx.pi(_csx.i32(d["r"])), nb,
                                            _csx.pi(p), _csx.pi(q), _csx.pi(r), _csx.pi(levels), nlev, hD, hF),
                   "csx_btf_split")
    D = _from_device(hD, lambda nnz: max(nnz, 1))
    F = _from_device(hF, lambda nnz: max(nnz, 1))
    ms["split"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    N = cs_lu(D, cs_sqr(0, D, False), tol)
    if N is None:
        return None
    L, U = cs_pin(N.L), cs_pin(N.U)
    ms["lu"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    fac = btfn()
    fac.L, fac.U, fac.F, fac.D = L, U, F, D
    fac.pinv = np.asarray(N.pinv, dtype=np.int32)
    fac.p, fac.q, fac.r, fac.levels = p, q, r, levels[:nb].copy()
    plan = _csx.new_handle()
    with _Resident(L) as dL, _Resident(U) as dU, _Resident(F) as dF:
        _csx.check(_csx.lib().csx_btf_plan(dL.handle, dU.handle, dF.handle, _csx.pi(fac.pinv), _csx.pi(p), _csx.pi(q),
                                           _csx.pi(r), _csx.pi(levels), nb, plan), "csx_btf_plan")
    ms["plan"] = 1e3 * (time.perf_counter() - t0)

    class _Solver(_Refinable):
        factors = fac
        factor_ms = ms      # host wall-clock of the four factor steps (each ends with a copy to the host or a sync)

        def __init__(self):
            self._fin = weakref.finalize(self, _csx.free, plan)
            # the plan makes the transposed solve's programs from these three on its first call: held while it lives, even
            # when a read of fac.L / .U / .F has turned a lazily downloaded factor into host lists
            self._keep = (L._dev, U._dev, F._dev)
            self._A2, self._norm = A, None         # the matrix condest() is about: A, or the last refactor's A2
            self._prepared, self._rinfo = False, None
            self._refine_init(A, n)

        def _solve_block(self, blk, trans, from_list):
            return self.solve(blk, trans)      # one order for lists and blocks

        def info(self):
            v = np.zeros(8, dtype=np.int64)
            _csx.check(_csx.lib().csx_btf_info(plan, v.ctypes.data_as(_csx.C.POINTER(_csx.C.c_int64))), "csx_btf_info")
            return dict(zip(("blocks", "levels", "max_block", "lnz", "unz", "fnz", "large_blocks", "launches"),
                            v.tolist()))

        def solve(self, b, trans=False):
            db, bhost = _vec_in(b, n, "b")
            work = dvec(n, db.k)
            if trans:
                _csx.check(_csx.lib().csx_btf_solve_trans(plan, db.handle, work.handle, db.k), "csx_btf_solve_trans")
            else:
                _csx.check(_csx.lib().csx_btf_solve(plan, db.handle, work.handle, db.k), "csx_btf_solve")
            _write_back(bhost, db, n * db.k)
            return True

        def condest(self):
            if self._norm is None:
                self._norm = _refactor_norm(A, self._A2)

            def one(v, t):
                d = dvec(v)
                self.solve(d, t)
                return d.numpy()

            return _condest(self._norm, one, n)

        def refactor(self, A2):
            t0 = time.perf_counter()
            A2 = _refactor_input(A, A2)
            ok, ratio, cols = _csx.C.c_int(0), _csx.C.c_double(0.0), (_csx.C.c_int64 * 2)()
            # D's device copy, when it still has one (a host cs_lu of D reads D's lists, which lets it go): D2 is written there
            dD = D._dev
            hD = dD.handle if dD is not None else 0

            def call(h2):
                if self._prepared:
                    st = _csx.lib().csx_btf_refactor(plan, 0, h2, hD, ok, ratio, cols)
                else:
                    with _Resident(A) as dA:      # the first call reads A's pattern: the maps and the schedule
                        st = _csx.lib().csx_btf_refactor(plan, dA.handle, h2, hD, ok, ratio, cols)
                self._prepared = self._prepared or st == _csx.OK
                return st

            _refactor_call(A2, call, ok)
            if ok.value:
                for M, dev in zip((L, U, F), self._keep):
                    _refactored(M, dev)
                if dD is not None:
                    _refactored(D, dD)
                elif D._x is not None:       # D's lists are its only copy: they get D2's values
                    nnz = D._p[n]
                    x = np.empty(max(nnz, 1), dtype=np.float64)
                    _csx.check(_csx.lib().csx_btf_refactor_dx(plan, _csx.pd(x)), "csx_btf_refactor_dx")
                    D._x[:nnz] = x[:nnz].tolist()
                self._A2, self._norm = A2, None
                self._operator_changed()
            self._rinfo = {"ok": bool(ok.value), "pivot_ratio": ratio.value, "device_columns": int(cols[0]),
                           "host_columns": int(cols[1]), "ms": 1e3 * (time.perf_counter() - t0)}
            return bool(ok.value)

        def refactor_info(self):
            return dict(self._rinfo) if self._rinfo is not None else None

    return _Solver()
