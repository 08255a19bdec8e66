"""Tolerances of the parity tests, written down once.

north_star: x[] within 1e-10 relative.  SURVEY 8d gives the measure for one vector against its reference:

    err = max_i |v_i - ref_i| / max(|ref_i|, eps * sum_i|terms|)

-- componentwise relative error, except that a component which cancelled far below the terms it was summed from is held
to the rounding of those terms (`componentwise`).  Where two DIFFERENT factorisations of the same matrix are compared (the
device's Cholesky against the reference's LU, QR against LU, the device's L against the oracle's L) the answers
legitimately differ by the conditioning of the problem: the bound is then `cross_bound(cond)` = max(1e-10, 8 cond_1(A) eps),
with cond_1 estimated from a sparse LU (`cond1`), instead of a round number."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

EPS = 2.0 ** -52
X_RTOL = 1e-10           # BASELINE.json north_star
# The supernodal solve against the oracle on the synthetic factors of tests/sn_cases.py, as the largest
# |x_i - ref_i| / (EPS * terms_i) with cholsolve_terms' terms: 8 x the largest value measured on an MI355X over the cases
# on the near side of the growth guard (4423.03, case bwd513; profiles/snsolve_edges.jsonl has every case).  The results
# are the same bits on every run, so the factor of 8 covers other seeds and a legitimate regrouping of the sums, not noise.
SN_EPS_UNITS = 8 * 4423.03
# The general cs_chol numeric against the oracle on the constructed cases of tests/chol_cases.py, as the largest
# |l_ij - ref_ij| / (EPS * terms_ij) with chol_terms' terms.  NOT taken from the device: 4 x the plain-C oracle's own distance,
# in the same units, from a factorisation of the same matrices in numpy.longdouble, largest over the rounding-route cases
# (738.22, case band176-no-window, second value set; tools/measure_chol_edges.py writes every case to profiles/chol_edges.jsonl).  Two
# results within K of the exact factor differ by at most 2 K; the other factor of 2 is for a regrouping into up to 16 partial
# sums that is less lucky than the reference's order.
CHOL_EPS_UNITS = 4 * 738.22
# The triangular solve in the rounding-equal order (the matrix-core sweep over a forest of small components) against the oracle on
# the cases of tests/tri_cases.py (ROUNDING), as the largest |x_i - ref_i| / (EPS * terms_i) with tri_cases.substitution's terms
# (cholsolve_terms' measure for any kind).  NOT taken from the device: 4 x the plain-C oracle's own distance, in the same units,
# from the same substitution in numpy.longdouble, largest over those cases (3.5346, case rag-lsolve-70; tools/measure_tri_edges.py
# writes every case to profiles/trisolve_edges.jsonl; two solves in a row -- tri_cases.PAIRS -- are measured in the terms of both
# substitutions, tri_cases.two_solves, and stay below that figure).  Two results within K of the exact one differ by at most 2 K; the other
# factor of 2 is for a regrouping of a row's terms that is less lucky than the reference's order.
TRI_EPS_UNITS = 4 * 3.5346


def componentwise(v, ref, terms=None):
    """SURVEY 8d's measure; terms[i] = sum of the magnitudes of the terms ref[i] was formed from (None: |ref| alone).
    Its limit: a component that cancelled to, say, 1e-8 of its terms is still held to 1e-10 of ITSELF (the floor is one
    rounding of the terms, eps * terms), which is a hundredth of a rounding of those terms -- less than any order of
    summation, the reference's included, can keep.  Among a few thousand components that does not occur; among 250 000
    of a solution to a random right-hand side it does (tests/test_gpu_snsolve.py, manufactured_rhs)."""
    v, ref = np.asarray(v, float), np.asarray(ref, float)
    scale = np.abs(ref) if terms is None else np.maximum(np.abs(ref), EPS * np.asarray(terms, float))
    scale = np.where(scale > 0.0, scale, 1.0)
    return float(np.max(np.abs(v - ref) / scale)) if len(ref) else 0.0


def normwise(v, ref):
    ref = np.asarray(ref, float)
    return float(np.max(np.abs(np.asarray(v, float) - ref)) / np.max(np.abs(ref)))


def csc(n, p, i, x, m=None):
    p = np.asarray(p)
    return sp.csc_matrix((np.asarray(x, float)[:p[-1]], np.asarray(i)[:p[-1]], p), shape=(m or n, n))


def cond1(A):
    """1-norm condition estimate of a square sparse matrix (Hager / Higham on a sparse LU)."""
    A = sp.csc_matrix(A)
    lu = spla.splu(A)
    n = A.shape[0]
    inv = spla.LinearOperator((n, n), matvec=lu.solve, rmatvec=lambda b: lu.solve(b, trans="T"))
    return float(spla.onenormest(A) * spla.onenormest(inv))


def cross_bound(cond):
    return max(X_RTOL, 8.0 * cond * EPS)


def cond2_dense(A):
    """2-norm condition number of a small (rectangular) sparse matrix from a dense SVD, rank-deficient directions left out."""
    sv = np.linalg.svd(sp.csc_matrix(A).toarray(), compute_uv=False)
    sv = sv[sv > sv[0] * max(A.shape) * EPS]
    return float(sv[0] / sv[-1])


def lsq_bound(cond2):
    """two QR factorisations of one least-squares / minimum-norm problem: the solution moves with cond_2(A)^2 (Wedin)"""
    return max(X_RTOL, 8.0 * cond2 * cond2 * EPS)


def cholsolve_terms(n, Lp, Li, Lx, y, x):
    """sum|terms| of the LAST substitution of cs_lsolve + cs_ltsolve (csparse.py:1360-1364): x_i = (y_i - sum_j L_ji x_j) / L_ii."""
    L = csc(n, Lp, Li, Lx)
    d = L.diagonal()
    S = abs(L - sp.diags(d))
    return (np.abs(y) + S.T @ np.abs(x)) / np.abs(d)


def chol_update_sums(n, Lp, Li, Lx):
    """sum over k < j of |l_ik l_jk| for every slot (i, j) of L (diagonal first, rows ascending)"""
    Lp, Li, Lx = np.asarray(Lp), np.asarray(Li), np.asarray(Lx, float)
    cols = np.repeat(np.arange(n), np.diff(Lp))
    off = Li != cols
    B = sp.csr_matrix((np.abs(Lx[off]), (Li[off], cols[off])), shape=(n, n))
    P = (B @ B.T).tocsc()
    P.sort_indices()
    keys = cols.astype(np.int64) * n + Li
    pk = np.repeat(np.arange(n, dtype=np.int64), np.diff(P.indptr)) * n + P.indices
    if len(pk) == 0:
        return np.zeros(len(keys))
    at = np.minimum(np.searchsorted(pk, keys), len(pk) - 1)
    return np.where(pk[at] == keys, P.data[at], 0.0)


def chol_terms(n, Lp, Li, Lx, absA):
    """sum|terms| of every entry of a Cholesky factor: l_ij = (a_ij - sum_{k<j} l_ik l_jk) / l_jj (the diagonal: the square
    root of the same sum), so terms_ij = (|a_ij| + sum_k |l_ik l_jk|) / l_jj.  absA: |a_ij| on the slots of L, 0 for fill."""
    Lp, Lx = np.asarray(Lp), np.asarray(Lx, float)
    ljj = np.repeat(Lx[Lp[:-1]], np.diff(Lp))
    return (np.asarray(absA, float) + chol_update_sums(n, Lp, Li, Lx)) / ljj
