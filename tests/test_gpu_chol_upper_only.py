"""cs_chol through a permutation on a matrix stored as its upper triangle alone.  cs_chol reads the upper triangle of A
(csparse.py:2220-2255, cs_symperm inside cs_chol): entry (i, j), i < j, is entry (min, max) of the permuted pair, and lower
entries are ignored.  The device's pattern step used to take, under a permutation, the entries with pinv[i] < pinv[j] whichever
triangle they were stored in, which is the same set only when both triangles are stored: an upper-only matrix at order >= 1 was
refused with a bad-argument status.  Here the upper-only matrix, the fully stored one and one with a foreign lower triangle all
give the factor of the oracle, byte for byte among themselves."""
import numpy as np
import pytest

import chol_refactor_cases as RC
import csparse_oracle as O
import tol as TOL
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu


def _variants(case):
    """(p, i, x) of the upper triangle alone, of both triangles, and of the upper triangle with a lower one of other values"""
    U = case.effective_upper()
    n = case.n
    out = {}
    for kind in ("upper", "full", "foreign-lower"):
        M = U.copy()
        if kind == "full":
            M = U + np.triu(U, 1).T
        elif kind == "foreign-lower":
            M = U + 7.5 * np.triu(U, 1).T
        p, i, x = [0], [], []
        for j in range(n):
            rows = np.nonzero(M[:, j])[0]
            i += rows.tolist()
            x += M[rows, j].tolist()
            p.append(len(i))
        out[kind] = (p, i, x)
    return out


@pytest.mark.parametrize("name", ["grid22", "grid24", "bcsstk01-ordered"])
def test_upper_triangle_alone_under_a_permutation(cs, name):
    case = RC.BY_NAME[name]
    n = case.n
    pinv = np.random.default_rng(3).permutation(n).tolist() if name == "bcsstk01-ordered" else \
        np.argsort(cs.cs_amd(1, case.matrix(cs))).tolist()
    So = RC.oracle_symbolic(O, case, pinv)
    ref = RC.oracle_factor(O, case, "A", So)
    got = {}
    for kind, (p, i, x) in _variants(case).items():
        A = cs.cs_spalloc(n, n, len(i), True, False)
        A.p, A.i, A.x = p, i, x
        S = cs.css()
        S.pinv, S.parent, S.cp, S.lnz = pinv, list(So.parent), list(So.cp), So.cp[n]
        N = cs.cs_chol(A, S)
        assert N is not None, kind
        nnz = N.L.p[n]
        assert np.array_equal(N.L.p, ref[0]) and np.array_equal(N.L.i[:nnz], ref[1]), kind
        got[kind] = np.asarray(N.L.x[:nnz])
        assert TOL.normwise(got[kind], ref[2]) < TOL.X_RTOL, kind
    assert got["upper"].tobytes() == got["full"].tobytes() == got["foreign-lower"].tobytes()
