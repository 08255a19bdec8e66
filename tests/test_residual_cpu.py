"""csx_residual_host (the value rule of csx_residual_block on host arrays) against the Python restatement
tests/residual_oracle.py: byte-equal R, omega and rnorm on every golden matrix and on seeded values of magnitudes
1e-8 .. 1e8, both directions, k = 1 and 3; the two mistakes the restatement keeps (a fused multiply-add, the reversed
order) give other bytes on those inputs; the special cases of the rule; and the argument checks of residual_block that
answer before the library is touched.  No GPU."""
import numpy as np
import pytest

import residual_oracle as RO
from conftest import golden

GOLDEN = ("t1", "west0067", "bcsstk01", "bcsstk16", "ash219", "lp_afiro", "fs_183_1", "ibm32a", "ibm32b", "mbeacxc")
KS = (1, 3)


def _matrix(name):
    """cs_compress's output of the fixture: unsorted columns, duplicates kept"""
    g = golden(name)
    m, n = int(g["A_mn"][0]), int(g["A_mn"][1])
    p = g["A_p"].astype(np.int32)
    nnz = int(p[n])
    return m, n, p, g["A_i"][:nnz].astype(np.int32), g["A_x"][:nnz].astype(np.float64)


def _wide(rng, count):
    """signed values of magnitudes 1e-8 .. 1e8"""
    return rng.choice([-1.0, 1.0], count) * 10.0 ** rng.uniform(-8.0, 8.0, count)


def _host(m, n, p, i, x, k, trans, X, B, store=True, in_place=False):
    import _csx
    lib = _csx.load()
    rows = n if trans else m
    X, B = np.ascontiguousarray(X, dtype=np.float64), np.array(B, dtype=np.float64)
    R = B if in_place else (np.full(rows * k, 7.0) if store else None)
    omega, rnorm = np.full(k, -1.0), np.full(k, -1.0)
    st = lib.csx_residual_host(m, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), k, 1 if trans else 0, _csx.pd(X), _csx.pd(B),
                               _csx.pd(R), _csx.pd(omega), _csx.pd(rnorm))
    assert st == _csx.OK
    return R, omega, rnorm


def _inputs(name, k, trans, seeded):
    m, n, p, i, x = _matrix(name)
    rng = np.random.default_rng(1000 * k + 10 * len(name) + (1 if trans else 0) + (100 if seeded else 0))
    rows, cols = (n, m) if trans else (m, n)
    if seeded:
        x = _wide(rng, len(x))
        X, B = _wide(rng, cols * k), _wide(rng, rows * k)
    else:
        X, B = rng.standard_normal(cols * k) * 4.0, rng.standard_normal(rows * k)
    return m, n, p, i, x, X, B


def _same(got, ref):
    return np.asarray(got, dtype=np.float64).tobytes() == np.asarray(ref, dtype=np.float64).tobytes()


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("trans", [False, True])
def test_host_rule_is_the_restatement(name, trans):
    for seeded in (False, True):
        for k in KS:
            m, n, p, i, x, X, B = _inputs(name, k, trans, seeded)
            R, omega, rnorm = _host(m, n, p, i, x, k, trans, X, B)
            Rr, wr, ar = RO.residual(m, n, p, i, x, k, trans, X, B)
            assert _same(R, Rr), (name, k, seeded)
            assert _same(omega, wr) and _same(rnorm, ar), (name, k, seeded)
            # omega and rnorm alone, and in place: the same numbers
            none, w2, a2 = _host(m, n, p, i, x, k, trans, X, B, store=False)
            assert none is None and _same(w2, wr) and _same(a2, ar)
            R3, w3, a3 = _host(m, n, p, i, x, k, trans, X, B, in_place=True)
            assert _same(R3, Rr) and _same(w3, wr) and _same(a3, ar)


@pytest.mark.parametrize("name", [g for g in GOLDEN if g not in ("bcsstk16", "mbeacxc")])
@pytest.mark.parametrize("trans", [False, True])
def test_a_fused_or_reversed_fold_gives_other_bytes(name, trans):
    """on the inputs of the test above (the two largest matrices left to it: exact rational arithmetic is slow)"""
    k = 3
    m, n, p, i, x, X, B = _inputs(name, k, trans, True)
    right = _host(m, n, p, i, x, k, trans, X, B)[0]
    fused = RO.residual(m, n, p, i, x, k, trans, X, B, fused=True)[0]
    rev = RO.residual(m, n, p, i, x, k, trans, X, B, reverse=True)[0]
    assert not _same(fused, right), name
    assert not _same(rev, right), name


def test_zero_rows_and_empty_rows():
    p, i, x = np.array([0, 1, 1], np.int32), np.array([0], np.int32), np.array([2.0])
    # A = [[2, 0], [0, 0]]: row 1 is empty.  b = (2, 0): both residuals 0, the second 0 / 0 -> ratio 0
    R, omega, rnorm = _host(2, 2, p, i, x, 1, False, [1.0, 5.0], [2.0, 0.0])
    assert R.tolist() == [0.0, 0.0] and omega.tolist() == [0.0] and rnorm.tolist() == [0.0]
    # b = (2, 3): the empty row has r = 3 over d = 3 -> ratio 1
    R, omega, rnorm = _host(2, 2, p, i, x, 1, False, [1.0, 5.0], [2.0, 3.0])
    assert R.tolist() == [0.0, 3.0] and omega.tolist() == [1.0] and rnorm.tolist() == [3.0]
    # transposed: column 1 of A is the empty row 1 of A'
    R, omega, rnorm = _host(2, 2, p, i, x, 1, True, [1.0, 5.0], [2.0, 3.0])
    assert R.tolist() == [0.0, 3.0] and omega.tolist() == [1.0] and rnorm.tolist() == [3.0]
    for got, ref in zip(_host(2, 2, p, i, x, 1, False, [1.0, 5.0], [2.0, 3.0]),
                        RO.residual(2, 2, p, i, x, 1, False, [1.0, 5.0], [2.0, 3.0])):
        assert _same(got, ref)
    # a zero term on a row with b = 0 and x = 0: 0 / 0 again, and the sign of the zero residual is the rule's
    R, omega, _ = _host(2, 2, p, i, x, 1, False, [-0.0, 0.0], [0.0, -0.0])
    Rr, wr, _ = RO.residual(2, 2, p, i, x, 1, False, [-0.0, 0.0], [0.0, -0.0])
    assert _same(R, Rr) and omega.tolist() == [0.0] == wr


@pytest.mark.parametrize("trans", [False, True])
def test_a_nan_stays_in_its_column(trans):
    k = 3
    m, n, p, i, x, X, B = _inputs("west0067", k, trans, False)
    X = X.copy()
    X[5 * k + 1] = np.nan
    R, omega, rnorm = _host(m, n, p, i, x, k, trans, X, B)
    Rr, wr, ar = RO.residual(m, n, p, i, x, k, trans, X, B)
    assert np.isnan(omega[1]) and np.isnan(rnorm[1]) and np.isnan(wr[1]) and np.isnan(ar[1])
    assert np.isfinite(omega[[0, 2]]).all() and np.isfinite(rnorm[[0, 2]]).all()
    R, Rr = R.reshape(-1, k), np.asarray(Rr).reshape(-1, k)
    for c in (0, 2):
        assert _same(R[:, c], Rr[:, c]) and _same(omega[c], wr[c]) and _same(rnorm[c], ar[c])
    assert np.array_equal(np.isnan(R[:, 1]), np.isnan(Rr[:, 1])) and np.isnan(R[:, 1]).any()
    # an inf residual over a finite denominator is inf, not NaN; inf ranks below NaN
    p1, i1, x1 = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1e300])
    _, omega, rnorm = _host(1, 1, p1, i1, x1, 2, trans, [1e300, 1.0], [1.0, 1.0])
    assert np.isnan(omega[0]) and rnorm[0] == np.inf and omega[1] == 1.0     # inf / inf; (1e300 - 1) / (1e300 + 1)
    assert _same(omega, RO.residual(1, 1, p1, i1, x1, 2, trans, [1e300, 1.0], [1.0, 1.0])[1])


def test_operators_without_rows_or_entries():
    k = 2
    none = np.zeros(0, np.int32)
    # 0 x 3 (forward: no rows) and 3 x 0 (transposed: no rows)
    for m, n, trans in ((0, 3, False), (3, 0, True)):
        p = np.zeros(n + 1, np.int32)
        R, omega, rnorm = _host(m, n, p, none, np.zeros(0), k, trans, np.ones(3 * k), np.zeros(0))
        assert R.size == 0 and omega.tolist() == [0.0, 0.0] and rnorm.tolist() == [0.0, 0.0]
        assert RO.residual(m, n, p, none, [], k, trans, [1.0] * (3 * k), [])[1:] == ([0.0, 0.0], [0.0, 0.0])
    # rows but no entries: R = B, omega by the 0 / 0 rule, rnorm = max |B|
    B = np.array([0.0, -3.0, 0.0, 2.0, 0.0, 0.5])
    for m, n, trans in ((3, 0, False), (0, 3, True), (3, 4, False), (4, 3, True)):
        p = np.zeros(n + 1, np.int32)
        cols = m if trans else n
        R, omega, rnorm = _host(m, n, p, none, np.zeros(0), k, trans, np.ones(max(cols, 1) * k), B)
        assert _same(R, B) and omega.tolist() == [0.0, 1.0] and rnorm.tolist() == [0.0, 3.0]


def test_host_rule_rejects_bad_arguments():
    import _csx
    lib = _csx.load()
    p, i, x = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([1.0, 2.0])
    X, B, w = np.ones(2), np.ones(2), np.zeros(1)

    def call(m, n, pp, ii, k):
        return lib.csx_residual_host(m, n, _csx.pi(pp), _csx.pi(ii), _csx.pd(x), k, 0, _csx.pd(X), _csx.pd(B), None,
                                     _csx.pd(w), None)

    assert call(2, 2, p, i, 1) == _csx.OK
    assert call(2, 2, p, i, 0) == _csx.EINVAL
    assert call(-1, 2, p, i, 1) == _csx.EINVAL
    assert call(2, 2, np.array([0, 2, 1], np.int32), i, 1) == _csx.EINVAL      # p decreases
    assert call(2, 2, p, np.array([0, 2], np.int32), 1) == _csx.EINVAL         # a row index past m


def test_residual_block_answers_bad_arguments_without_the_device():
    import csparse as cs
    A = cs.cs_spalloc(3, 2, 3, True, False)
    A.p, A.i, A.x = [0, 2, 3], [0, 2, 1], [1.0, -2.0, 3.0]
    T = cs.cs_spalloc(3, 2, 3, True, True)
    assert cs.residual_block(T, np.ones((2, 4)), np.ones((3, 4))) is False
    assert cs.residual_block(None, np.ones((2, 4)), np.ones((3, 4))) is False
    assert cs.residual_block(A, None, np.ones((3, 4))) is False and cs.residual_block(A, np.ones((2, 4)), None) is False
    assert cs.residual_block(A, np.ones((2, 4)), np.ones((3, 5))) is False      # unequal k
    assert cs.residual_block(A, [1.0, 1.0], np.ones((3, 2))) is False
    with pytest.raises(IndexError):
        cs.residual_block(A, np.ones((1, 4)), np.ones((3, 4)))
    with pytest.raises(IndexError):
        cs.residual_block(A, np.ones((2, 4)), np.ones((2, 4)))
    with pytest.raises(IndexError):                                               # transposed: X needs m rows, B n rows
        cs.residual_block(A, np.ones((2, 4)), np.ones((2, 4)), trans=True)
    with pytest.raises(IndexError):
        cs.residual_block(A, [1.0, 1.0, 1.0], [1.0], trans=True)
    P = cs.cs_spalloc(3, 2, 3, False, False)
    P.p, P.i = [0, 2, 3], [0, 2, 1]
    with pytest.raises(TypeError):
        cs.residual_block(P, np.ones((2, 4)), np.ones((3, 4)))
    with pytest.raises(TypeError):
        cs.residual_block(A, np.ones((2, 2, 2)), np.ones((3, 4)))
