"""csx_row_view (the rows of a CSC pattern with their storage positions: what the value batches build on the host for the rows of
A and of R) against a restatement in numpy: the entries sorted by (row, column, position), or by row with column
and position descending.  No device."""
import numpy as np
import pytest

import _csx


def model(p, i, descending):
    p, i = np.asarray(p, np.int64), np.asarray(i, np.int64)
    n = len(p) - 1
    col = np.repeat(np.arange(n), np.diff(p))
    pos = np.arange(len(i))
    sign = -1 if descending else 1
    order = np.lexsort((sign * pos, sign * col, i))          # by row, then column, then position
    rp = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))]) if n else np.zeros(1)
    return rp.astype(np.int32), col[order].astype(np.int32), pos[order].astype(np.int32)


def both(p, i):
    out = []
    for descending in (False, True):
        got, want = _csx.row_view(p, i, descending), model(p, i, descending)
        for g, w in zip(got, want):
            assert g.dtype == np.int32 and g.tolist() == w.tolist(), descending
        out.append(got)
    return out


def test_no_column_and_one_entry():
    (rp, rc, rpos), _ = both([0], [])
    assert rp.tolist() == [0] and len(rc) == 0 and len(rpos) == 0
    for rp, rc, rpos in both([0, 1], [0]):
        assert (rp.tolist(), rc.tolist(), rpos.tolist()) == ([0, 1], [0], [0])


def test_an_empty_row_stays_empty():
    # row 1 has no entry: the builder says so (it is the QR batch that refuses a row without its diagonal)
    for rp, rc, rpos in both([0, 2, 2, 3], [0, 2, 2]):
        assert rp.tolist() == [0, 1, 1, 3]
    assert _csx.row_view([0, 2, 2, 3], [0, 2, 2])[1].tolist() == [0, 0, 2]
    assert _csx.row_view([0, 2, 2, 3], [0, 2, 2], True)[1].tolist() == [0, 2, 0]


def test_a_row_stored_twice_in_a_column_keeps_the_direction():
    p, i = [0, 3, 5], [1, 0, 1, 1, 0]                        # column 0 holds row 1 at positions 0 and 2
    asc, desc = both(p, i)
    assert asc[1].tolist() == [0, 1, 0, 0, 1] and asc[2].tolist() == [1, 4, 0, 2, 3]
    assert desc[1].tolist() == [1, 0, 1, 0, 0] and desc[2].tolist() == [4, 1, 3, 2, 0]


@pytest.mark.parametrize("name", ["west-nd", "grid24-shift"])
def test_the_rows_of_r_end_with_the_diagonal(name):
    """R of the Householder QR cases: the diagonal is the last entry of its column and the entries before it come in the order the
    symbolic walk found them (in west-nd that order happens to ascend; in grid24-shift a sixth of the columns do not)"""
    import hqr_cases as HC
    import hqr_oracle as HO
    case = HC.BY_NAME[name]
    _, _, Rp, Ri = HO.pattern_of(case)
    n = case.analysis.n
    Rp, Ri = np.asarray(Rp[:n + 1]), np.asarray(Ri[:Rp[n]])
    unsorted = sum(bool(np.any(np.diff(Ri[Rp[j]:Rp[j + 1]]) < 0)) for j in range(n))
    assert (unsorted > 0) == (name == "grid24-shift")
    _, (rp, rc, rpos) = both(Rp, Ri)
    for r in range(n):
        assert rp[r + 1] > rp[r] and rc[rp[r + 1] - 1] == r and rpos[rp[r + 1] - 1] == Rp[r + 1] - 1
        assert np.all(np.diff(rc[rp[r]:rp[r + 1]]) < 0)


def test_random_patterns():
    rng = np.random.default_rng(39)
    for n in (2, 7, 65):
        counts = rng.integers(0, 6, n)
        p = np.concatenate([[0], np.cumsum(counts)])
        both(p, rng.integers(0, n, p[-1]))                   # unsorted, with repeats


@pytest.mark.parametrize("descending", [0, 1])
def test_bad_arguments_write_nothing(descending):
    lib = _csx.load()
    p, fill = _csx.i32([0, 2, 3]), 77

    def call(p, i, n=2, rp=True):
        out = [np.full(4, fill, np.int32) for _ in range(3)]
        st = lib.csx_row_view(n, _csx.pi(p), _csx.pi(i), descending, _csx.pi(out[0]) if rp else None, _csx.pi(out[1]), _csx.pi(out[2]))
        assert all(o.tolist() == [fill] * 4 for o in out) or st == _csx.OK
        return st

    assert call(p, _csx.i32([0, 1, 1])) == _csx.OK
    assert call(p, _csx.i32([0, 2, 1])) == _csx.EINVAL       # a row past the end, after a good one
    assert call(p, _csx.i32([0, 1, -1])) == _csx.EINVAL
    assert call(_csx.i32([1, 2, 3]), _csx.i32([0, 1, 1])) == _csx.EINVAL
    assert call(_csx.i32([0, 2, 1]), _csx.i32([0, 1, 1])) == _csx.EINVAL
    assert call(p, _csx.i32([0, 1, 1]), n=-1) == _csx.EINVAL
    assert call(None, _csx.i32([0, 1, 1])) == _csx.EINVAL
    assert call(p, None) == _csx.EINVAL
    assert call(p, _csx.i32([0, 1, 1]), rp=False) == _csx.EINVAL
