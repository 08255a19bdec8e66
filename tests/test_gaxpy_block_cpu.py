"""gaxpy_block's argument checks that answer before the library is touched (no GPU needed): a matrix that is not
compressed-column, or a missing block, gives False as cs_gaxpy does."""
import numpy as np


def _csc(cs):
    A = cs.cs_spalloc(3, 2, 3, True, False)
    A.p, A.i, A.x = [0, 2, 3], [0, 2, 1], [1.0, -2.0, 3.0]
    return A


def test_non_csc_matrix_returns_false():
    import csparse as cs
    T = cs.cs_spalloc(3, 2, 3, True, True)              # triplet form
    assert cs.gaxpy_block(T, np.ones((2, 4)), np.zeros((3, 4))) is False
    assert cs.gaxpy_block(None, np.ones((2, 4)), np.zeros((3, 4))) is False


def test_missing_blocks_return_false():
    import csparse as cs
    A = _csc(cs)
    Y = np.zeros((3, 4))
    assert cs.gaxpy_block(A, None, Y) is False
    assert cs.gaxpy_block(A, np.ones((2, 4)), None) is False
    assert cs.gaxpy_block(A, None, None) is False
    assert not Y.any()
