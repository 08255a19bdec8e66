"""csx_cholsol_forest_plan: the kind of solve plan csx_cholsol_factor makes for a forest of blocks, held to a
model of the table written from its description -- not from the library's code.  No device needed."""
import ctypes as C
import itertools

import pytest

SIZES = [(1, 1), (8, 8), (16, 16), (24, 24), (32, 32), (48, 48), (64, 64), (8, 16), (1, 64), (16, 64)]


def model(sparse, min_bs, max_bs, exact, dense_blocks):
    """the table, row by row"""
    if not dense_blocks:
        return "General"
    if sparse:                                    # small sparse trees, whatever their widths
        return "General" if exact else "BlockListLite"
    equal = min_bs == max_bs and max_bs in (8, 16, 32, 64)
    if equal and not exact:
        return "EmitEqual" if max_bs >= 16 else "Programs"
    if equal:
        return "BlockListExact"
    return "BlockListLite" if exact else "EmitRagged"


@pytest.mark.parametrize("sparse, sizes, exact, dense_blocks", list(itertools.product((0, 1), SIZES, (0, 1), (0, 1))))
def test_library_decides_as_the_table(sparse, sizes, exact, dense_blocks):
    import _csx
    assert _csx.cholsol_forest_plan(sparse, sizes[0], sizes[1], exact, dense_blocks) == model(sparse, *sizes, exact, dense_blocks)


def test_the_table_has_every_kind_and_24_is_not_equal():
    import _csx
    seen = {_csx.cholsol_forest_plan(s, a, b, e, d) for s, (a, b), e, d in itertools.product((0, 1), SIZES, (0, 1), (0, 1))}
    assert seen == set(_csx.FOREST_PLAN_KINDS)
    assert _csx.cholsol_forest_plan(0, 24, 24, 0, 1) == "EmitRagged" and _csx.cholsol_forest_plan(0, 24, 24, 1, 1) == "BlockListLite"
    assert _csx.cholsol_forest_plan(1, 16, 16, 0, 1) == "BlockListLite"       # sparse trees of one width are not equal blocks


def test_bad_arguments():
    import _csx
    lib = _csx.load()
    kind = C.c_int32(-1)
    assert lib.csx_cholsol_forest_plan(0, 17, 16, 0, 1, C.byref(kind)) == _csx.EINVAL      # min_bs > max_bs
    assert lib.csx_cholsol_forest_plan(0, 0, 0, 0, 1, C.byref(kind)) == _csx.EINVAL        # max_bs < 1
    assert lib.csx_cholsol_forest_plan(0, 8, 8, 0, 1, None) == _csx.EINVAL                 # no output
    assert kind.value == -1
