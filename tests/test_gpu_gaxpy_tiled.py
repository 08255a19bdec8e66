"""The tiled cs_gaxpy plan (csx_gaxpy_tiled.hip) at every launch shape it ships, with more than one column slab, with more than
one round of row blocks per workgroup, at the largest LDS tile, and at the edges of its group tail and of its 3-byte keys.

Every case comes from tests/tiled_cases.py: its sums are exact in any order (tests/test_tiled_cases_cpu.py checks that on the
CPU), so the kernel, which adds into LDS with atomics in arrival order, is held to the BYTES of the plain-C oracle -- a
dropped, doubled or misplaced entry cannot hide under a tolerance.  The plan's geometry is read back from the library
(csx_gaxpy_plan_geometry / csx_gaxpy_plan_groups) and asserted: a construction that no longer reaches its edge fails.
Through the C ABI with numpy arrays; needs an MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import c_oracle as CO
import tiled_cases as TC
from test_gpu_parity import RTOL, cs, rel_err  # noqa: F401

pytestmark = pytest.mark.gpu

GEO = ("row_block", "nrb", "nslab", "slab_cols", "rb_bits", "ngroups", "key_bytes", "shape", "groups_min", "groups_max")


@pytest.fixture(scope="module")
def lib(cs):
    import _csx
    return _csx.lib()


@pytest.fixture(scope="module")
def cus(lib):
    import _csx
    return _csx.device_info()[1]


@functools.lru_cache(maxsize=None)
def built(builder, *args):
    """the case (or list of cases) of tiled_cases.<builder>(*args), made once"""
    return getattr(TC, builder)(*args)


_refs = {}


def oracle(case):
    """c_oracle.gaxpy of a case, computed once (cases are read-only and live as long as the module)"""
    if id(case) not in _refs:
        ref = CO.gaxpy(*case)
        ref.setflags(write=False)
        _refs[id(case)] = (case, ref)
    return _refs[id(case)][1]


def upload(lib, case):
    import _csx
    m, n, Ap, Ai, Ax, x, y0 = case
    hA = _csx.new_handle()
    _csx.check(lib.csx_csc_upload(m, n, _csx.pi(Ap), _csx.pi(Ai), _csx.pd(Ax), hA), "csx_csc_upload")
    return hA


def vec(lib, a):
    import _csx
    h = _csx.new_handle()
    _csx.check(lib.csx_vec_upload(_csx.pd(np.ascontiguousarray(a)), a.size, h), "csx_vec_upload")
    return h


def gaxpy(lib, hA, x, y0, mode, times=1):
    """y0 += A x `times` times on the device; the result as a numpy array"""
    import _csx
    hx, hy = vec(lib, x), vec(lib, y0)
    try:
        for _ in range(times):
            _csx.check(lib.csx_gaxpy(hA, hx, hy, mode), "csx_gaxpy")
        y = np.empty(y0.size)
        _csx.check(lib.csx_vec_download(hy, _csx.pd(y), y.size), "csx_vec_download")
    finally:
        _csx.free(hx)
        _csx.free(hy)
    return y


def geometry(lib, hA):
    import _csx
    info = (C.c_int64 * 10)()
    _csx.check(lib.csx_gaxpy_plan_geometry(hA, info), "csx_gaxpy_plan_geometry")
    geo = dict(zip(GEO, (int(v) for v in info)))
    groups = np.zeros(geo["nrb"], np.int32)
    _csx.check(lib.csx_gaxpy_plan_groups(hA, _csx.pi(groups)), "csx_gaxpy_plan_groups")
    geo["groups"] = groups.tolist()
    assert (geo["groups_min"], geo["groups_max"]) == (min(geo["groups"]), max(geo["groups"]))
    assert sum(geo["groups"]) == geo["ngroups"]
    kb = C.c_int(0)
    _csx.check(lib.csx_gaxpy_plan_info(hA, None, None, kb))
    assert kb.value == geo["key_bytes"]
    return geo


def prepared(lib, cs, case, cus, keys24=1):
    """the matrix on the device with its tiled plan built under "gaxpy.keys24" = keys24; the plan's geometry, which must be the
    mirror's (tiled_cases.plan) in every field"""
    import _csx
    hA = upload(lib, case)
    with _csx.option("gaxpy.keys24", keys24):
        _csx.check(lib.csx_gaxpy_prepare(hA, cs.GAXPY_TILED), "csx_gaxpy_prepare")
    geo = geometry(lib, hA)
    want = TC.plan(case[0], case[1], cus, case[2], case[3])
    for k in ("row_block", "nrb", "nslab", "slab_cols", "rb_bits", "ngroups"):
        assert geo[k] == want[k], k
    assert geo["groups"] == want["groups"].tolist()
    assert geo["key_bytes"] == (want["key_bytes"] if keys24 else 4)
    return hA, geo


def same_bytes(got, case):
    ref = oracle(case)
    if got.tobytes() != ref.tobytes():
        bad = np.flatnonzero(got != ref)
        raise AssertionError("%d of %d rows differ from the oracle, first at row %d: got %r, want %r (y0 %r)"
                             % (bad.size, ref.size, bad[0], got[bad[0]], ref[bad[0]], case[6][bad[0]]))


# ------------------------------------------------------------------------------------------------ the option and the query

def test_shape_option_and_geometry_query(lib, cs, cus):
    import _csx
    v = C.c_int(99)
    _csx.check(lib.csx_get_option(b"gaxpy.shape", v))
    assert v.value == -1                                              # the default: the plan's own shape
    try:
        for given, kept in ((0, 0), (3, 3), (4, -1), (-5, -1), (2, 2), (-1, -1)):
            _csx.check(lib.csx_set_option(b"gaxpy.shape", given))
            _csx.check(lib.csx_get_option(b"gaxpy.shape", v))
            assert v.value == kept
    finally:
        _csx.check(lib.csx_set_option(b"gaxpy.shape", -1))
    hA = upload(lib, built("group_ladder", cus, 0))
    info = (C.c_int64 * 10)()
    try:
        assert lib.csx_gaxpy_plan_geometry(hA, info) == _csx.EINVAL   # no tiled plan yet
        assert lib.csx_gaxpy_plan_groups(hA, _csx.pi(np.zeros(cus, np.int32))) == _csx.EINVAL
        _csx.check(lib.csx_gaxpy_prepare(hA, cs.GAXPY_EXACT))
        assert lib.csx_gaxpy_plan_geometry(hA, info) == _csx.EINVAL   # the row plan is not the tiled plan
        _csx.check(lib.csx_gaxpy_prepare(hA, cs.GAXPY_TILED))
        assert lib.csx_gaxpy_plan_geometry(hA, None) == _csx.EINVAL
        assert geometry(lib, hA)["shape"] == 0                        # not tuned, not forced: 4 x 5
        for s in range(4):
            with _csx.option("gaxpy.shape", s):
                assert geometry(lib, hA)["shape"] == s                # read when asked, not when the plan was built
        shape = C.c_int(7)
        _csx.check(lib.csx_gaxpy_plan_shape(hA, shape, None))
        assert shape.value == -1                                      # the plan's own pick is untouched by the option
    finally:
        _csx.free(hA)


# ------------------------------------------------------------------------------------------------------- the launch shapes

@pytest.mark.parametrize("keys24", [1, 0])
@pytest.mark.parametrize("shape", range(4))
def test_group_ladder_at_each_shape(lib, cs, cus, shape, keys24):
    """groups per row block 0, 1, 2, NW - 1 .. NW + 1, NW NG - 1 .. NW NG + 1, 2 NW NG - 1 .. 2 NW NG + 1 of this shape, the last
    group full, one entry short and of a single entry: the clamp of the group index and the guards of the tail"""
    import _csx
    case = built("group_ladder", cus, shape)
    hA, geo = prepared(lib, cs, case, cus, keys24)
    try:
        assert (geo["row_block"], geo["nrb"], geo["nslab"], geo["key_bytes"]) == (8, cus, 1, 3 if keys24 else 4)
        assert geo["groups"] == [G for G, r in TC.ladder_groups(cus, shape)]
        with _csx.option("gaxpy.shape", shape):
            assert geometry(lib, hA)["shape"] == shape
            same_bytes(gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED), case)
    finally:
        _csx.free(hA)


@pytest.mark.parametrize("keys24", [1, 0])
def test_one_plan_runs_at_all_four_shapes(lib, cs, cus, keys24):
    import _csx
    case = built("group_ladder", cus, 2)             # the ladder with the most groups per row block (8 x 4)
    hA, geo = prepared(lib, cs, case, cus, keys24)
    try:
        out = {}
        for s in (-1, 0, 1, 2, 3):
            with _csx.option("gaxpy.shape", s):
                assert geometry(lib, hA)["shape"] == max(s, 0)
                out[s] = gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED)
            same_bytes(out[s], case)
        assert len({y.tobytes() for y in out.values()}) == 1
    finally:
        _csx.free(hA)


# ------------------------------------------------------------------------------------------------------------------- slabs

@pytest.mark.parametrize("keys24", [1, 0])
@pytest.mark.parametrize("shape", [0, 2])
def test_three_column_slabs(lib, cs, cus, shape, keys24):
    """the slab of a group (info >> 9), the tile of an entry (b nslab + s) and the x base (slab slab_cols) with nslab = 3, padding
    between the tiles of one row block, a last slab of 5 columns and a last row block of one row"""
    import _csx
    case = built("slabs", cus)
    hA, geo = prepared(lib, cs, case, cus, keys24)
    try:
        assert (geo["nslab"], geo["slab_cols"], geo["key_bytes"]) == (3, 131072, 3 if keys24 else 4)
        assert geo["nrb"] * geo["row_block"] > case[0] and geo["groups_min"] >= 3
        with _csx.option("gaxpy.shape", shape):
            same_bytes(gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED), case)
    finally:
        _csx.free(hA)


# --------------------------------------------------------------------------------------------------------------- key edges

@pytest.mark.parametrize("keys24", [1, 0])
@pytest.mark.parametrize("which", range(3))
def test_key_width_decision_at_its_edge(lib, cs, cus, which, keys24):
    """a run of 64 that is 511 columns wide (3-byte keys, the offset with every bit set), 512 wide (4-byte keys), and two narrow
    runs of a wide tile (3-byte keys, the second run gathered from its own base column)"""
    label, kb, case = built("key_edges", cus)[which]
    hA, geo = prepared(lib, cs, case, cus, keys24)
    try:
        assert geo["key_bytes"] == (kb if keys24 else 4), label
        assert (geo["ngroups"], geo["nslab"], geo["groups_max"]) == (1, 1, 1)
        same_bytes(gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED), case)
    finally:
        import _csx
        _csx.free(hA)


# --------------------------------------------------------------------------------------------------------------- LDS edges

@pytest.mark.parametrize("two_rounds", [False, True])
def test_largest_lds_tile_and_two_rounds(lib, cs, cus, two_rounds):
    """m = cus * 20446: one row block per workgroup, each of the most rows the LDS tile holds (163 584 bytes of dynamic LDS),
    with the saturated 3-byte key (local row 20445, run offset 511).  One row more: every workgroup walks two row blocks, so
    the tile is reloaded after it was written back; one workgroup's first block is empty."""
    import _csx
    case = built("lds_edges", cus, two_rounds)
    hA, geo = prepared(lib, cs, case, cus)
    try:
        assert geo["key_bytes"] == 3 and geo["nslab"] == 1
        if not two_rounds:
            assert geo["row_block"] == 20446 and geo["nrb"] == cus and geo["rb_bits"] == 15
            assert TC.plan(case[0], case[1], cus, case[2], case[3])["saturated"]
        else:
            assert geo["nrb"] > cus and geo["row_block"] < 20446
            assert geo["groups"][3] == 0 and geo["groups"][3 + cus] > 0
        with _csx.option("gaxpy.shape", 0):
            same_bytes(gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED), case)
    finally:
        _csx.free(hA)


# -------------------------------------------------------------------------------------------------------------- degenerate

@pytest.mark.parametrize("which", range(7))
def test_degenerate_shapes(lib, cs, cus, which):
    import _csx
    label, case = built("degenerate", cus)[which]
    hA, geo = prepared(lib, cs, case, cus)
    try:
        if label == "no_entries":
            assert geo["ngroups"] == 0 and geo["key_bytes"] == 4
        got = gaxpy(lib, hA, case[5], case[6], cs.GAXPY_TILED)
        same_bytes(got, case)
        if label == "no_entries":
            assert got.tobytes() == case[6].tobytes()                 # y untouched
        for mode in (cs.GAXPY_EXACT, cs.GAXPY_WAVE, cs.GAXPY_ATOMIC):
            same_bytes(gaxpy(lib, hA, case[5], case[6], mode), case)
    finally:
        _csx.free(hA)


# ------------------------------------------------------------------------------------------------------------ accumulation

@pytest.mark.parametrize("name", ["group_ladder", "slabs"])
def test_y_is_accumulated_not_overwritten(lib, cs, cus, name):
    """a second call with 2 x onto the first call's result: y0 + 3 A x on the integer class, and the oracle applied twice on
    every row"""
    import _csx
    case = built(name, cus, 0) if name == "group_ladder" else built(name, cus)
    m, n, Ap, Ai, Ax, x, y0 = case
    y1 = oracle(case)
    hA, geo = prepared(lib, cs, case, cus)
    try:
        got = gaxpy(lib, hA, 2.0 * x, y1, cs.GAXPY_TILED)
    finally:
        _csx.free(hA)
    assert got.tobytes() == CO.gaxpy(m, n, Ap, Ai, Ax, 2.0 * x, y1).tobytes()
    ints = TC.is_integer_row(case)
    assert got[ints].tobytes() == (y0 + 3.0 * (y1 - y0))[ints].tobytes()
    assert np.count_nonzero(y1[ints] != y0[ints]) > ints.sum() // 4


# ------------------------------------------------------------------------------------------- the other modes, same cases

@pytest.mark.parametrize("mode", ["WAVE", "ATOMIC", "EXACT", "AUTO"])
@pytest.mark.parametrize("name", ["ladder0", "ladder1", "ladder2", "ladder3", "slabs"])
def test_other_modes_give_the_same_bytes(lib, cs, cus, name, mode):
    import _csx
    case = built("slabs", cus) if name == "slabs" else built("group_ladder", cus, int(name[-1]))
    hA = upload(lib, case)
    try:
        same_bytes(gaxpy(lib, hA, case[5], case[6], getattr(cs, "GAXPY_" + mode)), case)
    finally:
        _csx.free(hA)


@pytest.mark.parametrize("avg", TC.DENSITIES)
def test_row_kernels_at_every_density_class(lib, cs, avg):
    """GAXPY_WAVE picks its kernel and lane-group width from the average entries per row, thresholds at 6, 12, 24 and 48:
    one matrix either side of each"""
    import _csx
    case = built("density_ladder", avg)
    hA = upload(lib, case)
    try:
        for mode in (cs.GAXPY_WAVE, cs.GAXPY_AUTO, cs.GAXPY_EXACT):
            same_bytes(gaxpy(lib, hA, case[5], case[6], mode), case)
    finally:
        _csx.free(hA)


# --------------------------------------------------------------------------------------------------------------- the tuner

def test_tuner_times_four_shapes_and_the_plan_stays_right(lib, cs):
    """csx_gen_grand(262144, 64): 2^24 entries, the least the tuner times.  Random values, so this is the one tolerance of the
    file, and it is test_gpu_parity's: rel_err against the absolute-terms scale below RTOL, with GAXPY_EXACT on the device as
    the reference (all values positive: the absolute terms of a row sum to the row's result)."""
    import _csx
    n, per_col = 262144, 64
    hA, hx = _csx.new_handle(), _csx.new_handle()
    old = C.c_int(0)
    _csx.check(lib.csx_get_option(b"gaxpy.tune_shape", old))
    try:
        _csx.check(lib.csx_gen_grand(n, per_col, 20240607, hA))
        _csx.check(lib.csx_gen_vec(n, 7, 0.5, 1.5, hx))
        _csx.check(lib.csx_set_option(b"gaxpy.tune_shape", 1))
        _csx.check(lib.csx_gaxpy_prepare(hA, cs.GAXPY_TILED))
        shape, ms = C.c_int(-7), (C.c_double * 4)()
        _csx.check(lib.csx_gaxpy_plan_shape(hA, shape, ms))
        assert shape.value in (0, 1, 2, 3) and all(t > 0 for t in ms)
        assert ms[shape.value] == min(ms)
        geo = geometry(lib, hA)
        assert geo["shape"] == shape.value and geo["ngroups"] * 256 >= n * per_col
        x = np.empty(n)
        _csx.check(lib.csx_vec_download(hx, _csx.pd(x), n))
        zero = np.zeros(n)
        ref = gaxpy(lib, hA, x, zero, cs.GAXPY_EXACT)
        assert np.all(np.isfinite(ref)) and ref.min() > 0
        got = gaxpy(lib, hA, x, zero, cs.GAXPY_TILED)
        assert rel_err(got, ref, ref) < RTOL
        for s in range(4):                                            # and every candidate it timed computes the same
            with _csx.option("gaxpy.shape", s):
                assert rel_err(gaxpy(lib, hA, x, zero, cs.GAXPY_TILED), ref, ref) < RTOL, s
    finally:
        _csx.check(lib.csx_set_option(b"gaxpy.tune_shape", old.value))
        _csx.free(hA)
        _csx.free(hx)
