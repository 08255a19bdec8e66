"""The integer primitives of csx_sort.hip on the device, one at a time through the csx_prim_* entry points, over the table of
tests/sort_cases.py: every result against plain numpy bit for bit (np.cumsum, the reversed np.minimum.accumulate, np.repeat,
np.searchsorted, the stable np.argsort applied to keys and payloads), every input read back as it went in, and the decisions
csx_prim_sort_info reports against the Python model field for field.  tests/test_sort_cases_cpu.py shows without a device that
the table sits on the edges it names.  Needs an MI355X."""
import numpy as np
import pytest

import c_oracle as CO
import sort_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def csx():
    import _csx
    _csx.init()
    return _csx


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("name", SC.NAMES["scan"])
def test_scan(csx, name, in_place):
    values = SC.inputs(name)["values"]
    ref = np.concatenate([[0], np.cumsum(values, dtype=np.int64)])
    assert ref[-1] <= SC.MAXINT
    out, total, back = csx.prim_scan(values, in_place)
    assert same_bits(out, ref.astype(np.int32)) and total == int(ref[-1])
    assert in_place or same_bits(back, values)


@pytest.mark.parametrize("name", SC.NAMES["sufmin"])
def test_suffix_min(csx, name):
    values = SC.inputs(name)["values"]
    ref = np.minimum.accumulate(values[::-1])[::-1]
    assert same_bits(csx.prim_suffix_min(values), np.ascontiguousarray(ref))


@pytest.mark.parametrize("name", SC.NAMES["expand"])
def test_expand_columns(csx, name):
    Ap = SC.inputs(name)["Ap"]
    n = len(Ap) - 1
    col, back = csx.prim_expand_columns(Ap)
    assert same_bits(col, np.repeat(np.arange(n, dtype=np.int32), np.diff(Ap))) and same_bits(back, Ap)


@pytest.mark.parametrize("name", SC.NAMES["boundaries"])
def test_boundaries(csx, name):
    d = SC.inputs(name)
    key, nkeys = d["key"], d["nkeys"]
    ptr, back = csx.prim_boundaries(key, nkeys, d["misalign"])
    ref = np.searchsorted(key, np.arange(nkeys + 1, dtype=np.uint32), "left").astype(np.int32)
    assert same_bits(ptr, ref) and same_bits(back, key)


@pytest.mark.parametrize("name", SC.NAMES["sort"])
def test_sort(csx, name):
    d, want = SC.inputs(name), SC.facts(name)
    key, a, v, xp, nkeys = d["key"], d.get("a"), d.get("v"), d.get("expand_ptr"), d.get("nkeys")
    with csx.option("sort.short_keys", d.get("short_keys", 1)):
        r = csx.prim_sort(key, a, v, d["key_limit"], d["want_key"], xp, nkeys, d.get("misalign", 0))
    info = csx.prim_sort_info()
    for field in csx.SORT_INFO:
        assert info[field] == want[field], (name, field, info, want)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    if d["want_key"]:
        assert same_bits(r["out_key"], skey), name
    else:
        assert r["out_key"] is None
    if xp is not None:
        a = np.repeat(np.arange(len(xp) - 1, dtype=np.uint32), np.diff(xp))      # the column of each position
    if a is not None:
        assert same_bits(r["out_a"], a[order]), name
    if v is not None:
        assert same_bits(r["out_v"], v[order]), name                             # as bytes: -0.0, infinities and NaN payloads
    if nkeys is not None:
        ref = np.searchsorted(skey, np.arange(nkeys + 1, dtype=np.uint32), "left").astype(np.int32)
        assert same_bits(r["out_ptr"], ref), name
    # the inputs as the device holds them after the sort
    assert same_bits(r["key"], key)
    for got, src in ((r["a"], d.get("a")), (r["v"], v), (r["expand_ptr"], xp)):
        assert (got is None and src is None) or same_bits(got, src), name


def test_sort_info_is_host_state_of_the_last_sort(csx):
    """an empty sort resets it; the fields past `cap` are left alone"""
    csx.prim_sort(SC.inputs("sort_av_tile_p1")["key"], key_limit=SC.inputs("sort_av_tile_p1")["key_limit"])
    assert csx.prim_sort_info()["nblocks"] == 2
    csx.prim_sort(np.zeros(0, np.uint32), key_limit=7)
    assert csx.prim_sort_info() == SC.sort_model(0, 7, False, False, True)
    out = (csx.C.c_int64 * 4)(-1, -1, -1, -1)
    assert csx.load().csx_prim_sort_info(out, 2) == csx.OK and list(out) == [0, 0, -1, -1]


@pytest.mark.parametrize("values", [True, False], ids=["values", "pattern"])
def test_transpose_of_a_wrapped_matrix_whose_rows_are_not_16_byte_aligned(csx, values):
    """csx_csc_wrap takes the caller's row-index pointer as it is, and csx_transpose sorts it: one word past a 16-byte boundary
    the histogram of the first pass reads key by key.  Against the C oracle's transpose, bit for bit."""
    lib, C = csx.lib(), csx.C
    tile = SC.TILE
    m, n, nnz = 70001, 400, 3 * tile + 100
    rng = np.random.default_rng(20240917)
    cols = np.sort(rng.integers(n // 10, n - n // 20, nnz))
    Ap = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int32)
    rows = rng.integers(0, m, nnz).astype(np.int32)
    rows[::5] = rows[1::5][:len(rows[::5])]                 # duplicates: source order must survive
    vals = rng.standard_normal(nnz)
    Rp, Ri, Rx = CO.transpose(m, n, Ap, rows, vals)

    def upload_i(arr):
        h = csx.new_handle()
        csx.check(lib.csx_ivec_upload(csx.pi(arr), len(arr), h))
        return h

    def ptr(h):
        p, length = C.c_void_p(), C.c_int64()
        csx.check(lib.csx_vec_ptr(h, p, length))
        return p.value

    hp, hi, hx = upload_i(Ap), upload_i(np.concatenate([[-1], rows]).astype(np.int32)), csx.new_handle()
    csx.check(lib.csx_vec_upload(csx.pd(vals), nnz, hx))
    base = ptr(hi)
    assert base % 16 == 0
    hA, hT = csx.new_handle(), csx.new_handle()
    csx.check(lib.csx_csc_wrap(m, n, nnz, ptr(hp), base + 4, ptr(hx) if values else None, hA))
    csx.check(lib.csx_transpose(hA, 1 if values else 0, hT))
    info = csx.prim_sort_info()
    assert info["key_misalign"] == 1 and info["count"] == nnz and info["k16"] == (1 if values else 0)
    Tp, Ti, Tx = np.empty(m + 1, np.int32), np.empty(nnz, np.int32), np.empty(nnz, np.float64)
    csx.check(lib.csx_csc_download(hT, csx.pi(Tp), csx.pi(Ti), csx.pd(Tx) if values else None))
    for h in (hT, hA, hp, hi, hx):
        csx.free(h)
    assert same_bits(Tp, Rp.astype(np.int32)) and same_bits(Ti, Ri.astype(np.int32))
    assert not values or Tx.tobytes() == np.asarray(Rx, np.float64).tobytes()
