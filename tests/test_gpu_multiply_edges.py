"""cs_multiply on the device at every accumulator bin, table and staging edge: the cases of tests/spgemm_cases.py.  For each:
  * C.p, C.i, nzmax and len(C.i) are the plain-C oracle's exactly (first-touch order);
  * csx_spgemm_info says what ran: it equals the Python model field for field (bins, path, grids, every launch counter);
  * with dyadic values (every product and partial sum exact) C.x is the oracle's byte for byte in the default mode, with the
    one-pass path off, and in the reference's order;
  * with mixed values every entry satisfies |x - exact| <= gamma_c sum|a b| + ulp(exact) / 2, gamma_c = c u / (1 - c u) for the c
    products behind it: the textbook bound of c rounded products and c - 1 rounded additions in any order, against the exact sum
    in rational arithmetic -- an entry that lost a product or took one twice does not pass it;
  * with mixed values in the reference's order ("spgemm.ordered") C.x is the oracle's byte for byte, twice;
  * pattern-only runs (A.x, B.x or both removed) give the same p and i and no x.
tests/test_spgemm_cases_cpu.py shows without a device that the cases sit where they say and launch every counted site."""
import functools

import numpy as np
import pytest

import c_oracle as CO
import csparse_oracle as O
import spgemm_cases as SC
from test_gpu_parity import _host_cs, cs  # noqa: F401

pytestmark = pytest.mark.gpu
NAMES = SC.names()
RATIOS = {}                              # family -> the largest |x - exact| / (gamma_c sum|a b|) seen (tools/measure_spgemm_edges.py)


@pytest.fixture(scope="module")
def cus(cs):
    import _csx
    return _csx.device_info()[1]


@functools.lru_cache(maxsize=4)
def reference(cus, name, kind):
    """(case, Ax, Bx, Cp, Ci, Cx) of the plain-C oracle; shared by the tests of a case and left unchanged"""
    case = SC.by_name(cus, name)
    Ax, Bx = SC.values_for(case, kind)
    Cp, Ci, Cx = CO.multiply(case.m, case.k, case.n, case.Ap, case.Ai, Ax, case.Bp, case.Bi, Bx)
    for a in (Ax, Bx, Cp, Ci, Cx):
        a.setflags(write=False)
    return case, Ax, Bx, Cp, Ci, Cx


def operands(cs, case, Ax, Bx):
    return _host_cs(cs, case.m, case.k, case.Ap, case.Ai, Ax), _host_cs(cs, case.k, case.n, case.Bp, case.Bi, Bx)


def same_pattern(C, Cp, Ci):
    nnz = int(Cp[-1])
    assert C.p == Cp.tolist()
    assert C.i[:nnz] == Ci.tolist()
    assert C.nzmax == nnz and len(C.i) == nnz


def same_info(case, cus, values, **how):
    import _csx
    want = SC.model(case.m, case.k, case.n, case.Ap, case.Bp, case.Bi, values, cus, **how)
    got = _csx.spgemm_info()
    for key in want:
        assert got[key] == want[key], (case.name, how, key)
    assert got == want


def modes(case):
    return [1, 0] if case.two_pass_too else [1]


@pytest.mark.parametrize("name", NAMES)
def test_dyadic_values_are_exact_in_every_mode(cs, cus, name):
    import _csx
    case, Ax, Bx, Cp, Ci, Cx = reference(cus, name, "dyadic")
    A, B = operands(cs, case, Ax, Bx)
    for one_pass in modes(case):
        with _csx.option("spgemm.one_pass", one_pass):
            C = cs.cs_multiply(A, B)
        same_info(case, cus, True, one_pass=bool(one_pass))
        same_pattern(C, Cp, Ci)
        assert np.asarray(C.x).tobytes() == Cx.tobytes(), (name, one_pass)
    with _csx.option("spgemm.ordered", 1):
        C = cs.cs_multiply(A, B)
    same_info(case, cus, True, ordered=True, Cp=Cp)
    same_pattern(C, Cp, Ci)
    assert np.asarray(C.x).tobytes() == Cx.tobytes(), name


def check_bound(case, Ax, Bx, x):
    """every entry within gamma_c sum|a b| + ulp(exact) / 2 of the exact sum; returns the largest |x - exact| / (gamma_c sum|a b|)"""
    sums, mags, terms = SC.exact_entries(case, Ax, Bx)
    assert len(x) == len(sums)
    worst = 0.0
    for e, (xe, s) in enumerate(zip(x, sums)):
        if xe == float(s):                   # the correctly rounded exact sum: within ulp / 2 by definition
            continue
        ok, ratio = SC.within_bound(xe, s, mags[e], terms[e])
        assert ok, (case.name, e, terms[e], xe, float(s), ratio)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_mixed_values_are_within_the_bound_of_their_products(cs, cus, name):
    import _csx
    case, Ax, Bx, Cp, Ci, _ = reference(cus, name, "mixed")
    A, B = operands(cs, case, Ax, Bx)
    C = cs.cs_multiply(A, B)
    same_info(case, cus, True)
    same_pattern(C, Cp, Ci)
    RATIOS[case.family] = max(RATIOS.get(case.family, 0.0), check_bound(case, Ax, Bx, C.x))
    assert _csx.spgemm_info()["ordered"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_mixed_values_in_the_reference_order_are_bit_identical(cs, cus, name):
    import _csx
    case, Ax, Bx, Cp, Ci, Cx = reference(cus, name, "mixed")
    A, B = operands(cs, case, Ax, Bx)
    with _csx.option("spgemm.ordered", 1):
        C = cs.cs_multiply(A, B)
        same_info(case, cus, True, ordered=True, Cp=Cp)
        C2 = cs.cs_multiply(A, B)
    same_pattern(C, Cp, Ci)
    assert np.asarray(C.x).tobytes() == Cx.tobytes(), name
    assert C2.x == C.x and C2.i == C.i


@pytest.mark.parametrize("name", NAMES)
def test_pattern_only(cs, cus, name):
    import _csx
    case, Ax, Bx, Cp, Ci, _ = reference(cus, name, "dyadic")
    for drop_a, drop_b, one_pass in [(1, 0, 1), (0, 1, 1), (1, 1, 1)] + ([(1, 1, 0)] if case.two_pass_too else []):
        A, B = operands(cs, case, Ax, Bx)
        if drop_a:
            A.x = None
        if drop_b:
            B.x = None
        with _csx.option("spgemm.one_pass", one_pass), _csx.option("spgemm.ordered", 1 - one_pass):   # (no values: no ordered pass)
            C = cs.cs_multiply(A, B)
        same_info(case, cus, False, one_pass=bool(one_pass))
        assert C.x is None
        same_pattern(C, Cp, Ci)


def _lists(cs_mod, m, n, cols, values):
    A = cs_mod.cs_spalloc(m, n, sum(len(c) for c in cols), values, False)
    A.p = [0] + np.cumsum([len(c) for c in cols]).astype(int).tolist()
    flat = [r for c in cols for r in c]
    A.i = flat + [0] * (A.nzmax - len(flat))
    if values:
        A.x = [0.5 + 0.25 * t for t in range(len(flat))] + [0.0] * (A.nzmax - len(flat))
    return A


@pytest.mark.parametrize("shape", SC.degenerate_shapes(), ids=lambda s: s[0])
@pytest.mark.parametrize("values", [True, False])
def test_empty_shapes(cs, cus, shape, values):
    import _csx
    _, m, k, n, acols, bcols = shape
    for ordered in (0, 1):
        with _csx.option("spgemm.ordered", ordered):
            C = cs.cs_multiply(_lists(cs, m, k, acols, values), _lists(cs, k, n, bcols, values))
        R = O.cs_multiply(_lists(O, m, k, acols, values), _lists(O, k, n, bcols, values))
        assert (C.m, C.n, C.nzmax, C.p, list(C.i), C.x) == (R.m, R.n, R.nzmax, R.p, list(R.i), R.x)
        info = _csx.spgemm_info()
        assert info["launches"] == {} and info["bins"] == (0,) * SC.NBINS and info["ordered"] == 0 and info["cus"] == cus
    assert cs.cs_multiply(_lists(cs, 5, 3, [[0], [1], []], values), _lists(cs, 4, 2, [[0], [1]], values)) is None


def test_a_column_of_two_to_the_32_products_is_refused_and_the_next_product_is_right(cs, cus):
    import _csx
    big = SC.too_big_case()
    Ax, Bx = SC.values_for(big, "dyadic")
    A, B = operands(cs, big, Ax, Bx)
    with pytest.raises(ValueError):
        cs.cs_multiply(A, B)
    assert b"2^32 products" in _csx.lib().csx_last_error()
    same_info(big, cus, True)                                    # nothing past k_sg_products was launched
    assert _csx.spgemm_info()["launches"] == {"products": 1}
    case, Ax, Bx, Cp, Ci, Cx = reference(cus, "h1-a-lengths", "dyadic")
    C = cs.cs_multiply(*operands(cs, case, Ax, Bx))
    same_info(case, cus, True)
    same_pattern(C, Cp, Ci)
    assert np.asarray(C.x).tobytes() == Cx.tobytes()


def test_the_info_call_writes_no_more_than_it_is_given(cs, cus):
    import _csx
    case, Ax, Bx, _, _, _ = reference(cus, "narrow-cut-length", "dyadic")
    cs.cs_multiply(*operands(cs, case, Ax, Bx))
    lib, C = _csx.lib(), _csx.C
    out, count = (C.c_int64 * 40)(*([-7] * 40)), C.c_int32(0)
    assert lib.csx_spgemm_info(out, 33, count) == _csx.OK and count.value == SC.LIM["INFO_FIELDS"]
    assert list(out)[33:] == [-7] * 7 and sum(list(out)[:32]) > 0
