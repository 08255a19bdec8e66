"""The multiply plan without a GPU (include/csx.h, "multiply plan"): the pure-Python restatement of its
definition against the oracle's cs_multiply, the library's host rule against the restatement, the scaled rule against
cs_multiply(A, B2), and the declarations.  Every comparison of values is byte equality."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import csparse_oracle as PO
import multiply_plan_oracle as MO
from conftest import ROOT

GOLDEN = [(name, tr) for name in MO.GOLDEN for tr in (False, True)]
GOLDEN_IDS = ["%s-%s" % (name, "ATA" if tr else "AAT") for name, tr in GOLDEN]
PAIRS = MO.synthetic_pairs() + MO.wide_pairs() + MO.edge_pairs()
ENTRY_POINTS = {"csx_multiply_plan_count": 9, "csx_multiply_plan_host": 11, "csx_multiply_fold_host": 6, "csx_multiply_plan": 3,
                "csx_multiply_plan_matrix": 5, "csx_multiply_plan_run": 5, "csx_multiply_plan_info": 2}


def host_plan(A, B):
    """(status of count, status of host, Cp, Ci, sp, pair) of the library's host rule"""
    import _csx
    lib = _csx.load()
    ap, ai, _ = MO.arrays(A)
    bp, bi, _ = MO.arrays(B)
    nnz, products = C.c_int64(-1), C.c_int64(-1)
    args = (A.m, A.n, B.n, _csx.pi(ap), _csx.pi(ai), _csx.pi(bp), _csx.pi(bi))
    st = lib.csx_multiply_plan_count(*args, nnz, products)
    if st != _csx.OK:
        return st, None, None, None, None, None
    Cp, Ci = np.full(B.n + 1, -7, np.int32), np.full(max(nnz.value, 1), -7, np.int32)
    sp, pair = np.full(nnz.value + 1, -7, np.int32), np.full(max(2 * products.value, 1), -7, np.int32)
    st2 = lib.csx_multiply_plan_host(*args, _csx.pi(Cp), _csx.pi(Ci), _csx.pi(sp), _csx.pi(pair))
    return st, st2, Cp, Ci[:nnz.value], sp, pair[:2 * products.value]


def host_fold(sp, pair, ax, bx):
    import _csx
    nnz = len(sp) - 1
    out = np.full(max(nnz, 1), np.nan)
    sp, pair, ax, bx = _csx.i32(sp), _csx.i32(pair), _csx.f64(ax), _csx.f64(bx)
    assert _csx.load().csx_multiply_fold_host(nnz, _csx.pi(sp), _csx.pi(pair), _csx.pd(ax), _csx.pd(bx), _csx.pd(out)) == _csx.OK
    return out[:nnz]


def check_plan_shape(A, B, p, i, sp, pair):
    """what the definition says about the lists, whatever the values"""
    nnz = p[B.n]
    assert len(i) == nnz and len(sp) == nnz + 1 and sp[0] == 0 and len(pair) == 2 * sp[nnz]
    assert all(sp[s] < sp[s + 1] for s in range(nnz))                       # every stored slot has a product
    for j in range(B.n):
        assert len(set(i[p[j]:p[j + 1]])) == p[j + 1] - p[j]                # a row once per column
        for s in range(p[j], p[j + 1]):
            prods = [(pair[2 * t + 1], pair[2 * t]) for t in range(sp[s], sp[s + 1])]
            assert prods == sorted(prods) and len(set(prods)) == len(prods)  # ib ascending, then ia ascending
            assert all(B.p[j] <= ib < B.p[j + 1] and A.p[B.i[ib]] <= ia < A.p[B.i[ib] + 1] and A.i[ia] == i[s]
                       for ib, ia in prods)
    assert sp[nnz] == sum(A.p[B.i[t] + 1] - A.p[B.i[t]] for t in range(B.p[B.n]))   # every product once


def check_host_abi(A, B, ref):
    import _csx
    p, i, sp, pair = ref
    st, st2, Cp, Ci, hsp, hpair = host_plan(A, B)
    assert (st, st2) == (_csx.OK, _csx.OK)
    assert Cp.tolist() == p and Ci.tolist() == i and hsp.tolist() == sp and np.array_equal(hpair, np.asarray(pair, np.int32))
    return hsp, hpair


@pytest.mark.parametrize("name,transposed", GOLDEN, ids=GOLDEN_IDS)
def test_restatement_and_host_rule_on_golden(name, transposed, meta):
    A, B = MO.golden_pair(name, transposed)
    ref = MO.golden_plan(name, transposed)
    p, i, sp, pair = ref
    Cp, Ci, Cx = MO.golden_product(name, transposed)
    assert p == Cp and i == Ci
    small = name in MO.SMALL
    if small:
        check_plan_shape(A, B, p, i, sp, pair)
    hsp, hpair = check_host_abi(A, B, ref)
    nnz = p[B.n]
    want = np.asarray(Cx, np.float64).tobytes()
    if small or not transposed:
        assert MO.as_bytes(MO.fold(sp, pair, A.x[:A.p[A.n]], B.x[:B.p[B.n]])) == want
    assert host_fold(hsp, hpair, A.x[:A.p[A.n]], B.x[:B.p[B.n]]).tobytes() == want
    if not transposed:
        mm = meta[name]["AAT"]
        assert (mm["m"], mm["n"], mm["nnz"]) == (A.m, B.n, nnz)
        assert hashlib.sha256(want).hexdigest() == mm["sha_x"]
        assert hashlib.sha256(np.asarray(p, np.int64).tobytes()).hexdigest() == mm["sha_p"]
        assert hashlib.sha256(np.asarray(i, np.int64).tobytes()).hexdigest() == mm["sha_i"]


@pytest.mark.parametrize("case", PAIRS, ids=lambda c: c[0])
def test_restatement_and_host_rule_on_synthetic_wide_and_edges(case):
    label, A, B = case
    ref = MO.plan(A, B)
    p, i, sp, pair = ref
    Cref = PO.cs_multiply(A, B)
    nnz = p[B.n]
    assert p == Cref.p and i == Cref.i[:nnz] and len(Cref.x) == nnz
    check_plan_shape(A, B, p, i, sp, pair)
    want = MO.as_bytes(Cref.x)
    right = MO.fold(sp, pair, A.x, B.x)
    assert MO.as_bytes(right) == want
    hsp, hpair = check_host_abi(A, B, ref)
    assert host_fold(hsp, hpair, A.x, B.x).tobytes() == want
    if label.startswith("wide"):
        # the comparison can tell the two plausible wrong kernels from the right one
        assert max(sp[s + 1] - sp[s] for s in range(nnz)) >= 8
        assert MO.as_bytes(MO.fold(sp, pair, A.x, B.x, reverse=True)) != want
        assert MO.as_bytes(MO.fold(sp, pair, A.x, B.x, fused=True)) != want
    if label == "negzero":
        assert want == MO.as_bytes([-0.0, 0.0])
        assert MO.as_bytes([0.0 + -0.0 + -0.0]) != MO.as_bytes([-0.0])      # why the first term is assigned
    if label in ("k0", "n0", "m0", "products0"):
        assert nnz == 0 and sp == [0] and pair == []


@pytest.mark.parametrize("case", MO.synthetic_pairs() + MO.wide_pairs(), ids=lambda c: c[0])
def test_scaled_rule_is_the_product_with_b2(case):
    label, A, B = case
    rng = np.random.default_rng(len(label) + A.n)
    d = MO.wide(rng, A.n)
    p, i, sp, pair = MO.plan(A, B)
    B2 = MO.scaled(PO, B, d)
    Cref = PO.cs_multiply(A, B2)
    assert p == Cref.p and i == Cref.i[:p[B.n]]
    got = MO.fold(sp, pair, A.x, B.x, d=d, bi=B.i)
    assert MO.as_bytes(got) == MO.as_bytes(Cref.x)
    assert host_fold(sp, pair, A.x[:A.p[A.n]], B2.x[:B.p[B.n]]).tobytes() == MO.as_bytes(Cref.x)
    ones = MO.fold(sp, pair, A.x, B.x, d=[1.0] * A.n, bi=B.i)
    assert MO.as_bytes(ones) == MO.as_bytes(MO.fold(sp, pair, A.x, B.x))


def test_errors():
    import _csx
    import csparse as cs
    rng = np.random.default_rng(5)
    A, B = MO.random_csc(rng, 4, 3, [2, 1, 2]), MO.random_csc(rng, 3, 2, [2, 2])
    assert host_plan(A, B)[:2] == (_csx.OK, _csx.OK)
    for which, index, bad in (("A", 1, 4), ("A", 0, -1), ("B", 3, 3), ("B", 0, -1)):
        A2, B2 = MO.csc(PO, 4, 3, A.p, A.i, A.x), MO.csc(PO, 3, 2, B.p, B.i, B.x)
        (A2 if which == "A" else B2).i[index] = bad
        assert host_plan(A2, B2)[0] == _csx.EINVAL
        with pytest.raises(IndexError):
            MO.plan(A2, B2)
    A2 = MO.csc(PO, 4, 3, [0, 2, 1, 5], A.i, A.x)                           # pointers that decrease
    assert host_plan(A2, B)[0] == _csx.EINVAL
    # A.n != B.m: no plan, as cs_multiply gives no product (decided before any device work)
    with pytest.raises(ValueError):
        MO.plan(A, A)
    assert PO.cs_multiply(A, A) is None
    assert cs.multiply_plan(MO.csc(cs, 4, 3, A.p, A.i, A.x), MO.csc(cs, 4, 3, A.p, A.i, A.x)) is None
    T = cs.cs_spalloc(3, 3, 1, True, True)
    assert cs.multiply_plan(T, T) is None and cs.multiply_plan(None, T) is None


def test_fold_is_not_contracted():
    """acc + beta * a as one fused multiply-add rounds differently on these three numbers; the host fold must not"""
    a, b, c = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0
    sp, pair = [0, 2], [0, 0, 1, 1]
    ax, bx = [c, a], [1.0, b]
    plain = MO.fold(sp, pair, ax, bx)
    assert plain == [0.0] and MO.fold(sp, pair, ax, bx, fused=True) == [-2.0 ** -60]
    assert host_fold(sp, pair, ax, bx).tobytes() == MO.as_bytes(plain)


def test_header_declares_and_csx_binds_the_entry_points():
    import _csx
    text = open(os.path.join(ROOT, "include", "csx.h")).read()
    assert "multiply plan" in text and "NEVER fused" in text and "The first term is ASSIGNED" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _csx.load()
    for name, arity in ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity == len(_csx._PROTOS[name]), name
        assert hasattr(lib, name), name
