"""The add plan without a GPU (include/csx.h, "add plan"): the pure-Python restatement of its definition
against the oracle's cs_add (chained for more than two operands), the library's host rule against the restatement, the edges,
the signs of zero, that a fused multiply-add would show, and the declarations.  Every comparison of values is byte equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import add_plan_oracle as AO
import csparse_oracle as PO
from conftest import ROOT

GOLDEN = [(name, k) for name in AO.GOLDEN for k in (2, 3)]
CASES = AO.synthetic_cases() + AO.edge_cases() + [c[:3] for c in AO.zero_cases()]
ENTRY_POINTS = {"csx_add_plan_host": 10, "csx_add_fold_host": 8, "csx_add_plan": 3, "csx_add_plan_matrix": 4,
                "csx_add_plan_run": 4, "csx_add_plan_info": 2}


def pointers(arrays, ctype):
    return (C.POINTER(ctype) * len(arrays))(*(a.ctypes.data_as(C.POINTER(ctype)) for a in arrays))


def host_plan(ops, k=None, m=None, n=None):
    """(status, Cp, Ci, sp, src) of the library's host rule"""
    import _csx
    lib = _csx.load()
    k = len(ops) if k is None else k
    m, n = ops[0].m if m is None else m, ops[0].n if n is None else n
    ps = [_csx.i32(A.p) for A in ops]
    idx = [_csx.i32(list(A.i[:A.p[A.n]]) + [0]) for A in ops]
    terms = sum(max(int(A.p[A.n]), 0) for A in ops)
    Cp, Ci = np.full(n + 1, -7, np.int32), np.full(terms + 1, -7, np.int32)
    sp, src = np.full(terms + 2, -7, np.int32), np.full(terms + 1, -7, np.int32)
    nnz = C.c_int32(-1)
    st = lib.csx_add_plan_host(m, n, k, pointers(ps, C.c_int32), pointers(idx, C.c_int32), _csx.pi(Cp), _csx.pi(Ci), _csx.pi(sp),
                               _csx.pi(src), nnz)
    if st != _csx.OK:
        return st, None, None, None, None
    assert Ci[terms] == -7 and sp[terms + 1] == -7 and src[terms] == -7          # nothing written past the sizes promised
    return st, Cp.tolist(), Ci[:nnz.value].tolist(), sp[:nnz.value + 1].tolist(), src[:terms].tolist()


def host_fold(sp, src, off, coef, xs):
    import _csx
    nnz, k = len(sp) - 1, len(xs)
    out = np.full(max(nnz, 1), np.nan)
    xa = [_csx.f64(list(x) + [0.0]) for x in xs]
    coef = _csx.f64([float(c) for c in coef])
    st = _csx.load().csx_add_fold_host(nnz, k, _csx.pi(_csx.i32(sp)), _csx.pi(_csx.i32(src + [0])), _csx.pi(_csx.i32(off)),
                                       _csx.pd(coef), pointers(xa, C.c_double), _csx.pd(out))
    assert st == _csx.OK
    return out[:nnz]


def check_plan_shape(ops, p, i, sp, src, off):
    """what the definition says about the lists, whatever the values"""
    n, nnz = ops[0].n, p[-1]
    assert len(i) == nnz and len(sp) == nnz + 1 and sp[0] == 0 and len(src) == sp[nnz] == off[-1]
    assert all(sp[s] < sp[s + 1] for s in range(nnz))                           # every stored slot has a term
    assert sorted(src) == list(range(off[-1]))                                   # every entry of every operand exactly once
    owner = [r for r in range(len(ops)) for _ in range(off[r + 1] - off[r])]
    for j in range(n):
        assert len(set(i[p[j]:p[j + 1]])) == p[j + 1] - p[j]                     # a row once per column
        for s in range(p[j], p[j + 1]):
            terms = src[sp[s]:sp[s + 1]]
            assert terms == sorted(terms)                                        # operand order, then stored position
            for g in terms:
                A, e = ops[owner[g]], g - off[owner[g]]
                assert A.p[j] <= e < A.p[j + 1] and A.i[e] == i[s]


def check_case(ops, coef, shape=True):
    """restatement == chained oracle, host rule == restatement; returns the restatement and the expected bytes"""
    import _csx
    ref = AO.plan(ops)
    p, i, sp, src, off = ref
    Cref = AO.chain(PO, ops, coef)
    nnz = p[-1]
    assert p == Cref.p and i == Cref.i[:nnz]
    want = AO.as_bytes(Cref.x[:nnz])
    if shape:
        check_plan_shape(ops, p, i, sp, src, off)
    xs = [AO.values(A) for A in ops]
    assert AO.as_bytes(AO.fold(sp, src, off, coef, xs)) == want
    st, Cp, Ci, hsp, hsrc = host_plan(ops)
    assert st == _csx.OK and (Cp, Ci, hsp, hsrc) == (p, i, sp, src)
    assert host_fold(hsp, hsrc, off, coef, xs).tobytes() == want
    return ref, want


@pytest.mark.parametrize("name,k", GOLDEN, ids=["%s-k%d" % g for g in GOLDEN])
def test_restatement_and_host_rule_on_golden(name, k):
    ops, coef, Cref = AO.golden_case(name, k)
    (p, i, sp, src, off), want = check_case(ops, coef, shape=name != "bcsstk16")
    assert p == AO.golden_plan(name, k)[0]
    # nzmax as the chain leaves it: cs_add does not trim
    A = ops[0]
    assert Cref.nzmax == (2 * A.p[A.n] if k == 2 else AO.chain(PO, ops[:2], coef[:2]).p[A.n] + A.p[A.n])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_restatement_and_host_rule_on_synthetic_and_edges(case):
    label, ops, coef = case
    (p, i, sp, src, off), want = check_case(ops, coef)
    nnz = p[-1]
    if label in ("m0", "n0", "all_empty"):
        assert nnz == 0 and sp == [0] and src == []
    if label.startswith("random"):
        # duplicates inside a column of an operand, and the comparison can tell a wrong order from the right one
        assert any(len(set(A.i[A.p[j]:A.p[j + 1]])) < A.p[j + 1] - A.p[j] for A in ops for j in range(A.n))
        assert AO.as_bytes(AO.fold(sp, src, off, coef, [AO.values(A) for A in ops], reverse=True)) != want
    if label.startswith("identical"):
        k = len(ops)
        assert src == [off[r] + s for s in range(nnz) for r in range(k)]         # the aligned class
    if label == "reordered":
        assert sorted(i) == sorted(ops[0].i[:nnz]) and src != [off[r] + s for s in range(nnz) for r in range(2)]
    if label == "disjoint":
        assert nnz == off[-1] and all(sp[s + 1] - sp[s] == 1 for s in range(nnz))


@pytest.mark.parametrize("thr", [64, 2])
def test_class_boundary_case_and_fused_multiply_add(thr):
    """the GPU test's case: the slot lengths it was built for, and at least one slot whose defined bytes are not the bytes a
    fused multiply-add gives (computed exactly, one final rounding) -- so byte equality on the GPU means "never fused" """
    ops, coef, lens = AO.boundary_case(thr, 5)
    (p, i, sp, src, off), want = check_case(ops, coef)
    assert [sp[s + 1] - sp[s] for s in range(p[-1])] == lens
    assert sorted(lens) == sorted([thr - 1, thr, thr + 1, 63, 64, 65, 127, 128, 129])
    owner = [r for r in range(8) for _ in range(off[r + 1] - off[r])]
    for s in range(p[-1]):
        if lens[s] >= 8:
            assert {owner[g] for g in src[sp[s]:sp[s + 1]]} == set(range(8))     # every branch of the operand selection
    xs = [AO.values(A) for A in ops]
    fused = np.asarray(AO.fold(sp, src, off, coef, xs, fused=True))
    plain = np.frombuffer(want, np.float64)
    differ = [s for s in range(p[-1]) if fused[s].tobytes() != plain[s].tobytes()]
    assert len(differ) >= 1
    assert AO.as_bytes(AO.fold(sp, src, off, coef, xs, reverse=True)) != want


def test_fold_is_not_contracted():
    """acc + c * x as one fused multiply-add rounds differently on these numbers; the host fold must not"""
    import csparse_oracle as PO
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    ops = [AO.csc(PO, 1, 1, [0, 1], [0], [-1.0]), AO.csc(PO, 1, 1, [0, 1], [0], [a])]
    p, i, sp, src, off = AO.plan(ops)
    plain = AO.fold(sp, src, off, [1.0, b], [[-1.0], [a]])
    assert plain == [0.0] and AO.fold(sp, src, off, [1.0, b], [[-1.0], [a]], fused=True) == [-2.0 ** -60]
    assert host_fold(sp, src, off, [1.0, b], [[-1.0], [a]]).tobytes() == AO.as_bytes(plain)
    assert AO.as_bytes(PO.cs_add(ops[0], ops[1], 1.0, b).x[:1]) == AO.as_bytes(plain)


@pytest.mark.parametrize("case", AO.zero_cases(), ids=lambda c: c[0])
def test_signed_zeros(case):
    label, ops, coef, expected = case
    (p, i, sp, src, off), want = check_case(ops, coef)
    assert want == AO.as_bytes(expected)
    if label == "all_negzero":
        assert AO.as_bytes([0.0 + -0.0 + -0.0 + -0.0]) != AO.as_bytes([-0.0])     # why the first term is assigned


def test_operand_counts_and_bad_input_are_refused():
    import _csx
    rng = np.random.default_rng(5)
    A, B = AO.random_csc(rng, 4, 3, [2, 1, 2]), AO.random_csc(rng, 4, 3, [0, 3, 1])
    assert host_plan([A, B])[0] == _csx.OK and host_plan([A] * 8)[0] == _csx.OK
    assert host_plan([A], k=1)[0] == _csx.EINVAL
    assert host_plan([A] * 9, k=9)[0] == _csx.EINVAL
    for count in (1, 9):
        with pytest.raises(ValueError):
            AO.plan([A] * count)
    for which, index, bad in ((0, 1, 4), (0, 0, -1), (1, 3, 4), (1, 0, -1)):
        ops = [AO.csc(PO, 4, 3, A.p, A.i, A.x), AO.csc(PO, 4, 3, B.p, B.i, B.x)]
        ops[which].i[index] = bad
        assert host_plan(ops)[0] == _csx.EINVAL
        with pytest.raises(IndexError):
            AO.plan(ops)
    for bad_p in ([0, 2, 1, 5], [1, 2, 3, 5]):                                   # pointers that decrease, that do not start at 0
        A2 = AO.csc(PO, 4, 3, A.p, A.i, A.x)
        A2.p = bad_p
        assert host_plan([A2, B])[0] == _csx.EINVAL and host_plan([B, A2])[0] == _csx.EINVAL
        with pytest.raises(IndexError):
            AO.plan([A2, B])
    assert host_plan([A, B], m=3)[0] == _csx.EINVAL                               # a row index of A reaches 3
    assert host_plan([A, B], m=-1)[0] == _csx.EINVAL and host_plan([A, B], n=-1)[0] == _csx.EINVAL


def test_python_refusals_without_a_device():
    """decided before any device work: what cs_add refuses gives no plan, more than 8 operands is a ValueError"""
    import csparse as cs
    rng = np.random.default_rng(6)
    Ao = AO.random_csc(rng, 4, 3, [2, 1, 2])
    A = AO.csc(cs, 4, 3, Ao.p, Ao.i, Ao.x)
    W = AO.csc(cs, 3, 4, [0, 0, 0, 0, 0], [], [])
    T = cs.cs_spalloc(4, 3, 1, True, True)
    assert cs.add_plan(A, W) is None and cs.cs_add(A, W, 1, 1) is None
    assert cs.add_plan(A, A, W) is None
    assert cs.add_plan(A, T) is None and cs.add_plan(T, A) is None and cs.add_plan(None, A) is None and cs.add_plan(A, None) is None
    with pytest.raises(ValueError):
        cs.add_plan(*([A] * 9))


def test_header_declares_and_csx_binds_the_entry_points():
    import _csx
    text = open(os.path.join(ROOT, "include", "csx.h")).read()
    assert "add plan" in text and "NEVER fused" in text and "first-touch order through A_0(:,j)" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _csx.load()
    for name, arity in ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity == len(_csx._PROTOS[name]), name
        assert hasattr(lib, name), name
