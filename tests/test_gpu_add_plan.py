"""add_plan on the device (include/csx.h "add plan"): the pattern is the oracle's exactly, every comparison of
values is byte equality against the oracle's cs_add (chained for more than two operands), at the smallest shapes where each
class of step (the aligned stream, one lane per slot, one wave per long slot) can go wrong.  tests/test_add_plan_cpu.py shows
that the same cases tell a fused multiply-add and a reversed order from the definition."""
import numpy as np
import pytest

import add_plan_oracle as AO
import csparse_oracle as PO

pytestmark = pytest.mark.gpu

GOLDEN = [(name, k) for name in AO.GOLDEN if name != "bcsstk16" for k in (2, 3)]   # (the CPU file has the large one)


def cs():
    import csparse
    return csparse


def threshold():
    import _csx
    v = _csx.C.c_int(0)
    _csx.check(_csx.lib().csx_get_option(b"add.long", v), "csx_get_option")
    return v.value


def product_cs(Ao, values=True):
    """the product module's copy of an oracle matrix"""
    return AO.csc(cs(), Ao.m, Ao.n, Ao.p, Ao.i, Ao.x if values else None)


def product_ops(ops):
    """copies of the operands, the same object wherever the oracle's list names the same object"""
    made = {}
    return [made.setdefault(id(A), product_cs(A)) for A in ops]


def check_plan(ops, coef, aligned=None):
    """plan, info, .add and .matrix against the restatement and the oracle's chain; returns (P, restatement, expected bytes)"""
    c = cs()
    ref = AO.plan(ops)
    p, i, sp, src, off = ref
    nnz, k = p[-1], len(ops)
    Cref = AO.chain(PO, ops, coef)
    assert p == Cref.p and i == Cref.i[:nnz]
    want = AO.as_bytes(Cref.x[:nnz])
    P = c.add_plan(*product_ops(ops), coef=coef)
    assert (P.m, P.n, P.k, P.nnz, P.terms) == (ops[0].m, ops[0].n, k, nnz, off[-1])
    info = P.info()
    lens = [sp[s + 1] - sp[s] for s in range(nnz)]
    assert (info["k"], info["m"], info["n"], info["nnz"], info["terms"]) == (k, ops[0].m, ops[0].n, nnz, off[-1])
    assert info["max_terms"] == max(lens, default=0) and info["build_us"] >= 0
    is_aligned = src == [off[r] + s for s in range(nnz) for r in range(k)]
    assert info["aligned"] == int(is_aligned)
    if aligned is not None:
        assert is_aligned == aligned
    assert info["long_slots"] == (0 if is_aligned else sum(1 for v in lens if v > threshold()))
    assert info["nzmax"] == (Cref.nzmax if off[-1] else 0)
    got = P.add()
    assert len(got) == nnz and got.numpy().tobytes() == want
    assert P.info()["kernel_us"] >= 0
    M = P.matrix
    assert M is P.matrix and (M.m, M.n, M.nz, M.nzmax) == (Cref.m, Cref.n, -1, Cref.nzmax)
    assert M.p == p and M.i[:nnz] == i and len(M.i) == len(Cref.i)
    assert AO.as_bytes(M.x[:nnz]) == want and len(M.x) == len(Cref.x)
    return P, ref, want


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "general"])
@pytest.mark.parametrize("nnz", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_slot_counts_at_wave_and_workgroup_edges(nnz, aligned):
    """identical patterns take the aligned class (two slots per lane, an odd last slot); one more entry in the first column of
    one operand forces the fold"""
    ops, coef = AO.edge_count_case(nnz, aligned, nnz)
    P, (p, i, sp, src, off), want = check_plan(ops, coef, aligned=aligned)
    assert P.nnz == nnz and P.terms == len(ops) * nnz + (0 if aligned else 1)
    assert P.info()["max_terms"] == len(ops) + (0 if aligned else 1)


@pytest.mark.parametrize("long_option", [None, 2])
def test_slot_lengths_at_the_class_boundary(long_option):
    """slots of thr - 1, thr, thr + 1, 63 .. 65, 127 .. 129 terms from all eight operands (duplicates inside every operand's
    column): one lane or one wave per slot, every branch of the operand selection"""
    import _csx

    def run():
        thr = threshold()
        ops, coef, lens = AO.boundary_case(thr, 5)
        P, (p, i, sp, src, off), want = check_plan(ops, coef, aligned=False)
        assert [sp[s + 1] - sp[s] for s in range(P.nnz)] == lens
        info = P.info()
        assert info["terms"] == sum(lens) and info["max_terms"] == 129
        assert info["long_slots"] == sum(1 for v in lens if v > thr) >= 4
        xs = [AO.values(A) for A in ops]
        x = P.add().numpy().tobytes()
        # the comparison separates the right kernel from the two plausible wrong ones
        assert x != AO.as_bytes(AO.fold(sp, src, off, coef, xs, reverse=True))
        assert x != AO.as_bytes(AO.fold(sp, src, off, coef, xs, fused=True))

    if long_option is None:
        run()
    else:
        with _csx.option("add.long", long_option):
            assert threshold() == long_option
            run()


@pytest.mark.parametrize("case", AO.synthetic_cases() + AO.edge_cases(), ids=lambda c: c[0])
def test_operand_counts_duplicates_and_edges(case):
    """k = 2, 3, 8; duplicates inside columns; the same operand twice; disjoint, identical and reordered patterns; empty shapes"""
    label, ops, coef = case
    P, (p, i, sp, src, off), want = check_plan(ops, coef)
    if label.startswith("identical"):
        assert P.info()["aligned"] == 1
    if label in ("reordered", "twice_k3", "disjoint") or label.startswith("random"):
        assert P.info()["aligned"] == 0
    if label == "twice":
        assert P._ops[0] is P._ops[1] and P.info()["aligned"] == 0            # duplicates inside A's columns: A + A is a fold
    if label in ("m0", "n0", "all_empty"):
        assert P.nnz == 0 and len(P.add()) == 0 and P.update() is P.matrix and P.matrix.p == [0] * (ops[0].n + 1)


def test_nine_operands_and_a_plus_a():
    c = cs()
    rng = np.random.default_rng(31)
    Ao = AO.csc(PO, 6, 4, [0, 2, 2, 5, 6], [3, 0, 5, 1, 2, 4], AO.wide(rng, 6))
    A = product_cs(Ao)
    with pytest.raises(ValueError):
        c.add_plan(*([A] * 9))
    P = c.add_plan(A, A)
    assert P.info()["aligned"] == 1 and P.k == 2
    assert P.add().numpy().tobytes() == AO.as_bytes(PO.cs_add(Ao, Ao, 1.0, 1.0).x[:6])
    assert P.add((3, -2)).numpy().tobytes() == AO.as_bytes(PO.cs_add(Ao, Ao, 3, -2).x[:6])
    P8 = c.add_plan(*([A] * 8), coef=range(1, 9))
    assert P8.add().numpy().tobytes() == AO.as_bytes(AO.chain(PO, [Ao] * 8, list(range(1, 9))).x[:6])


@pytest.mark.parametrize("case", AO.zero_cases(), ids=lambda c: c[0])
def test_signed_zeros(case):
    label, ops, coef, expected = case
    P, ref, want = check_plan(ops, coef)
    assert want == AO.as_bytes(expected)


@pytest.mark.parametrize("name,k", GOLDEN, ids=["%s-k%d" % g for g in GOLDEN])
def test_golden_matrices(name, k):
    """A + A' and A + 2 A' - 0.5 A through .matrix, .add and .update"""
    c = cs()
    ops, coef, Cref = AO.golden_case(name, k)
    nnz = Cref.p[Cref.n]
    want = AO.as_bytes(Cref.x[:nnz])
    P = c.add_plan(*product_ops(ops), coef=coef)
    M = P.matrix
    assert (M.m, M.n, M.nz, M.nzmax, P.nnz) == (Cref.m, Cref.n, -1, Cref.nzmax, nnz)
    assert M.p == Cref.p and M.i == Cref.i and AO.as_bytes(M.x[:nnz]) == want
    first = P.add().numpy().tobytes()
    assert first == want and P.add().numpy().tobytes() == first
    coef2 = [0.75, -1.0 / 3.0, 1e-3][:k]
    want2 = AO.as_bytes(AO.chain(PO, ops, coef2).x[:nnz])
    assert want2 != want
    assert P.update(coef2) is M and AO.as_bytes(M.x[:nnz]) == want2
    assert P.update() is M and AO.as_bytes(M.x[:nnz]) == want
    assert P.info()["kernel_us"] >= 0


def override_case():
    label, ops, coef = AO.synthetic_cases()[1]                                 # random_k3
    assert label == "random_k3"
    return ops, coef


def test_value_overrides():
    c = cs()
    ops, coef = override_case()
    rng = np.random.default_rng(21)
    nz = [A.p[A.n] for A in ops]
    new = [AO.wide(rng, v) for v in nz]
    P = c.add_plan(*product_ops(ops), coef=coef)
    nnz = P.nnz

    def expect(which, cf):
        ops2 = [AO.with_values(A, new[r]) if r in which else A for r, A in enumerate(ops)]
        return AO.as_bytes(AO.chain(PO, ops2, cf).x[:nnz])

    dv = [c.dvec(v) for v in new]
    forms = ([v for v in new], [v.tolist() for v in new], dv)
    seen = set()
    for form in forms:
        for which in ((0,), (1,), (2,), (0, 2), (0, 1, 2)):
            given = [form[r] if r in which else None for r in range(3)]
            got = P.add(values=given).numpy().tobytes()
            assert got == expect(which, coef)
            seen.add(got)
    assert len(seen) == 5
    assert P.add((2, -3, 5), [dv[0], None, new[2].tolist()]).numpy().tobytes() == expect((0, 2), [2, -3, 5])   # integer coefficients
    assert P.add(np.array([2.0, -3.0, 5.0])).numpy().tobytes() == expect((), [2.0, -3.0, 5.0])
    # the inputs are unchanged afterwards, and so are the operands and the plan's own coefficients
    assert all(d.numpy().tobytes() == v.tobytes() for d, v in zip(dv, new))
    assert all(AO.as_bytes(Q.x[:v]) == AO.as_bytes(A.x[:v]) for Q, A, v in zip(P._ops, ops, nz))
    assert P.add().numpy().tobytes() == expect((), coef)


def test_coefficients_change_and_come_back():
    c = cs()
    K, M = AO.pencil()
    P = c.add_plan(product_cs(K), product_cs(M))
    assert P.info()["aligned"] == 1
    nnz = P.nnz
    s1, s2 = 0.1 + 1e-9, -2.5 / 3.0
    w1, w2 = (AO.as_bytes(PO.cs_add(K, M, 1.0, s).x[:nnz]) for s in (s1, s2))
    assert w1 != w2
    assert P.add((1, s1)).numpy().tobytes() == w1
    assert P.add((1, s2)).numpy().tobytes() == w2
    assert P.add((1, s1)).numpy().tobytes() == w1


def test_update_in_place():
    c = cs()
    ops, coef, C1 = AO.golden_case("west0067", 3)
    coef2 = [1.5, -0.25, 1.0 / 7.0]
    C2 = AO.chain(PO, ops, coef2)
    P = c.add_plan(*product_ops(ops), coef=coef)
    M = P.matrix
    nnz = P.nnz
    rng = np.random.default_rng(22)
    xs = rng.uniform(-1, 1, M.n).tolist()
    y, yo = [0.0] * M.m, [0.0] * M.m
    assert c.cs_gaxpy(M, xs, y) and PO.cs_gaxpy(C1, xs, yo)    # exact mode for lists: builds and caches the row-gather plan
    assert AO.as_bytes(y) == AO.as_bytes(yo)
    held = M.x                                                  # a host list read before the update
    assert AO.as_bytes(held) == AO.as_bytes(C1.x) and len(held) == C1.nzmax
    version = M._dev.version
    assert P.update(coef2) is M and P.matrix is M and M._dev.version == version + 1
    assert held is M.x and AO.as_bytes(held[:nnz]) == AO.as_bytes(C2.x[:nnz])
    y, yo = [0.0] * M.m, [0.0] * M.m
    assert c.cs_gaxpy(M, xs, y) and PO.cs_gaxpy(C2, xs, yo)
    assert AO.as_bytes(y) == AO.as_bytes(yo)                    # the cached SpMV plan held the old values: it was dropped
    assert c.cs_norm(M) == PO.cs_norm(C2)
    assert P.update() is M and AO.as_bytes(M.x[:nnz]) == AO.as_bytes(C1.x[:nnz]) and held is M.x


def test_pattern_only_operands():
    c = cs()
    ops, coef = override_case()
    want = AO.chain(PO, ops, coef)
    nnz = want.p[want.n]
    for has in ((False, True, True), (True, True, False), (False, False, False)):
        P = c.add_plan(*[product_cs(A, h) for A, h in zip(ops, has)], coef=coef)
        M = P.matrix
        assert M.x is None and M.p == want.p and M.i == want.i and M.nzmax == want.nzmax
        given = [None if h else AO.values(A) for A, h in zip(ops, has)]
        with pytest.raises(ValueError):
            P.add()
        with pytest.raises(ValueError):
            P.update()
        missing = [r for r, h in enumerate(has) if not h]
        if len(missing) > 1:
            with pytest.raises(ValueError):
                P.add(values=[v if r != missing[0] else None for r, v in enumerate(given)])
        assert P.add(values=given).numpy().tobytes() == AO.as_bytes(want.x[:nnz])
        assert P.matrix.x is None
        assert P.update(values=given) is M and AO.as_bytes(M.x[:nnz]) == AO.as_bytes(want.x[:nnz])   # the first update gives it values
        assert len(M.x) == want.nzmax and c.cs_norm(M) == PO.cs_norm(want)


def test_errors_change_nothing():
    c = cs()
    ops, coef = override_case()
    nz = [A.p[A.n] for A in ops]
    pops = product_ops(ops)
    P = c.add_plan(*pops, coef=coef)
    nnz = P.nnz
    before = AO.as_bytes(P.matrix.x)
    bad = [dict(values=[np.ones(nz[0] - 1), None, None]), dict(values=[None, [1.0] * (nz[1] + 1), None]),
           dict(values=[None, None, c.dvec(np.ones(nz[2] + 1))]), dict(values=[None, None]), dict(values=[None] * 4),
           dict(coef=[1.0, 2.0]), dict(coef=[1.0] * 4)]
    for kw in bad:
        with pytest.raises(ValueError):
            P.add(**kw)
        with pytest.raises(ValueError):
            P.update(**kw)
    assert AO.as_bytes(P.matrix.x) == before and P.add().numpy().tobytes() == before[:8 * nnz]
    W = AO.csc(c, ops[0].n, ops[0].m, [0] * (ops[0].m + 1), [], [])
    assert c.add_plan(pops[0], W) is None and c.cs_add(pops[0], W, 1, 1) is None      # shapes differ, as cs_add
    T = c.cs_spalloc(ops[0].m, ops[0].n, 1, True, True)
    assert c.add_plan(pops[0], T) is None and c.add_plan(None, pops[0]) is None         # a triplet operand, no operand


def test_c_abi_refuses_what_does_not_fit():
    """the handles' own checks, below the Python layer: nothing is written on a refusal"""
    import _csx
    c = cs()
    lib = _csx.lib()
    ops, coef = override_case()
    pops = [c.cs_pin(A) for A in product_ops(ops)]
    P = c.add_plan(*pops, coef=coef)
    hs = [A._dev.handle.value for A in pops]
    cf = _csx.f64(coef)
    H3 = _csx.H * 3
    out = c.dvec(np.full(P.nnz, 7.0))
    short = c.dvec(np.full(P.nnz - 1, 7.0))
    sevens = out.numpy().tobytes()
    long0 = c.dvec(np.ones(ops[0].p[ops[0].n] + 1))
    Wd = c.cs_pin(AO.csc(c, ops[0].n + 1, ops[0].m, [0] * (ops[0].m + 1), [], []))
    other = c.cs_pin(product_cs(AO.synthetic_cases()[0][1][0]))                  # a matrix of another entry count
    assert other._dev.info()[2] != P.nnz
    refused = [(H3(0, hs[1], hs[2]), out.handle), (H3(long0.handle.value, hs[1], hs[2]), out.handle),
               (H3(out.handle.value, hs[1], hs[2]), out.handle), (H3(hs[0], hs[1], hs[2]), short.handle),
               (H3(hs[0], hs[1], hs[2]), other._dev.handle), (H3(hs[0], hs[1], Wd._dev.handle.value), out.handle),
               (H3(hs[0], hs[1], hs[2]), P._handle)]
    for X, o in refused:
        assert lib.csx_add_plan_run(P._handle, _csx.pd(cf), X, o) == _csx.EINVAL
    assert lib.csx_add_plan_run(P._handle, None, H3(*hs), out.handle) == _csx.EINVAL
    assert lib.csx_add_plan_run(P._handle, _csx.pd(cf), None, out.handle) == _csx.EINVAL
    assert out.numpy().tobytes() == sevens
    # out aliases an input vector: A + A on a matrix without duplicates, where a vector of nnz(A) values is long enough to be out
    Ao = AO.csc(PO, 6, 4, [0, 2, 2, 5, 6], [3, 0, 5, 1, 2, 4], np.arange(1.0, 7.0))
    A = c.cs_pin(product_cs(Ao))
    P2 = c.add_plan(A, A)
    x0 = c.dvec(np.arange(1.0, 7.0))
    two = _csx.f64([1.0, 1.0])
    hA = A._dev.handle.value
    for X in ((_csx.H * 2)(x0.handle.value, hA), (_csx.H * 2)(hA, x0.handle.value), (_csx.H * 2)(x0.handle.value, x0.handle.value)):
        assert lib.csx_add_plan_run(P2._handle, _csx.pd(two), X, x0.handle) == _csx.EINVAL
    assert lib.csx_add_plan_run(P2._handle, _csx.pd(two), (_csx.H * 2)(hA, hA), A._dev.handle) == _csx.EINVAL   # ... or A's own values
    assert x0.numpy().tobytes() == np.arange(1.0, 7.0).tobytes() and AO.as_bytes(A.x[:6]) == np.arange(1.0, 7.0).tobytes()
    h = _csx.new_handle()
    assert lib.csx_add_plan_matrix(P._handle, _csx.pd(cf), H3(hs[0], 0, hs[2]), h) == _csx.EINVAL
    assert lib.csx_add_plan_run(P._handle, _csx.pd(cf), H3(*hs), out.handle) == _csx.OK
    assert out.numpy().tobytes() == AO.as_bytes(AO.chain(PO, ops, coef).x[:P.nnz])
    assert lib.csx_add_plan(2, (_csx.H * 2)(hs[0], Wd._dev.handle.value), h) == _csx.EINVAL    # shapes differ
    assert lib.csx_add_plan(1, (_csx.H * 1)(hs[0]), h) == _csx.EINVAL
    assert lib.csx_add_plan(9, (_csx.H * 9)(*([hs[0]] * 9)), h) == _csx.EINVAL
    assert lib.csx_add_plan_info(hs[0], (_csx.C.c_int64 * 11)()) == _csx.EINVAL


def test_through_the_factors():
    """K + sigma M on the 12 x 12 grid pattern straight into refactor(): the solves of cholsol_factor and of lusol_factor are
    byte-equal to those of fresh factors of cs_add(K, M, 1, sigma)"""
    c = cs()
    Ko, Mo = AO.pencil()
    K, M = product_cs(Ko), product_cs(Mo)
    P = c.add_plan(K, M, coef=(1, 0.5))
    assert P.info()["aligned"] == 1 and (P.m, P.nnz) == (144, Ko.p[144])
    rng = np.random.default_rng(23)
    b = rng.uniform(-1, 1, 144)
    for factor in (c.cholsol_factor, c.lusol_factor):
        F = factor(P.matrix)
        assert F is not None
        for step, sigma in enumerate((0.1 + 1e-9, 2.0 / 3.0)):
            want = PO.cs_add(Ko, Mo, 1, sigma)
            if step == 0:
                v = P.add((1, sigma))
                assert v.numpy().tobytes() == AO.as_bytes(want.x[:P.nnz])
                assert F.refactor(v) is True
            else:
                assert F.refactor(P.update((1, sigma))) is True
                assert AO.as_bytes(P.matrix.x[:P.nnz]) == AO.as_bytes(want.x[:P.nnz])
            fresh = factor(c.cs_add(K, M, 1, sigma))
            assert fresh is not None
            x, xf = b.tolist(), b.tolist()
            assert F.solve(x) is True and fresh.solve(xf) is True
            assert AO.as_bytes(x) == AO.as_bytes(xf)
        P.update((1, 0.5))
