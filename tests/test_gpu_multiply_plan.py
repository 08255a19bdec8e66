"""multiply_plan on the device (include/csx.h "multiply plan"): the pattern is the oracle's exactly, every
comparison of values is byte equality against tests/multiply_plan_oracle.py or the oracle's cs_multiply, at the smallest
shapes where each kernel class (one lane per slot, one wave per long slot, the scale) can go wrong."""
import hashlib

import numpy as np
import pytest

import csparse_oracle as PO
import multiply_plan_oracle as MO

pytestmark = pytest.mark.gpu

GOLDEN = [(name, False) for name in MO.GOLDEN] + [(name, True) for name in MO.SMALL]
GOLDEN_IDS = ["%s-%s" % (name, "ATA" if tr else "AAT") for name, tr in GOLDEN]


def cs():
    import csparse
    return csparse


def threshold():
    import _csx
    v = _csx.C.c_int(0)
    _csx.check(_csx.lib().csx_get_option(b"multiply.long", v), "csx_get_option")
    return v.value


def product_cs(Ao, values=True):
    """the product module's copy of an oracle matrix"""
    return MO.csc(cs(), Ao.m, Ao.n, Ao.p, Ao.i, Ao.x if values else None)


def check_plan(Ao, Bo):
    """plan, .matrix and .multiply against the restatement and the oracle's product; returns (P, (p, i, sp, pair))"""
    c = cs()
    ref = MO.plan(Ao, Bo)
    p, i, sp, pair = ref
    nnz = p[Bo.n]
    Cref = PO.cs_multiply(Ao, Bo)
    assert p == Cref.p and i == Cref.i[:nnz] and len(Cref.x) == nnz
    want = MO.as_bytes(Cref.x)
    assert MO.as_bytes(MO.fold(sp, pair, Ao.x, Bo.x)) == want
    P = c.multiply_plan(product_cs(Ao), product_cs(Bo))
    assert (P.m, P.n, P.k, P.nnz, P.products) == (Ao.m, Bo.n, Ao.n, nnz, sp[nnz])
    info = P.info()
    lens = [sp[s + 1] - sp[s] for s in range(nnz)]
    assert (info["m"], info["n"], info["nnz"], info["products"]) == (Ao.m, Bo.n, nnz, sp[nnz])
    assert info["max_products"] == max(lens, default=0) and info["build_us"] >= 0
    assert info["long_slots"] == sum(1 for v in lens if v > threshold())
    got = P.multiply()
    assert len(got) == nnz and got.numpy().tobytes() == want
    assert P.info()["kernel_us"] >= 0
    M = P.matrix
    assert M is P.matrix and (M.m, M.n, M.nz, M.nzmax) == (Ao.m, Bo.n, -1, nnz)
    assert M.p == p and M.i == i and len(M.i) == nnz
    assert MO.as_bytes(M.x) == want and len(M.x) == nnz
    return P, ref


@pytest.mark.parametrize("nnz", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_slot_counts_at_wave_and_workgroup_edges(nnz):
    """A is nnz x 1 with distinct rows in shuffled order, B is 1 x 1: one product per slot"""
    rng = np.random.default_rng(nnz)
    A = MO.csc(PO, nnz, 1, [0, nnz], rng.permutation(nnz), MO.wide(rng, nnz))
    B = MO.csc(PO, 1, 1, [0, 1], [0], MO.wide(rng, 1))
    P, _ = check_plan(A, B)
    assert P.info()["max_products"] == 1 and P.info()["long_slots"] == 0 and P.products == nnz


def boundary_case(thr, seed):
    """A 4 x 3 product whose 12 slots have the lengths at the class boundary and at the wave's step.  Slot s is entry
    (s % 4, s // 4) and has its own inner indices, shuffled over 0 .. k-1: A(:,c) is the one entry (s % 4, c), B(c, s // 4)
    the other factor.  B's columns store their rows shuffled: not ascending, the slots of a column interleaved."""
    special = {9: [-0.0] * 200, 10: [-0.0, 0.0], 11: [1e8, -1e8, 1e-8]}
    lens = [1, 2, thr - 1, thr, thr + 1, 127, 128, 129, 4097] + [len(special[s]) for s in (9, 10, 11)]
    assert min(lens) >= 1
    k = sum(lens)
    rng = np.random.default_rng(seed)
    slot_of = rng.permutation(np.repeat(np.arange(12), lens))          # inner index -> its slot
    Ai, Ax = slot_of % 4, MO.wide(rng, k)
    cols = [rng.permutation(np.flatnonzero(slot_of // 4 == j)) for j in range(3)]
    Bi = np.concatenate(cols)
    Bp = np.concatenate([[0], np.cumsum([len(v) for v in cols])])
    Bx = MO.wide(rng, k)
    assert all(np.any(np.diff(v) < 0) for v in cols)
    for s, vals in special.items():                                     # the slot's terms, in the order B stores them
        at = np.flatnonzero(slot_of[Bi] == s)
        Bx[at] = 1.0
        Ax[Bi[at]] = vals
    A = MO.csc(PO, 4, k, np.arange(k + 1), Ai, Ax)
    B = MO.csc(PO, k, 3, Bp, Bi, Bx)
    return A, B, lens


@pytest.mark.parametrize("long_option", [None, 2])
def test_slot_lengths_at_the_class_boundary(long_option):
    import _csx

    def run():
        thr = threshold()
        A, B, lens = boundary_case(thr, 5)
        P, (p, i, sp, pair) = check_plan(A, B)
        assert p[3] == 12 and sorted(sp[s + 1] - sp[s] for s in range(12)) == sorted(lens)
        info = P.info()
        assert info["products"] == sum(lens) and info["max_products"] == 4097
        assert info["long_slots"] == sum(1 for v in lens if v > thr) >= 5
        x = P.multiply().numpy()
        # the comparison separates the right kernel from the two plausible wrong ones
        assert x.tobytes() != MO.as_bytes(MO.fold(sp, pair, A.x, B.x, reverse=True))
        assert x.tobytes() != MO.as_bytes(MO.fold(sp, pair, A.x, B.x, fused=True))
        at = {(i[s], j): s for j in range(3) for s in range(p[j], p[j + 1])}
        assert MO.as_bytes([x[at[9 % 4, 9 // 4]]]) == MO.as_bytes([-0.0])     # 200 terms, all -0.0
        assert MO.as_bytes([x[at[10 % 4, 10 // 4]]]) == MO.as_bytes([0.0])    # -0.0 + 0.0
        assert x[at[11 % 4, 11 // 4]] == 1e-8                                 # (1e8 + -1e8) + 1e-8

    if long_option is None:
        run()
    else:
        with _csx.option("multiply.long", long_option):
            assert threshold() == long_option
            run()


@pytest.mark.parametrize("name,transposed", GOLDEN, ids=GOLDEN_IDS)
def test_golden_matrices(name, transposed, meta):
    c = cs()
    Ao, Bo = MO.golden_pair(name, transposed)
    Cp, Ci, Cx = MO.c_multiply(Ao, Bo)
    nnz = Cp[-1]
    A, B = product_cs(Ao), product_cs(Bo)
    P = c.multiply_plan(A, B)
    M = P.matrix
    assert (M.m, M.n, M.nz, M.nzmax, P.nnz) == (Ao.m, Bo.n, -1, nnz, nnz)
    assert M.p == Cp and M.i == Ci and len(M.i) == nnz
    D = c.cs_multiply(A, B)
    assert D.p == Cp and D.i[:nnz] == Ci
    assert MO.as_bytes(M.x) == Cx.tobytes() and len(M.x) == nnz
    first = P.multiply().numpy().tobytes()
    assert first == Cx.tobytes() and P.multiply().numpy().tobytes() == first
    if not transposed:
        mm = meta[name]["AAT"]
        assert hashlib.sha256(first).hexdigest() == mm["sha_x"]
        assert hashlib.sha256(np.asarray(M.p, np.int64).tobytes()).hexdigest() == mm["sha_p"]
        assert hashlib.sha256(np.asarray(M.i, np.int64).tobytes()).hexdigest() == mm["sha_i"]
    assert P.info()["kernel_us"] >= 0 and P.info()["products"] >= nnz


DUPLICATES = [c for c in MO.edge_pairs() if c[0] in ("duplicates", "negzero", "single")] + MO.synthetic_pairs()[:12]


@pytest.mark.parametrize("case", DUPLICATES, ids=lambda c: c[0])
def test_duplicates_inside_columns_of_a_and_of_b(case):
    """the same row stored twice in a column of A, and of B (the synthetic cases have both): plan and values"""
    label, A, B = case
    P, (p, i, sp, pair) = check_plan(A, B)
    if label == "duplicates":
        assert any(len(set(A.i[A.p[j]:A.p[j + 1]])) < A.p[j + 1] - A.p[j] for j in range(A.n))
        assert any(len(set(B.i[B.p[j]:B.p[j + 1]])) < B.p[j + 1] - B.p[j] for j in range(B.n))


@pytest.mark.parametrize("case", MO.wide_pairs()[:2] + MO.synthetic_pairs()[10:12], ids=lambda c: c[0])
def test_scale(case):
    c = cs()
    label, A, B = case
    rng = np.random.default_rng(len(label))
    d = MO.wide(rng, A.n)
    Cref = PO.cs_multiply(A, MO.scaled(PO, B, d))
    P = c.multiply_plan(product_cs(A), product_cs(B))
    assert P.matrix.p == Cref.p and P.matrix.i == Cref.i[:P.nnz]
    plain = P.multiply().numpy().tobytes()
    for given in (d, d.tolist(), c.dvec(d)):
        assert P.multiply(scale=given).numpy().tobytes() == MO.as_bytes(Cref.x)
    assert MO.as_bytes(Cref.x) != plain
    assert P.multiply(scale=np.ones(A.n)).numpy().tobytes() == plain == MO.as_bytes(PO.cs_multiply(A, B).x)
    assert P.multiply().numpy().tobytes() == plain                      # the scratch of a scaled step is not B's values


def test_value_overrides():
    c = cs()
    label, Ao, Bo = MO.wide_pairs()[2]
    rng = np.random.default_rng(21)
    anz, bnz = Ao.p[Ao.n], Bo.p[Bo.n]
    ax2, bx2, d = MO.wide(rng, anz), MO.wide(rng, bnz), MO.wide(rng, Ao.n)
    A, B = product_cs(Ao), product_cs(Bo)
    P = c.multiply_plan(A, B)
    A2, B2 = MO.csc(PO, Ao.m, Ao.n, Ao.p, Ao.i, ax2), MO.csc(PO, Bo.m, Bo.n, Bo.p, Bo.i, bx2)
    want_a = MO.as_bytes(PO.cs_multiply(A2, Bo).x)
    want_b = MO.as_bytes(PO.cs_multiply(Ao, B2).x)
    want_ab = MO.as_bytes(PO.cs_multiply(A2, B2).x)
    want_abd = MO.as_bytes(PO.cs_multiply(A2, MO.scaled(PO, B2, d)).x)
    assert len({want_a, want_b, want_ab, want_abd}) == 4
    da, db = c.dvec(ax2), c.dvec(bx2)
    la, lb = ax2.tolist(), bx2.tolist()
    for ga, gb in ((ax2, bx2), (la, lb), (da, db)):
        assert P.multiply(ax=ga).numpy().tobytes() == want_a
        assert P.multiply(bx=gb).numpy().tobytes() == want_b
        assert P.multiply(ax=ga, bx=gb).numpy().tobytes() == want_ab
        assert P.multiply(ga, gb, d).numpy().tobytes() == want_abd
    # the inputs are unchanged afterwards, and so are the operands
    assert da.numpy().tobytes() == ax2.tobytes() and db.numpy().tobytes() == bx2.tobytes()
    assert la == ax2.tolist() and lb == bx2.tolist()
    assert MO.as_bytes(A.x[:anz]) == MO.as_bytes(Ao.x[:anz]) and MO.as_bytes(B.x[:bnz]) == MO.as_bytes(Bo.x[:bnz])
    assert P.multiply().numpy().tobytes() == MO.as_bytes(PO.cs_multiply(Ao, Bo).x)


def test_update_in_place():
    c = cs()
    Ao, Bo = MO.golden_pair("west0067")
    rng = np.random.default_rng(22)
    d = rng.uniform(0.5, 2.0, Ao.n)
    C1, C2 = PO.cs_multiply(Ao, Bo), PO.cs_multiply(Ao, MO.scaled(PO, Bo, d))
    P = c.multiply_plan(product_cs(Ao), product_cs(Bo))
    M = P.matrix
    n = M.n
    xs = rng.uniform(-1, 1, n).tolist()
    y, yo = [0.0] * M.m, [0.0] * M.m
    assert c.cs_gaxpy(M, xs, y) and PO.cs_gaxpy(C1, xs, yo)    # exact mode for lists: builds and caches the row-gather plan
    assert MO.as_bytes(y) == MO.as_bytes(yo)
    held = M.x                                                  # a host list read before the update
    assert MO.as_bytes(held) == MO.as_bytes(C1.x)
    version = M._dev.version
    assert P.update(scale=d) is M and P.matrix is M and M._dev.version == version + 1
    assert held is M.x and MO.as_bytes(held) == MO.as_bytes(C2.x)
    y, yo = [0.0] * M.m, [0.0] * M.m
    assert c.cs_gaxpy(M, xs, y) and PO.cs_gaxpy(C2, xs, yo)
    assert MO.as_bytes(y) == MO.as_bytes(yo)                    # the cached SpMV plan held the old values: it was dropped
    assert c.cs_norm(M) == PO.cs_norm(C2)
    assert P.update() is M and MO.as_bytes(M.x) == MO.as_bytes(C1.x) and held is M.x


def test_pattern_only_operands():
    c = cs()
    label, Ao, Bo = MO.wide_pairs()[3]
    want = PO.cs_multiply(Ao, Bo)
    anz, bnz = Ao.p[Ao.n], Bo.p[Bo.n]
    for a_values, b_values in ((False, True), (True, False), (False, False)):
        P = c.multiply_plan(product_cs(Ao, a_values), product_cs(Bo, b_values))
        M = P.matrix
        assert M.x is None and M.p == want.p and M.i == want.i[:P.nnz] and M.nzmax == want.p[Bo.n]
        given = dict(([] if a_values else [("ax", Ao.x[:anz])]) + ([] if b_values else [("bx", Bo.x[:bnz])]))
        with pytest.raises(ValueError):
            P.multiply()
        with pytest.raises(ValueError):
            P.update()
        for name in given:
            if len(given) == 2:
                with pytest.raises(ValueError):
                    P.multiply(**{name: given[name]})
        assert P.multiply(**given).numpy().tobytes() == MO.as_bytes(want.x)
        assert P.matrix.x is None
        assert P.update(**given) is M and MO.as_bytes(M.x) == MO.as_bytes(want.x)   # the first update gives it its values
        assert c.cs_norm(M) == PO.cs_norm(want)


@pytest.mark.parametrize("case", [c for c in MO.edge_pairs() if c[0] in ("k0", "n0", "m0", "products0", "empty_columns")],
                         ids=lambda c: c[0])
def test_empty_shapes(case):
    label, A, B = case
    P, (p, i, sp, pair) = check_plan(A, B)
    if label != "empty_columns":
        assert P.nnz == 0 and P.products == 0 and P.matrix.p == [0] * (B.n + 1) and len(P.multiply()) == 0
        assert P.update() is P.matrix
        assert len(P.multiply(scale=[1.0] * A.n)) == 0


def test_errors_change_nothing():
    c = cs()
    label, Ao, Bo = MO.wide_pairs()[0]
    anz, bnz, k = Ao.p[Ao.n], Bo.p[Bo.n], Ao.n
    A, B = product_cs(Ao), product_cs(Bo)
    P = c.multiply_plan(A, B)
    before = MO.as_bytes(P.matrix.x)
    bad = [dict(ax=np.ones(anz - 1)), dict(ax=np.ones(anz + 1)), dict(ax=c.dvec(np.ones(anz + 1))), dict(bx=[1.0] * (bnz - 1)),
           dict(bx=c.dvec(np.ones(bnz + 1))), dict(scale=np.ones(k - 1)), dict(scale=[1.0] * (k + 1)),
           dict(scale=c.dvec(np.ones(k + 1)))]
    for kw in bad:
        with pytest.raises(ValueError):
            P.multiply(**kw)
        with pytest.raises(ValueError):
            P.update(**kw)
    assert MO.as_bytes(P.matrix.x) == before == P.multiply().numpy().tobytes()
    assert c.multiply_plan(A, A) is None                                   # A.n != B.m, as cs_multiply
    assert c.cs_multiply(A, A) is None
    T = c.cs_spalloc(k, 3, 1, True, True)
    assert c.multiply_plan(A, T) is None and c.multiply_plan(T, B) is None  # a triplet operand
    assert c.multiply_plan(None, B) is None


def test_c_abi_refuses_what_does_not_fit():
    """the handles' own checks, below the Python layer: nothing is written on a refusal"""
    import _csx
    c = cs()
    lib = _csx.lib()
    label, Ao, Bo = MO.wide_pairs()[1]
    A, B = c.cs_pin(product_cs(Ao)), c.cs_pin(product_cs(Bo))
    P = c.multiply_plan(A, B)
    hA, hB = A._dev.handle, B._dev.handle
    out = c.dvec(np.full(P.nnz, 7.0))
    short = c.dvec(np.full(max(P.nnz - 1, 0), 7.0))
    d_short = c.dvec(np.ones(Ao.n - 1))
    sevens = out.numpy().tobytes()
    for args in ((hB, hB, 0, out.handle), (hA, hA, 0, out.handle), (hA, hB, d_short.handle, out.handle), (hA, hB, 0, short.handle),
                 (hA, 0, 0, out.handle), (hA, hB, out.handle, out.handle), (hA, hB, 0, hA)):
        assert lib.csx_multiply_plan_run(P._handle, *args) == _csx.EINVAL
    ax = c.dvec(np.asarray(Ao.x[:Ao.p[Ao.n]]))
    assert lib.csx_multiply_plan_run(P._handle, ax.handle, hB, 0, ax.handle) == _csx.EINVAL   # out aliases an input
    assert out.numpy().tobytes() == sevens
    h = _csx.new_handle()
    assert lib.csx_multiply_plan_matrix(P._handle, hA, 0, 0, h) == _csx.EINVAL
    assert lib.csx_multiply_plan_run(P._handle, hA, hB, 0, out.handle) == _csx.OK
    assert out.numpy().tobytes() == MO.as_bytes(PO.cs_multiply(Ao, Bo).x)
    assert lib.csx_multiply_plan(hA, hA, h) == _csx.EINVAL                 # A.n != B.m
    assert lib.csx_multiply_plan_info(hA, (_csx.C.c_int64 * 8)()) == _csx.EINVAL


def test_into_the_factor_end_to_end():
    """A' diag(d) A of ash219 (219 x 85; A'A is positive definite, smallest eigenvalue 1.3) straight into cholsol_factor's
    refactor: L.x and a list solve byte-equal to a fresh factor of the oracle's product"""
    import _csx
    c = cs()
    ATo, Ao = MO.golden_pair("ash219", True)
    assert (Ao.m, Ao.n) == (219, 85)
    P = c.multiply_plan(product_cs(ATo), product_cs(Ao))
    C0 = PO.cs_multiply(ATo, Ao)
    assert P.matrix.p == C0.p and P.matrix.i == C0.i[:P.nnz] and MO.as_bytes(P.matrix.x) == MO.as_bytes(C0.x)
    F = c.cholsol_factor(P.matrix)
    assert F is not None

    def device_Lx(G):
        dev = G.L._dev
        nnz = dev.info()[2]
        x = np.empty(max(nnz, 1), np.float64)
        _csx.check(_csx.lib().csx_csc_download(dev.handle, None, None, _csx.pd(x)), "csx_csc_download")
        return x[:nnz].tobytes()

    rng = np.random.default_rng(23)
    b = rng.uniform(-1, 1, 85)
    for step in range(2):
        d = rng.uniform(0.5, 2.0, 219)
        Cd = PO.cs_multiply(ATo, MO.scaled(PO, Ao, d))
        assert Cd.p == C0.p and Cd.i == C0.i
        if step == 0:
            v = P.multiply(scale=d)
            assert v.numpy().tobytes() == MO.as_bytes(Cd.x)
            assert F.refactor(v) is True
        else:
            assert F.refactor(P.update(scale=d)) is True
            assert MO.as_bytes(P.matrix.x) == MO.as_bytes(Cd.x)
        fresh = c.cholsol_factor(MO.csc(c, Cd.m, Cd.n, Cd.p, Cd.i, Cd.x))
        assert fresh is not None and device_Lx(F) == device_Lx(fresh)
        x, xf = b.tolist(), b.tolist()
        assert F.solve(x) is True and fresh.solve(xf) is True
        assert MO.as_bytes(x) == MO.as_bytes(xf)
