"""assembly_plan on the device (include/csx.h "assembly plan"): the pattern is the oracle's exactly, every
comparison of values is byte equality against tests/assemble_oracle.py or the oracle's cs_dupl(cs_compress(T)), at the
smallest shapes where each kernel class (permuted copy, one lane per slot, one wave per long slot) can go wrong."""
import numpy as np
import pytest

import assemble_oracle as AO
import csparse_oracle as PO
import tol

pytestmark = pytest.mark.gpu

GOLDEN = [(name, split) for name in AO.GOLDEN_WITH_TRIPLETS for split in (False, True)]
GOLDEN_IDS = ["%s-%s" % (c[0], "split" if c[1] else "plain") for c in GOLDEN]


def cs():
    import csparse
    return csparse


def threshold():
    import _csx
    v = _csx.C.c_int(0)
    _csx.check(_csx.lib().csx_get_option(b"assemble.long", v), "csx_get_option")
    return v.value


def check_plan(m, n, Ti, Tj, Tx, pattern_only=False):
    """plan, .matrix and .assemble against the restatement; returns (P, (p, i, sp, src))"""
    c = cs()
    ref = AO.plan(m, n, Ti, Tj)
    p, i, sp, src = ref
    P = c.assembly_plan(AO.triplet(c, m, n, Ti, Tj, None if pattern_only else Tx))
    assert (P.m, P.n, P.nz, P.nnz) == (m, n, len(Ti), p[n])
    info = P.info()
    lens = [sp[s + 1] - sp[s] for s in range(p[n])]
    assert (info["nz"], info["nnz"], info["max_dup"]) == (len(Ti), p[n], max(lens, default=0))
    assert info["long_slots"] == sum(1 for v in lens if v > threshold())
    got = P.assemble(Tx)
    assert len(got) == p[n] and got.numpy().tobytes() == AO.as_bytes(AO.fold(sp, src, Tx))
    M = P.matrix
    assert M is P.matrix and (M.m, M.n, M.nz, M.nzmax) == (m, n, -1, p[n])
    assert M.p == p and M.i == i and len(M.i) == p[n]
    if pattern_only:
        assert M.x is None
    else:
        assert AO.as_bytes(M.x) == AO.as_bytes(AO.fold(sp, src, Tx)) and len(M.x) == p[n]
    return P, ref


@pytest.mark.parametrize("nnz", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_slot_counts_at_wave_and_workgroup_edges(nnz):
    """one column, all rows distinct: the permuted copy (nz == nnz)"""
    rng = np.random.default_rng(nnz)
    Ti = rng.permutation(nnz)
    P, _ = check_plan(nnz, 1, Ti, np.zeros(nnz, np.int64), AO.wide(rng, nnz))
    assert P.info()["max_dup"] == 1 and P.info()["long_slots"] == 0


def boundary_case(rows, extra, seed):
    """a rows x 3 matrix whose slots have the lengths at the class boundary and at the wave's step; slot k is entry
    (k % rows, k // rows); the triplets are interleaved, not grouped; extra: (length, values in triplet order) of further slots"""
    thr = threshold()
    lens = [1, 2, thr - 1, thr, thr + 1, 127, 128, 129, 4097] + [v[0] for v in extra]
    assert len(lens) <= 3 * rows and min(lens) >= 1
    rng = np.random.default_rng(seed)
    slot = rng.permutation(np.repeat(np.arange(len(lens)), lens))
    Tx = AO.wide(rng, len(slot))
    for k, (_, vals) in enumerate(extra):
        Tx[np.flatnonzero(slot == 9 + k)] = vals
    return rows, 3, slot % rows, slot // rows, Tx, lens


@pytest.mark.parametrize("long_option", [None, 2])
@pytest.mark.parametrize("shape", ["3x3", "4x3"])
def test_slot_lengths_at_the_class_boundary(shape, long_option):
    import _csx
    extra = [] if shape == "3x3" else [(200, [-0.0] * 200), (2, [-0.0, 0.0]), (3, [1e8, -1e8, 1e-8])]

    def run():
        m, n, Ti, Tj, Tx, lens = boundary_case(3 if shape == "3x3" else 4, extra, 5)
        P, (p, i, sp, src) = check_plan(m, n, Ti, Tj, Tx)
        assert sorted(sp[s + 1] - sp[s] for s in range(p[n])) == sorted(lens)
        x = P.assemble(Tx).numpy()
        # the comparison separates the right order from a plausible wrong one
        assert x.tobytes() != AO.as_bytes(AO.fold(sp, src, Tx, reverse=True))
        if extra:
            at = {(i[s], j): s for j in range(n) for s in range(p[j], p[j + 1])}
            assert AO.as_bytes([x[at[9 % m, 9 // m]]]) == AO.as_bytes([-0.0])    # 200 terms, all -0.0
            assert AO.as_bytes([x[at[10 % m, 10 // m]]]) == AO.as_bytes([0.0])   # -0.0 + 0.0
            assert x[at[11 % m, 11 // m]] == 1e-8                                # (1e8 + -1e8) + 1e-8
        assert P.info()["long_slots"] >= 3

    if long_option is None:
        run()
    else:
        with _csx.option("assemble.long", long_option):
            run()


def test_structure_edges():
    c = cs()
    for case in AO.random_cases():
        label, m, n, Ti, Tj, Tx = case
        P, (p, i, sp, src) = check_plan(m, n, Ti, Tj, Tx)
        if label == "nz0":
            assert P.nnz == 0 and P.matrix.p == [0] * (n + 1) and len(P.assemble([])) == 0
            assert P.update([]) is P.matrix
    # src at both ends: triplets 0 and nz - 1 share a slot that nothing else touches
    rng = np.random.default_rng(3)
    nz = 300
    Ti, Tj = rng.integers(0, 5, nz), rng.integers(0, 4, nz)
    Ti[0] = Ti[-1] = 5
    Tj[0] = Tj[-1] = 2
    P, (p, i, sp, src) = check_plan(6, 4, Ti, Tj, AO.wide(rng, nz))
    s = [s for s in range(p[4]) if src[sp[s]] == 0][0]
    assert src[sp[s]:sp[s + 1]] == [0, nz - 1]
    # a pattern-only T: the matrix has no values until the first update gives it some
    Tx = AO.wide(rng, nz)
    P, (p, i, sp, src) = check_plan(6, 4, Ti, Tj, Tx, pattern_only=True)
    with pytest.raises(ValueError):
        P.update()
    M = P.update(Tx)
    assert M is P.matrix and AO.as_bytes(M.x) == AO.as_bytes(AO.fold(sp, src, Tx)) and M.p == p and M.i == i
    assert c.cs_norm(M) == PO.cs_norm(AO.composite(PO, 6, 4, Ti, Tj, Tx))


@pytest.mark.parametrize("name,split", GOLDEN, ids=GOLDEN_IDS)
def test_golden_matrices(name, split):
    c = cs()
    m, n, Ti, Tj, Tx, Cref = AO.golden_case(name, split)
    p, i, sp, src = AO.golden_plan(name, split)
    P = c.assembly_plan(AO.triplet(c, m, n, Ti, Tj, Tx))
    M = P.matrix
    assert (M.m, M.n, M.nz, M.nzmax) == (Cref.m, Cref.n, -1, Cref.nzmax)
    assert M.p == Cref.p and M.i == Cref.i and len(M.i) == len(Cref.i)
    assert AO.as_bytes(M.x) == AO.as_bytes(Cref.x) and len(M.x) == len(Cref.x)
    v1 = P.assemble(Tx)
    first = v1.numpy()
    assert first.tobytes() == AO.as_bytes(Cref.x)
    rng = np.random.default_rng(len(Ti))
    Tx2 = AO.wide(rng, len(Ti))
    d2 = c.dvec(Tx2)
    v2 = P.assemble(d2)
    want2 = AO.as_bytes(AO.fold(sp, src, Tx2))
    assert v2.numpy().tobytes() == want2
    assert v1.numpy().tobytes() == first.tobytes()            # a second assemble leaves the first result alone
    assert d2.numpy().tobytes() == Tx2.tobytes()              # a dvec input is not modified
    assert P.assemble(Tx2.tolist()).numpy().tobytes() == want2   # the same input, the same bytes (list / numpy / dvec)
    assert P.info()["kernel_us"] >= 0


def mesh(ne, seed):
    """Bilinear quads on an ne x ne grid of unit squares, 16 triplets per element in element order.  Local matrix
    c_e K + d_e M with K the Laplace stiffness and M the LUMPED mass matrix (1/4 on the diagonal): K's columns sum to zero with
    a positive diagonal (|off-diagonals| = diagonal), so any d_e > 0 makes every element column, and therefore every
    assembled column, strictly diagonally dominant."""
    K = np.array([[4, -1, -2, -1], [-1, 4, -1, -2], [-2, -1, 4, -1], [-1, -2, -1, 4]], dtype=np.float64) / 6.0
    Ml = np.eye(4) / 4.0
    ex, ey = np.meshgrid(np.arange(ne), np.arange(ne), indexing="ij")
    n0 = (ex * (ne + 1) + ey).ravel()
    nodes = np.stack([n0, n0 + ne + 1, n0 + ne + 2, n0 + 1], axis=1)            # (elements, 4)
    Ti = np.repeat(nodes, 4, axis=1).ravel()                                   # local (a, b): row nodes[a], column nodes[b]
    Tj = np.tile(nodes, (1, 4)).ravel()

    def values(seed):
        rng = np.random.default_rng(seed)
        ce, de = rng.uniform(0.5, 2.0, ne * ne), rng.uniform(1.0, 2.0, ne * ne)
        return (ce[:, None, None] * K + de[:, None, None] * Ml).reshape(-1)

    return (ne + 1) ** 2, Ti, Tj, values


def product_csc(Co):
    c = cs()
    A = c.cs_spalloc(Co.m, Co.n, max(Co.nzmax, 1), True, False)
    A.p, A.i, A.x = list(Co.p), list(Co.i), list(Co.x)
    return A


@pytest.fixture(scope="module")
def mesh_case():
    n, Ti, Tj, values = mesh(40, 0)
    v1, v2 = values(1), values(2)
    return n, Ti, Tj, v1, v2, AO.composite(PO, n, n, Ti, Tj, v1), AO.composite(PO, n, n, Ti, Tj, v2)


@pytest.mark.parametrize("factor", ["lusol_factor", "btf_factor"])
def test_mesh_plan_factor_refactor(mesh_case, factor):
    c = cs()
    n, Ti, Tj, v1, v2, C1, C2 = mesh_case
    S2 = tol.csc(n, C2.p, C2.i, C2.x)
    diag = np.abs(S2.diagonal())
    assert np.all(diag > np.asarray(abs(S2).sum(axis=0)).ravel() - diag)       # strictly column diagonally dominant
    P = c.assembly_plan(AO.triplet(c, n, n, Ti, Tj, v1))
    assert P.matrix.p == C1.p and P.matrix.i == C1.i and P.info()["max_dup"] == 4
    F = getattr(c, factor)(P.matrix)
    assert F is not None
    dv2 = P.assemble(v2)
    assert dv2.numpy().tobytes() == AO.as_bytes(C2.x)
    assert F.refactor(dv2) is True
    fresh = getattr(c, factor)(product_csc(C2))
    b = np.random.default_rng(4).uniform(-1, 1, n)
    x, xf = b.tolist(), b.tolist()
    assert F.solve(x) is True and fresh.solve(xf) is True
    pinv = (lambda f: f.factors.pinv)
    same = F.refactor_info()["pivot_ratio"] == 1.0 and list(pinv(F)) == list(pinv(fresh))
    if factor == "btf_factor":
        same = same and all(np.array_equal(getattr(F.factors, k), getattr(fresh.factors, k)) for k in ("p", "q", "r"))
    if same:
        assert np.asarray(x).tobytes() == np.asarray(xf).tobytes()
    else:
        assert tol.normwise(x, xf) <= tol.cross_bound(tol.cond1(S2))


def test_update_in_place(mesh_case):
    c = cs()
    n, Ti, Tj, v1, v2, C1, C2 = mesh_case
    P = c.assembly_plan(AO.triplet(c, n, n, Ti, Tj, v1))
    M = P.matrix
    xs = np.random.default_rng(8).uniform(-1, 1, n).tolist()
    y = [0.0] * n
    assert c.cs_gaxpy(M, xs, y)                   # exact mode for lists: builds and caches the row-gather plan
    yo = [0.0] * n
    assert PO.cs_gaxpy(C1, xs, yo) and AO.as_bytes(y) == AO.as_bytes(yo)
    held = M.x                                    # a host list read before the update
    assert AO.as_bytes(held) == AO.as_bytes(C1.x)
    version = M._dev.version
    assert P.update(v2) is M and M._dev.version == version + 1
    assert held is M.x and AO.as_bytes(held) == AO.as_bytes(C2.x)
    y, yo = [0.0] * n, [0.0] * n
    assert c.cs_gaxpy(M, xs, y) and PO.cs_gaxpy(C2, xs, yo)
    assert AO.as_bytes(y) == AO.as_bytes(yo)      # the cached SpMV plan held the old values: it was dropped
    assert c.cs_norm(M) == PO.cs_norm(C2)
    F = c.lusol_factor(M)                         # a new factorisation sees the new values
    Ff = c.lusol_factor(product_csc(C2))
    b = np.random.default_rng(9).uniform(-1, 1, n)
    x, xf = b.tolist(), b.tolist()
    assert F.solve(x) and Ff.solve(xf) and AO.as_bytes(x) == AO.as_bytes(xf)


def test_errors_change_nothing():
    c = cs()
    rng = np.random.default_rng(12)
    m, n, nz = 6, 5, 90
    Ti, Tj, Tx = rng.integers(0, m, nz), rng.integers(0, n, nz), AO.wide(rng, nz)
    P = c.assembly_plan(AO.triplet(c, m, n, Ti, Tj, Tx))
    before = AO.as_bytes(P.matrix.x)
    for bad in (np.ones(nz - 1), np.ones(nz + 1), c.dvec(np.ones(nz + 1)), [1.0] * (nz - 1)):
        with pytest.raises(ValueError):
            P.assemble(bad)
        with pytest.raises(ValueError):
            P.update(bad)
    assert AO.as_bytes(P.matrix.x) == before
    d = c.dvec(Tx)
    assert P.assemble(d).numpy().tobytes() == before and d.numpy().tobytes() == Tx.tobytes()
    for Ti_bad, Tj_bad in (([0, m], [0, 1]), ([0, 1], [0, n]), ([-1, 1], [0, 1])):
        T = AO.triplet(c, m, n, Ti_bad, Tj_bad, [1.0, 2.0])
        with pytest.raises(IndexError, match="list index out of range"):
            c.assembly_plan(T)
    assert c.assembly_plan(P.matrix) is None      # not a triplet matrix
