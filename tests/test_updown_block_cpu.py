"""updown_block's column-fused order (tests/updown_block_oracle.py, the device kernel's order) against the loop of rank-1
cs_updown calls it stands for (csparse_oracle, the reference's restatement): L.x byte-equal and the same count applied, for
one and several chunks of 64 terms per tree, mixed signs, a downdate that fails mid-batch (the loop's partial state; with all
or nothing, L as it was), duplicate rows, rows off the path and empty columns.  CPU only."""
import numpy as np
import pytest

import csparse_oracle as O
import synth
import updown_block_oracle as UB
from conftest import golden


def _L_from(p, i, x):
    n = len(p) - 1
    L = O.cs_spalloc(n, n, len(i), True, False)
    L.p, L.i, L.x = [int(v) for v in p], [int(v) for v in i], [float(v) for v in x]
    return L


def _factor(p, i, x):
    n = len(p) - 1
    A = O.cs_spalloc(n, n, len(i), True, False)
    A.p, A.i, A.x = [int(v) for v in p], [int(v) for v in i], [float(v) for v in x]
    N = O.cs_chol(A, O.cs_schol(0, A))
    nz = N.L.p[n]
    return _L_from(N.L.p, N.L.i[:nz], N.L.x[:nz])


def _grid(gx, gy):
    import scipy.sparse as sp
    Tx = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gx, gx))
    Ty = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gy, gy))
    A = (sp.kron(sp.identity(gy), Tx) + sp.kron(Ty, sp.identity(gx)) + 0.01 * sp.identity(gx * gy)).tocsc()
    A.sort_indices()
    return A.indptr, A.indices, A.data


def _factors():
    g = golden("updown")
    yield "bcsstk01", _L_from(g["bcsstk01_L_p"], g["bcsstk01_L_i"], g["bcsstk01_L_x"])
    p, i, x = synth.gspd(5, 12, 3)
    yield "gspd", _factor(p, i, x)
    yield "grid", _factor(*_grid(7, 6))


FACTORS = dict(_factors())


def _copy(L):
    return _L_from(L.p, L.i, L.x)


def _columns(L, k, seed, scale=0.05, extras=True):
    """k columns: f random, rows from L(:, f)'s pattern (so on the path), a few duplicates, rows off the path and empty columns"""
    rng = np.random.default_rng(seed)
    n = L.n
    cols = []
    for t in range(k):
        if extras and t % 11 == 5:
            cols.append(([], []))
            continue
        f = int(rng.integers(0, n))
        pat = L.i[L.p[f]:L.p[f + 1]]
        take = [f] + [int(r) for r in rng.choice(pat, size=min(len(pat), 3), replace=True)]
        vals = [float(v) for v in scale * rng.uniform(-1, 1, len(take))]
        if extras and t % 3 == 1:
            path = set(_path(L, f))
            off = [r for r in range(f + 1, n) if r not in path]
            if off:
                take.append(off[int(rng.integers(0, len(off)))])   # after f, not on its path: assigned, never read
                vals.append(7.0)
        if extras and t % 4 == 2:
            take.append(take[1] if len(take) > 1 else f)  # duplicate: the later one wins
            vals.append(-0.03)
        perm = rng.permutation(len(take))
        cols.append(([take[q] for q in perm], [vals[q] for q in perm]))
    return cols


def _path(L, f):
    out, parent = [], UB.tree_of(L)
    while f != -1:
        out.append(f)
        f = parent[f]
    return out


def _bad_column(L, f):
    """a downdate that is not positive definite part way along f's path: small at f, three times L(r, r) at its parent r"""
    path = _path(L, f)
    if len(path) == 1:
        return [f], [2.0 * L.x[L.p[f]]]
    r = path[1]
    return [r, f], [3.0 * L.x[L.p[r]], 0.3 * L.x[L.p[f]]]


def _C(n, cols):
    C = O.cs_spalloc(n, len(cols), max(1, sum(len(r) for r, _ in cols)), True, False)
    p, i, x = [0], [], []
    for r, v in cols:
        i += r
        x += v
        p.append(len(i))
    C.p, C.i, C.x = p, i or [0], x or [0.0]
    return C


def _signs(mode, k, seed):
    if mode == "up":
        return 1
    if mode == "down":
        return -1
    return [1 if s else -1 for s in np.random.default_rng(seed).integers(0, 2, k)]


def _check(L0, sigma, C, aon=False):
    La, Lb = _copy(L0), _copy(L0)
    parent = UB.tree_of(L0)
    want = UB.loop(La, sigma, C, parent, O)
    got = UB.updown_block(Lb, sigma, C, None, aon)
    assert got == want
    if aon and want < C.n:
        assert np.asarray(Lb.x).tobytes() == np.asarray(L0.x).tobytes()
    else:
        assert np.asarray(Lb.x).tobytes() == np.asarray(La.x).tobytes()
    return want


@pytest.mark.parametrize("name", sorted(FACTORS))
@pytest.mark.parametrize("k", [1, 2, 7, 64, 65, 130])
@pytest.mark.parametrize("mode", ["up", "down", "mixed"])
def test_fused_order_is_the_loop(name, k, mode):
    L0 = FACTORS[name]
    C = _C(L0.n, _columns(L0, k, 11 * k + len(mode), 0.05 if mode == "up" else 0.002))
    got = _check(L0, _signs(mode, k, k), C)
    assert got == k or mode != "up"                 # (the grid's smallest eigenvalue is 0.01: downdates may fail there)


@pytest.mark.parametrize("name", sorted(FACTORS))
@pytest.mark.parametrize("aon", [False, True])
@pytest.mark.parametrize("k,bad", [(7, 3), (65, 64), (130, 70)])
def test_failing_downdate_mid_batch(name, aon, k, bad):
    L0 = FACTORS[name]
    cols = _columns(L0, k, 5 * k + bad, 0.002, extras=False)
    cols[bad] = _bad_column(L0, min(cols[bad][0]))
    C = _C(L0.n, cols)
    sig = [1 if t % 2 else -1 for t in range(k)]
    sig[bad] = -1
    assert _check(L0, sig, C, aon) == bad


def test_many_terms_in_one_tree_and_chunks_across_trees():
    """ranks 0..63 of each tree in chunk 0: with a second tree of few terms the chunks of the big tree run beside it"""
    L0 = FACTORS["gspd"]
    n = L0.n
    cols = []
    rng = np.random.default_rng(2)
    for t in range(150):
        b = 0 if t % 5 else 1 + t % 4                       # most terms in block 0, the others spread
        f = 12 * b + int(rng.integers(0, 12))
        pat = L0.i[L0.p[f]:L0.p[f + 1]]
        rows = [int(r) for r in rng.choice(pat, size=min(len(pat), 4), replace=False)]
        cols.append((rows, [float(v) for v in 0.02 * rng.uniform(-1, 1, len(rows))]))
    C = _C(n, cols)
    sig = [1 if t % 3 else -1 for t in range(150)]
    assert _check(L0, sig, C) == 150


def test_empty_and_k0():
    L0 = FACTORS["bcsstk01"]
    C = _C(L0.n, [([], []), ([], [])])
    L = _copy(L0)
    assert UB.updown_block(L, 1, C) == 2 and L.x == L0.x
    assert UB.updown_block(L, 1, _C(L0.n, [])) == 0
