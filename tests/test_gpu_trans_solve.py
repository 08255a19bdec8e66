"""Transposed solves and condest() on the device: lusol_factor(A).solve(b, trans=True) byte-equal to
cs_pvec(q), cs_utsolve(U), cs_ltsolve(L), cs_pvec(pinv) on the factor's own factors in the exact order, within 1e-10 in the
rounding-equal order, fused on W; btf_factor(A).solve(b, trans=True) byte-equal to trans_oracle.btf_solve_trans; the
triangular plans shared with the list-level solves left as they were; condest() against the dense restatement; the
sharded path at world size 2."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import scipy.sparse as sp

import btf_oracle
import csparse_oracle as O
import synth
import tol
import trans_oracle as T
from conftest import ROOT, golden

pytestmark = pytest.mark.gpu


def cs():
    import csparse
    return csparse


def _fixture(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])
    p = g["C_p"].astype(np.int64)
    S = sp.coo_matrix(sp.csc_matrix((g["C_x"][:p[n]], g["C_i"][:p[n]], p), shape=(m, n))).tocsc()
    S.sum_duplicates()
    return S


def _cs(S):
    S = sp.csc_matrix(S)
    A = cs().cs_spalloc(S.shape[0], S.shape[1], max(S.nnz, 1), True, False)
    A.p, A.i, A.x = S.indptr.tolist(), S.indices.tolist(), S.data.tolist()
    return A


def _device(S):
    import _csx
    S = sp.csc_matrix(S)
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(S.shape[0], S.shape[1], _csx.pi(_csx.i32(S.indptr)), _csx.pi(_csx.i32(S.indices)),
                                         _csx.pd(_csx.f64(S.data)), h), "upload")
    return cs()._from_device(h, lambda nnz: max(nnz, 1))


def _lusol_oracle(F, b):
    N, Sy = F.factors, F.symbolic
    return np.asarray(T.lusol_trans(N.L, N.U, N.pinv, Sy.q, list(b)))


# ---------------------------------------------------------------------------------------------------- lusol --

@pytest.mark.parametrize("name", ["west0067", "fs_183_1"])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_lusol_trans_exact_order(name, order):
    c = cs()
    S = _fixture(name)
    n = S.shape[0]
    F = c.lusol_factor(_cs(S), order, 1.0, exact=True)
    assert F is not None
    rng = np.random.default_rng(order)
    b = rng.uniform(-1, 1, n)
    x = b.tolist()
    assert F.solve(x, trans=True) is True
    assert np.asarray(x).tobytes() == _lusol_oracle(F, b).tobytes()
    for k in (1, 7, 33, 64, 130):
        B = rng.uniform(-1, 1, (n, k))
        dB = c.dvec(B)
        assert F.solve(dB, trans=True) is True
        X = dB.numpy().reshape(n, k)
        for col in range(k):
            assert np.ascontiguousarray(X[:, col]).tobytes() == _lusol_oracle(F, B[:, col]).tobytes(), (k, col)


@pytest.mark.parametrize("name", ["west0067", "fs_183_1"])
@pytest.mark.parametrize("order", [0, 3])
def test_lusol_trans_default_order(name, order):
    """exact=None: a list exact, a block rounding-equal (1e-10 componentwise)"""
    c = cs()
    S = _fixture(name)
    n = S.shape[0]
    F = c.lusol_factor(_cs(S), order, 1.0)
    rng = np.random.default_rng(10 + order)
    b = rng.uniform(-1, 1, n)
    x = b.tolist()
    F.solve(x, trans=True)
    assert np.asarray(x).tobytes() == _lusol_oracle(F, b).tobytes()
    for k in (7, 64):
        B = rng.uniform(-1, 1, (n, k))
        dB = c.dvec(B)
        F.solve(dB, trans=True)
        X = dB.numpy().reshape(n, k)
        for col in range(k):
            assert tol.componentwise(X[:, col], _lusol_oracle(F, B[:, col])) <= 1e-10, (k, col)


def _w_matrix(nb):
    """W of test_gpu_configs: nb copies of west0067's pattern on the diagonal, block b scaled by 1 + 1e-3 u_b."""
    g = golden("west0067")
    bp, bi, bx = g["C_p"].astype(np.int64), g["C_i"].astype(np.int64), g["C_x"]
    bs = 67
    u = synth.vec(nb, 20240604, 0.0, 1.0)
    Ai = (bi[None, :] + (np.arange(nb) * bs)[:, None]).reshape(-1).astype(np.int32)
    Ax = (bx[None, :] * (1.0 + 1e-3 * u)[:, None]).reshape(-1)
    Ap = np.concatenate([[0], np.cumsum(np.tile(np.diff(bp), nb))]).astype(np.int32)
    return nb * bs, Ap, Ai, Ax


def _host_cs(n, Ap, Ai, Ax):
    A = cs().cs_spalloc(n, n, len(Ai), True, False)
    A.p, A.i, A.x = Ap.tolist(), Ai.tolist(), Ax.tolist()
    return A


def test_lusol_trans_on_W_1024_fused_both_orders():
    import c_oracle as CO
    c = cs()
    n, Ap, Ai, Ax = _w_matrix(1493)
    A = _host_cs(n, Ap, Ai, Ax)
    k = 1024
    b = 1.0 + np.arange(n) / n
    scales = 1.0 + 0.25 * np.arange(k)
    Fe = c.lusol_factor(A, 0, 1.0, exact=True)
    N = Fe.factors
    Lp, Li, Lx = (np.asarray(v) for v in (N.L.p, N.L.i, N.L.x))
    Up, Ui, Ux = (np.asarray(v) for v in (N.U.p, N.U.i, N.U.x))
    Lp, Li, Up, Ui = (v.astype(np.int32) for v in (Lp, Li, Up, Ui))
    q = Fe.symbolic.q
    dB = c.dvec(np.ascontiguousarray(b[:, None] * scales[None, :]))
    assert Fe.solve(dB, trans=True) is True
    assert Fe.last_fused
    Xe = dB.numpy().reshape(n, k)
    for r in (0, 1, 511, k - 1):
        y = CO.pvec(q, b * scales[r])
        y = CO.ltsolve(n, Lp, Li, Lx, CO.utsolve(n, Up, Ui, Ux, y))
        want = CO.pvec(np.asarray(N.pinv), y)
        assert np.ascontiguousarray(Xe[:, r]).tobytes() == want.tobytes(), r
    Fd = c.lusol_factor(A, 0, 1.0)
    dBd = c.dvec(np.ascontiguousarray(b[:, None] * scales[None, :]))
    assert Fd.solve(dBd, trans=True) is True
    assert Fd.last_fused
    Xd = dBd.numpy().reshape(n, k)
    for r in (0, 1, 511, k - 1):
        # normwise: the dense tile inverses of the rounding-equal order move components a million times smaller than the
        # largest by a few 1e-10 of themselves, forward and transposed alike
        assert tol.normwise(Xd[:, r], Xe[:, r]) <= 1e-12, r
    del dB, dBd, Xe, Xd
    # backward error of the transposed system, one column
    x = b.tolist()
    Fe.solve(x, trans=True)
    At = sp.csc_matrix((Ax, Ai, Ap), shape=(n, n)).T.tocsr()
    res = np.max(np.abs(At @ np.asarray(x) - b))
    assert res <= 1e-12 * (abs(At).sum(axis=1).max() * np.max(np.abs(x)) + np.max(np.abs(b)))


def test_shared_plans_stay_intact():
    """the U' / L' plans of a transposed solve are the ones cs_utsolve / cs_ltsolve use on the same factor: the order a
    transposed block solve sets is put back, and every solve gives the same bits before and after"""
    c = cs()
    n, Ap, Ai, Ax = _w_matrix(200)
    F = c.lusol_factor(_host_cs(n, Ap, Ai, Ax), 0, 1.0)
    L, U = F.factors.L, F.factors.U
    rng = np.random.default_rng(4)
    b = rng.uniform(-1, 1, n)
    B = rng.uniform(-1, 1, (n, 40))

    def run():
        out = []
        x = b.tolist()
        F.solve(x)
        out.append(np.asarray(x).tobytes())
        dB = c.dvec(B)
        F.solve(dB)
        out.append(dB.numpy().tobytes())
        for fn in (c.cs_lsolve, c.cs_usolve, c.cs_ltsolve, c.cs_utsolve):
            x = b.tolist()
            assert fn(L if fn in (c.cs_lsolve, c.cs_ltsolve) else U, x)
            out.append(np.asarray(x).tobytes())
            dX = c.dvec(B)
            fn(L if fn in (c.cs_lsolve, c.cs_ltsolve) else U, dX)
            out.append(dX.numpy().tobytes())
        return out

    before = run()
    dB = c.dvec(B)
    F.solve(dB, trans=True)                  # rounding-equal: sets the U' / L' plans' order, then puts it back
    assert F.last_fused
    x = b.tolist()
    F.solve(x, trans=True)
    after = run()
    assert before == after
    for fn, M in ((c.cs_utsolve, U), (c.cs_ltsolve, L)):      # and the exact list solves match the oracle's functions
        y = b.tolist()
        fn(M, y)
        z = b.tolist()
        getattr(O, fn.__name__)(T._M(M), z)
        assert np.asarray(y).tobytes() == np.asarray(z).tobytes()


# ------------------------------------------------------------------------------------------------------ btf --

def _btf_oracle(sol, b):
    f = sol.factors
    return np.asarray(T.btf_solve_trans(f.L, f.U, f.F, f.pinv, f.p, f.q, f.r, list(b)))


def _btf_check(S, widths, seed=1):
    """trans x byte-equal to the oracle; every column of a block byte-equal to the list solve of that column; reruns equal"""
    c = cs()
    n = S.shape[0]
    sol = c.btf_factor(_cs(S))
    assert sol is not None
    rng = np.random.default_rng(seed)
    b = rng.uniform(-1, 1, n)
    x = b.tolist()
    assert sol.solve(x, trans=True) is True
    x = np.asarray(x)
    assert x.tobytes() == _btf_oracle(sol, b).tobytes()
    for k in widths:
        B = rng.uniform(-1, 1, (n, k))
        dB = c.dvec(B)
        assert sol.solve(dB, trans=True) is True
        X = dB.numpy().reshape(n, k)
        for col in range(k):
            xc = B[:, col].tolist()
            sol.solve(xc, trans=True)
            assert np.asarray(xc).tobytes() == X[:, col].tobytes(), (k, col)
        dB2 = c.dvec(B)
        sol.solve(dB2, trans=True)
        assert dB2.numpy().reshape(n, k).tobytes() == X.tobytes()
    # the forward solve is untouched by the transposed one's programs
    y = b.tolist()
    sol.solve(y)
    assert np.asarray(y).tobytes() == np.asarray(btf_oracle.solve(sol.factors.L, sol.factors.U, sol.factors.F,
                                                                  sol.factors.pinv, sol.factors.p, sol.factors.q,
                                                                  sol.factors.r, list(b))).tobytes()
    return sol


@pytest.mark.parametrize("name", ["fs_183_1", "west0067", "bcsstk16"])
def test_btf_trans_fixture_exact(name):
    _btf_check(_fixture(name), (1, 7, 64, 65, 130) if name != "bcsstk16" else (1, 7, 65))


def test_btf_trans_generated_exact():
    S, blocks, depth = btf_oracle.reducible(btf_oracle.block_sizes(3000, 12), 9, 12)
    sol = _btf_check(S, (1, 64, 65, 130))
    assert sol.info()["blocks"] == len(blocks) and sol.info()["levels"] == depth


def test_btf_trans_with_a_large_block():
    S, blocks, depth = btf_oracle.reducible(btf_oracle.block_sizes(4000, 7, big=(300,)), 6, 7)
    sol = _btf_check(S, (1, 64, 65))
    assert sol.info()["large_blocks"] == 1 and sol.info()["max_block"] == 300


def test_btf_trans_chain_of_2x2_blocks_natural_order():
    nbk = 2000
    n = 2 * nbk
    rows, cols, vals = [], [], []
    for k in range(nbk):
        a = 2 * k
        rows += [a, a + 1, a, a + 1]
        cols += [a, a, a + 1, a + 1]
        vals += [4.0, 1.0, 1.0, 5.0]
        if k:
            rows.append(a)
            cols.append(a - 1)
            vals.append(-1.0)
    sol = _btf_check(sp.csc_matrix((vals, (rows, cols)), shape=(n, n)), (1, 3, 64))
    assert sol.info()["levels"] == nbk


def test_btf_trans_after_the_factors_were_read():
    """the programs are made from the factors on the first transposed solve: reading .L / .U / .F to host lists before it
    changes nothing"""
    S, _, _ = btf_oracle.reducible(btf_oracle.block_sizes(2000, 3), 5, 3)
    sol = cs().btf_factor(_device(S))
    f = sol.factors
    _ = (f.L.p, f.U.x, f.F.i)
    b = np.linspace(-1, 1, S.shape[0])
    x = b.tolist()
    sol.solve(x, trans=True)
    assert np.asarray(x).tobytes() == _btf_oracle(sol, b).tobytes()


def test_btf_trans_scale_1m_128_rhs():
    c = cs()
    sizes = btf_oracle.block_sizes(1_000_000, 11)
    S, blocks, depth = btf_oracle.reducible(sizes, 8, 11)
    n = S.shape[0]
    sol = c.btf_factor(_device(S))
    assert sol is not None
    k = 128
    B = np.random.default_rng(3).uniform(-1, 1, (n, k))
    dB = c.dvec(B)
    assert sol.solve(dB, trans=True)
    X = dB.numpy().reshape(n, k)
    At = S.T.tocsr()
    nA = abs(At).sum(axis=1).max()
    for c0 in range(0, k, 16):
        R = At @ X[:, c0:c0 + 16] - B[:, c0:c0 + 16]
        for j in range(R.shape[1]):
            x = X[:, c0 + j]
            res = np.max(np.abs(R[:, j]))
            assert res / (nA * np.max(np.abs(x)) + np.max(np.abs(B[:, c0 + j]))) < 1e-13, c0 + j


# -------------------------------------------------------------------------------------------------- condest --

def _condest_cases():
    S1, _, _ = btf_oracle.reducible(btf_oracle.block_sizes(400, 21), 5, 21)
    return [("west0067", _fixture("west0067")), ("reducible400", sp.csc_matrix(S1))]


@pytest.mark.parametrize("case", [0, 1])
def test_condest_both_solvers(case):
    c = cs()
    name, S = _condest_cases()[case]
    want = T.condest_dense(S)
    for make in (lambda: c.lusol_factor(_cs(S), 0, 1.0), lambda: c.btf_factor(_cs(S))):
        sol = make()
        e1, e2 = sol.condest(), sol.condest()
        assert e1 == e2, name
        assert abs(e1 - want) <= 1e-10 * want, (name, e1, want)
    c3 = c.lusol_factor(_cs(S), 3, 1.0).condest()
    assert abs(c3 - want) <= 1e-10 * want, (name, c3, want)


def test_condest_of_one_by_one():
    c = cs()
    A = c.cs_spalloc(1, 1, 1, True, False)
    A.p, A.i, A.x = [0, 1], [0], [-4.0]
    assert c.lusol_factor(A).condest() == 1.0
    assert c.btf_factor(A).condest() == 1.0


# -------------------------------------------------------------------------------------------------- sharded --

TWO_RANKS = textwrap.dedent("""
    import os, sys, json
    import numpy as np
    sys.path[:0] = [os.path.join(r"{root}", "csparse.py_amd"), os.path.join(r"{root}", "oracle"),
                    os.path.join(r"{root}", "tests")]
    import shard, synth, _csx
    import csparse as cs
    import trans_oracle as T
    from conftest import golden, unpack
    comm = shard.Comm(backend="gloo")        # two ranks, one device: the host stand-in carries the exchange
    _csx.init(0)
    rank = comm.rank
    out = dict(rank=rank)
    K = 5
    W = cs.cs_pin(unpack(cs, golden("west0067"), "C"))
    n = W.n
    F = cs.lusol_factor(W, 3, 1.0, exact=True)
    B = synth.rhs(n, K, 7)
    dB = cs.dvec(B) if rank == 0 else None
    assert F.solve(dB, comm=comm, nrhs=K, trans=True)
    if rank == 0:
        X = dB.numpy().reshape(n, K)
        N, S = F.factors, F.symbolic
        out["ok"] = all(np.ascontiguousarray(X[:, r]).tobytes()
                        == np.asarray(T.lusol_trans(N.L, N.U, N.pinv, S.q, B[:, r].tolist())).tobytes() for r in range(K))
    print("RESULT " + json.dumps(out))
    comm.close()
""")


def _env(**kw):
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "CSX_FORCE_DIST", "CSX_COMM_BACKEND"):
        e.pop(k, None)
    e.update(kw)
    return e


def test_lusol_trans_sharded_world_two(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(TWO_RANKS.format(root=ROOT))
    procs = [subprocess.Popen([sys.executable, str(script)],
                              env=_env(RANK=str(rk), LOCAL_RANK=str(rk), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                                       MASTER_PORT="29731", CSX_SINGLE_DEVICE="1", CSX_COMM_BACKEND="gloo"),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for rk in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=600))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, se[-3000:]
    res = {d["rank"]: d for d in (json.loads([l for l in so.splitlines() if l.startswith("RESULT ")][0][7:])
                                  for so, _ in outs)}
    assert res[0]["ok"] is True
