#!/usr/bin/env python3
"""Times of updown_block (csx_updown_block) beside the loop of rank-1 csx_updown calls it stands for.

    python tools/time_updown_block.py [--reps 5] [--only bcsstk16,gspd,grid] [--out FILE]

bcsstk16 (natural order): k = 1, 8, 64, 256 columns, each f and 7 rows of L(:, f), all updates, against k csx_updown calls
given parent already as an int32 array.  G-spd at 5M rows (config 5's matrix: 78 125 dense blocks of 64): one block per column,
8 rows each, k = 64 and 1 024; the loop at k = 64.  300 x 300 grid Laplacian, order 1, k = 64: cholsol_factor.update(C) and
the first list solve after it, against a fresh cholsol_factor(A + C C') and its first solve.  Wall medians (every call
synchronises) of --reps calls after one warm-up, the block call and the loop alternated in one process; kernel_ms is the block
kernels' hipEvent time from csx_updown_block_info.  One JSON line per case on stdout and in --out (default
profiles/updown_block_time.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402


def lib():
    return _csx.lib()


def columns(Lp, Li, fs, rows, seed, scale):
    rng = np.random.default_rng(seed)
    p, i, x = [0], [], []
    for f in fs:
        pat = Li[Lp[f]:Lp[f + 1]]
        r = [int(f)] + [int(v) for v in rng.choice(pat[1:], size=min(len(pat) - 1, rows - 1), replace=False)] if len(pat) > 1 \
            else [int(f)]
        i += r
        x += (scale * rng.uniform(0.5, 1.0, len(r))).tolist()
        p.append(len(i))
    return np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x)


def upload(m, n, p, i, x):
    h = _csx.new_handle()
    _csx.check(lib().csx_csc_upload(m, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), h), "csx_csc_upload")
    return h


def block_call(hL, hC, k):
    sg = np.ones(k, np.int32)
    out = C.c_int32(0)
    t0 = time.perf_counter()
    _csx.check(lib().csx_updown_block(hL, hC, _csx.pi(sg), None, 0, out), "csx_updown_block")
    wall = 1e3 * (time.perf_counter() - t0)
    assert out.value == k, out.value
    ch, uc, gr, ms = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    _csx.check(lib().csx_updown_block_info(ch, uc, gr, ms), "csx_updown_block_info")
    return wall, {"chunks": ch.value, "union_columns": uc.value, "groups": gr.value, "kernel_ms": ms.value}


def loop_call(hL, Cp, Ci, Cx, parent):
    ok = C.c_int(0)
    t0 = time.perf_counter()
    for t in range(len(Cp) - 1):
        a, b = int(Cp[t]), int(Cp[t + 1])
        ci, cx = np.ascontiguousarray(Ci[a:b]), np.ascontiguousarray(Cx[a:b])
        _csx.check(lib().csx_updown(hL, 1, b - a, _csx.pi(ci), _csx.pd(cx), _csx.pi(parent), ok), "csx_updown")
        assert ok.value == 1
    return 1e3 * (time.perf_counter() - t0)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def compare(case, k, hL, Cp, Ci, Cx, parent, reps, with_loop, out, extra=None):
    n = len(parent)
    hC = upload(n, k, Cp, Ci, Cx)
    block_call(hL, hC, k)
    if with_loop:
        loop_call(hL, Cp, Ci, Cx, parent)
    bw, lw, info = [], [], None
    for _ in range(reps):
        w, info = block_call(hL, hC, k)
        bw.append(w)
        if with_loop:
            lw.append(loop_call(hL, Cp, Ci, Cx, parent))
    _csx.free(hC)
    rec = {"case": case, "k": k, "block_ms": float(np.median(bw)), "block_min_ms": float(min(bw)), **info}
    if with_loop:
        rec["loop_ms"] = float(np.median(lw))
        rec["speedup"] = rec["loop_ms"] / rec["block_ms"]
    rec.update(extra or {})
    emit(rec, out)


def case_bcsstk16(reps, out):
    from conftest import golden, unpack
    A = cs.cs_pin(unpack(cs, golden("bcsstk16"), "C"))
    N = cs.cs_chol(A, cs.cs_schol(0, A))
    hL = N.L._dev.handle
    m, n, nnz, _ = N.L._dev.info()
    Lp, Li = np.empty(n + 1, np.int32), np.empty(nnz, np.int32)
    _csx.check(lib().csx_csc_download(hL, _csx.pi(Lp), _csx.pi(Li), None), "csx_csc_download")
    parent = np.where(np.diff(Lp) > 1, Li[np.minimum(Lp[:-1] + 1, nnz - 1)], -1).astype(np.int32)
    for k in (1, 8, 64, 256):
        fs = np.random.default_rng(k).integers(0, n, k)
        Cp, Ci, Cx = columns(Lp, Li, fs, 8, k, 1e-3)
        compare("bcsstk16", k, hL, Cp, Ci, Cx, parent, reps, True, out, {"n": n})


def case_gspd(reps, out):
    nb, bs = 78125, 64
    hA = _csx.new_handle()
    _csx.check(lib().csx_gen_gspd(nb, bs, 5, hA), "csx_gen_gspd")
    hL, hP = _csx.new_handle(), _csx.new_handle()
    _csx.check(lib().csx_cholsol_factor(hA, 1, hL, hP), "csx_cholsol_factor")
    _csx.free(hP)
    _csx.free(hA)
    n = nb * bs
    # L of dense blocks: column j holds rows j .. the end of its block; parent[j] = j + 1 inside a block
    j = np.arange(n)
    parent = np.where(j % bs == bs - 1, -1, j + 1).astype(np.int32)
    for k in (64, 1024):
        rng = np.random.default_rng(k)
        blocks = rng.choice(nb, size=k, replace=False)
        f = blocks * bs + rng.integers(0, bs - 8, k)
        Cp = np.arange(k + 1, dtype=np.int32) * 8
        Ci = (f[:, None] + np.arange(8)[None, :]).reshape(-1).astype(np.int32)   # f and the 7 rows after it, in its block
        Cx = 1e-3 * rng.uniform(0.5, 1.0, 8 * k)
        compare("gspd_5M", k, hL, Cp, Ci, Cx, parent, reps, k == 64, out, {"n": n})
    _csx.free(hL)


def case_grid(reps, out):
    import scipy.sparse as sp
    g = 300
    T = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(g, g))
    Asp = (sp.kron(sp.identity(g), T) + sp.kron(T, sp.identity(g)) + 0.01 * sp.identity(g * g)).tocsc()
    Asp.sort_indices()
    n = g * g

    def mk(M):
        A = cs.cs_spalloc(n, n, M.nnz, True, False)
        A.p, A.i, A.x = M.indptr.tolist(), M.indices.tolist(), M.data.tolist()
        return cs.cs_pin(A)

    A = mk(Asp)
    b = np.random.default_rng(1).uniform(0.5, 1.5, n)
    F = cs.cholsol_factor(A, order=1)
    pinv = np.asarray(F.symbolic.pinv)
    perm = np.empty(n, np.int64)
    perm[pinv] = np.arange(n)
    m, _, nnz, _ = F.L._dev.info()
    Lp, Li = np.empty(n + 1, np.int32), np.empty(nnz, np.int32)
    _csx.check(lib().csx_csc_download(F.L._dev.handle, _csx.pi(Lp), _csx.pi(Li), None), "csx_csc_download")
    k = 64
    Cp, CiL, Cx = columns(Lp, Li, np.random.default_rng(3).integers(0, n, k), 8, 3, 0.1)
    Ci = perm[CiL].astype(np.int32)
    Cm = cs.cs_spalloc(n, k, len(Ci), True, False)
    Cm.p, Cm.i, Cm.x = Cp.tolist(), Ci.tolist(), Cx.tolist()
    Csp = sp.csc_matrix((Cx, Ci, Cp), shape=(n, k))
    A2 = (Asp + Csp @ Csp.T).tocsc()
    A2.sort_indices()
    A2c = mk(A2)
    F.solve(b.tolist())
    up, fresh, info = [], [], None
    for r in range(reps + 1):
        t0 = time.perf_counter()
        assert F.update(Cm)
        xs = b.tolist()
        F.solve(xs)
        t1 = time.perf_counter()
        info = F.updown_info()
        assert F.downdate(Cm)
        F.solve(b.tolist())
        t2 = time.perf_counter()
        F2 = cs.cholsol_factor(A2c, order=1)
        F2.solve(b.tolist())
        t3 = time.perf_counter()
        del F2
        if r:
            up.append(1e3 * (t1 - t0))
            fresh.append(1e3 * (t3 - t2))
    emit({"case": "grid300_order1", "k": k, "n": n, "update_and_solve_ms": float(np.median(up)),
          "fresh_factor_and_solve_ms": float(np.median(fresh)), "update_kernel_ms": info["kernel_ms"],
          "update_wall_ms": info["wall_ms"], "chunks": info["chunks"], "union_columns": info["union_columns"]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="bcsstk16,gspd,grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "updown_block_time.jsonl"))
    a = ap.parse_args()
    _csx.init(0)
    with open(a.out, "w") as out:
        for name in a.only.split(","):
            {"bcsstk16": case_bcsstk16, "gspd": case_gspd, "grid": case_grid}[name](a.reps, out)


if __name__ == "__main__":
    main()
