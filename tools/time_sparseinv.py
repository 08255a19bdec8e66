#!/usr/bin/env python3
"""Times of sparseinv (csx_chol_inverse) beside the only route to entries of the inverse without it: solve() of
identity blocks of 128 columns.

    python tools/time_sparseinv.py [--reps 5] [--only gspd64,gspd32,ragged,trees24,bcsstk16_0,bcsstk16_1,grid,tridiag] [--out FILE]

Cases: G-spd at 5M rows (config 5's matrix, 78 125 dense blocks of 64; and 156 250 blocks of 32), ragged cliques of 8 .. 64
columns at 5M rows, 200 000 sparse trees of 24 columns, bcsstk16 at order 0 (nearly a chain) and order 1, the 300 x 300 grid
Laplacian at order 1, a tridiagonal matrix of 200 000 rows (one column per depth).  Per case: depths, terms, the call (wall
median of --reps calls after one warm-up; every call ends with a download of its flag, so it is synchronised) and its launches
between two events, the algorithmic bytes (20 lnz read + 8 lnz written + the two pointer arrays) over the event time as a
share of 8 TB/s; and in the same process cholsol_factor(...).solve of a block of 128 unit vectors (rounding-equal order, the
solver's default for blocks; events around the solve alone): every block on bcsstk16 and the grid, ONE block times the number
of blocks ("unit_blocks_timed": 1) on the 5M-row cases and the tridiagonal.  bcsstk16 and the tridiagonal also with
"sparseinv.walk" = 0 (one launch per depth: the nowalk_* fields).  One JSON line per case on stdout and in --out (default
profiles/sparseinv_time.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402

PEAK = 8e12   # bytes / s
NRHS = 128


def lib():
    return _csx.lib()


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def dev_matrix(n, p, i, x):
    h = _csx.new_handle()
    p, i, x = np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64)
    _csx.check(lib().csx_csc_upload(n, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), h), "csx_csc_upload")
    A = cs._from_device(h, lambda z: max(z, 1))
    A._pinned = True
    return A


def inverse_times(L, reps):
    wall, kern, info = [], [], None
    for r in range(reps + 1):
        Z = cs.sparseinv(L)
        info = cs.sparseinv_info()
        del Z
        if r:
            wall.append(info["wall_ms"])
            kern.append(info["kernel_ms"])
    return float(np.median(wall)), float(np.median(kern)), info


def unit_block_ms(F, n, B, first):
    """solve() of columns [first, first + NRHS) of the identity (B: an n-by-NRHS dvec), events around the solve alone"""
    B.fill(0.0)
    rows = min(NRHS, n - first)
    eye = np.zeros((rows, NRHS))
    eye[np.arange(rows), np.arange(rows)] = 1.0
    h = _csx.new_handle()
    _csx.check(lib().csx_vec_wrap(C.c_void_p(B.device_ptr() + 8 * first * NRHS), rows * NRHS, h), "csx_vec_wrap")
    _csx.check(lib().csx_vec_write(h, _csx.pd(eye), eye.size), "csx_vec_write")
    _csx.free(h)
    with _csx.Timer() as t:
        F.solve(B)
    return t.ms


def run_case(name, A, order, reps, out, all_blocks, extra=None):
    n = A.n
    F = cs.cholsol_factor(A, order=order)
    assert F is not None
    _, _, lnz, _ = F.L._dev.info()
    wall, kern, info = inverse_times(F.L, reps)
    nbytes = 28 * lnz + 8 * (n + 1)
    rec = {"case": name, "order": order, "n": n, "lnz": lnz, "depths": info["depths"], "widest": info["widest"],
           "terms": info["terms"], "call_ms": wall, "kernel_ms": kern, "bytes": nbytes,
           "share_of_peak": nbytes / (kern * 1e-3) / PEAK}
    if extra:
        rec.update(extra(F))
    B = cs.dvec(n, NRHS)
    nblocks = (n + NRHS - 1) // NRHS
    unit_block_ms(F, n, B, 0)                                      # warm-up: plans of the block order are built here
    if all_blocks:
        total = sum(unit_block_ms(F, n, B, b * NRHS) for b in range(nblocks))
        timed = nblocks
    else:
        one = float(np.median([unit_block_ms(F, n, B, (nblocks // 2) * NRHS) for _ in range(reps)]))
        total, timed = one * nblocks, 1
    rec.update({"unit_route_ms": total, "unit_blocks": nblocks, "unit_blocks_timed": timed, "speedup": total / wall})
    emit(rec, out)


def no_walk(reps):
    def f(F):
        with _csx.option("sparseinv.walk", 0):
            wall, kern, _ = inverse_times(F.L, reps)
        return {"nowalk_call_ms": wall, "nowalk_kernel_ms": kern}
    return f


def gen_gspd(nb, bs):
    h = _csx.new_handle()
    _csx.check(lib().csx_gen_gspd(nb, bs, 20240601 + 5, h), "csx_gen_gspd")
    A = cs._from_device(h, lambda z: max(z, 1))
    A._pinned = True
    return A


def arrow_trees(nb, bs):
    """nb blocks of bs columns, tridiagonal plus a full last row / column (tools/time_forest_sparse.py's matrix)"""
    cols = []
    for c in range(bs):
        rows = {c, bs - 1} | ({c - 1} if c > 0 else set()) | ({c + 1} if c + 1 < bs else set())
        cols.append(sorted(range(bs)) if c == bs - 1 else sorted(rows))
    bi = np.concatenate([np.asarray(r, np.int64) for r in cols])
    bp = np.concatenate([[0], np.cumsum([len(r) for r in cols])])
    bx = np.concatenate([[(8.0 + (c % 5)) if r == c else -1.0 / (1 + abs(r - c)) for r in cols[c]] for c in range(bs)])
    Ap = np.concatenate([(np.arange(nb)[:, None] * bp[-1] + bp[None, :-1]).reshape(-1), [nb * bp[-1]]]).astype(np.int32)
    Ai = (bi[None, :] + (np.arange(nb) * bs)[:, None]).reshape(-1).astype(np.int32)
    return Ap, Ai, np.tile(bx, nb)


def bcsstk16():
    from conftest import golden
    g = golden("bcsstk16")
    p = np.asarray(g["C_p"])
    return len(p) - 1, p, np.asarray(g["C_i"])[:p[-1]], np.asarray(g["C_x"])[:p[-1]]


def grid(gx, gy):
    Tx = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gx, gx))
    Ty = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(gy, gy))
    A = (sp.kron(sp.identity(gy), Tx) + sp.kron(Ty, sp.identity(gx)) + 0.5 * sp.identity(gx * gy)).tocsc()
    A.sort_indices()
    return A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="gspd64,gspd32,ragged,trees24,bcsstk16_0,bcsstk16_1,grid,tridiag")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparseinv_time.jsonl"))
    a = ap.parse_args()
    _csx.init(0)
    with open(a.out, "w") as out:
        for name in a.only.split(","):
            if name == "gspd64":
                run_case("gspd_5m_blocks_of_64", gen_gspd(78125, 64), 0, a.reps, out, False)
            elif name == "gspd32":
                run_case("gspd_5m_blocks_of_32", gen_gspd(156250, 32), 0, a.reps, out, False)
            elif name == "ragged":
                import synth
                n, p, i, x, _ = synth.ragged_cliques(5000000, 8, 64, 9)
                run_case("ragged_cliques_5m", dev_matrix(n, p, i, x), 0, a.reps, out, False)
            elif name == "trees24":
                p, i, x = arrow_trees(200000, 24)
                run_case("sparse_trees_200000_of_24", dev_matrix(len(p) - 1, p, i, x), 0, a.reps, out, False)
            elif name in ("bcsstk16_0", "bcsstk16_1"):
                n, p, i, x = bcsstk16()
                run_case("bcsstk16", dev_matrix(n, p, i, x), int(name[-1]), a.reps, out, True, no_walk(a.reps))
            elif name == "grid":
                M = grid(300, 300)
                run_case("grid300", dev_matrix(M.shape[0], M.indptr, M.indices, M.data), 1, a.reps, out, True)
            elif name == "tridiag":
                n = 200000
                rng = np.random.default_rng(4)
                o = rng.uniform(-1.0, 1.0, n - 1)
                M = sp.diags([o, rng.uniform(2.5, 3.5, n), o], [-1, 0, 1], shape=(n, n)).tocsc()
                M.sort_indices()
                run_case("tridiagonal_200000", dev_matrix(n, M.indptr, M.indices, M.data), 0, a.reps, out, False, no_walk(a.reps))
            else:
                raise SystemExit("unknown case " + name)
            _csx.check(lib().csx_mem_trim(), "csx_mem_trim")


if __name__ == "__main__":
    main()
