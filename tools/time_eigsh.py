#!/usr/bin/env python3
"""eigsh() on the 300 x 300 grid, and the three csx_bgs_* kernels alone beside the csx_gs_* kernels of §28.

    python tools/time_eigsh.py [--reps 3] [--only kernels,eigsh] [--rows 5000000] [--out FILE]

kernels: csx_bgs_gram / update / combine at --rows x 8 and --rows x 32 (b = q) with nv = 1, 8, 17 basis blocks, hipEvent-timed
(median of --reps after one warm call), as GB/s on their algorithmic bytes with B = 8 rows b: gram (nv + ceil(nv / BGS_GROUP)) B,
update (nv + 2) B, combine (nv + 1) B; and in the same run csx_gs_project / update / combine on blocks of the same byte count
(nrhs = b).  A call's time includes its staging copy and, for gram / project / gs update, the download of the sums.
eigsh: nev = 8 on the five-point Laplacian K of the 300 x 300 grid at order 1, M = None: cholsol_factor(K) with sigma = 0 and
ldlsol_factor(K - 3.7 I) with sigma = 3.7; wall clock to a synchronise (median of --reps after one warm run), and from one more
run with a synchronise around every call the split into solves, products (the residual kernel: M products and the
verification), kernels (csx_bgs_* and csx_gs_*) and host (the rest: the dense steps, copies, Python).
One JSON line per case on stdout and in --out (default profiles/eigsh_time.jsonl).  Nothing here is a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402
from time_gmres import grid_upper  # noqa: E402
from time_refine import event_ms, lib, wall  # noqa: E402

KERNELS = ("csx_bgs_gram", "csx_bgs_update", "csx_bgs_combine", "csx_gs_project", "csx_gs_scale")


def kernel_cases(rows, reps, emit):
    most = 17
    L, G = _csx.bgs_limits(), _csx.gmres_limits()
    for b in (8, 32):
        B = 8 * rows * b
        V = cs.dvec(rows * b * most)
        V.fill(2.0 ** -10)
        W, U = cs.dvec(rows, b), cs.dvec(rows, b)
        W.fill(1.0)
        work = cs.dvec(max(_csx.bgs_work_len(rows, b, b, most), _csx.gs_work_len(rows, b, most)))
        pm = _csx.pi(_csx.i32(np.ones(b)))
        for nv in (1, 8, most):
            H, h, nrm2 = np.full((nv, b, b), 2.0 ** -20), np.full((nv, b), 2.0 ** -20), np.zeros(b)
            ln = _csx.i32(np.full(b, nv))
            calls = {
                "bgs_gram": (lambda: lib().csx_bgs_gram(V.handle, nv, b, W.handle, b, work.handle, rows, 0, _csx.pd(np.empty((nv, b, b)))),
                             (nv + -(-nv // L["BGS_GROUP"])) * B),
                "bgs_update": (lambda: lib().csx_bgs_update(V.handle, nv, b, W.handle, b, work.handle, rows, _csx.pd(H)), (nv + 2) * B),
                "bgs_combine": (lambda: lib().csx_bgs_combine(V.handle, nv, b, U.handle, b, work.handle, rows, _csx.pd(H)), (nv + 1) * B),
                "gs_project": (lambda: lib().csx_gs_project(V.handle, nv, W.handle, work.handle, rows, b, pm, 0, _csx.pd(np.empty((nv, b)))),
                               (nv + -(-nv // G["GS_GROUP"])) * B),
                "gs_update": (lambda: lib().csx_gs_update(V.handle, nv, W.handle, work.handle, rows, b, pm, 0, _csx.pd(h), _csx.pd(nrm2)),
                              (nv + 2) * B),
                "gs_combine": (lambda: lib().csx_gs_combine(V.handle, nv, U.handle, work.handle, rows, b, pm, _csx.pd(h), _csx.pi(ln)),
                               (nv + 1) * B),
            }
            for name, (fn, nbytes) in calls.items():
                t = []
                for rep in range(reps + 1):
                    t.append(event_ms(lambda: _csx.check(fn(), name)))
                ms = float(np.median(t[1:]))
                emit({"case": "kernel", "kernel": name, "rows": rows, "b": b, "q": b, "nv": nv, "reps": reps, "ms": round(ms, 3),
                      "algorithmic_bytes": nbytes, "GBs": round(nbytes / (ms * 1e-3) / 1e9, 1)})
        del V, W, U, work
        lib().csx_mem_trim()


def split_run(F, run):
    """one run with a synchronise around every solve, residual call and kernel call: milliseconds per kind, the rest is host"""
    spent = {"solves": 0.0, "products": 0.0, "kernels": 0.0}

    def timed(kind, fn):
        def call(*args):
            _csx.sync()
            t0 = time.perf_counter()
            out = fn(*args)
            _csx.sync()
            spent[kind] += 1e3 * (time.perf_counter() - t0)
            return out
        return call

    L = lib()
    kept = {name: getattr(L, name) for name in KERNELS}
    F._solve_block = timed("solves", F._solve_block)
    F._residual_into = timed("products", type(F)._residual_into)
    for name, fn in kept.items():
        setattr(L, name, timed("kernels", fn))
    try:
        _, total = wall(run)
    finally:
        for name, fn in kept.items():
            setattr(L, name, fn)
        del F._solve_block, F._residual_into
    spent["host"] = total - sum(spent.values())
    return {k + "_ms": round(v, 3) for k, v in spent.items()}, round(total, 3)


def eigsh_cases(reps, emit):
    g, nev = 300, 8
    n = g * g
    for solver, sigma in (("cholsol_factor", 0.0), ("ldlsol_factor", 3.7)):
        A = cs.cs_pin(grid_upper(g, np.arange(n), -sigma))
        F = getattr(cs, solver)(A, 1)
        if F is None:
            emit({"case": "eigsh", "solver": solver, "grid": g, "sigma": sigma, "factor": None})
            continue

        def run():
            return F.eigsh(nev, sigma=sigma)

        t, out = [], None
        for rep in range(reps + 1):
            out, ms = wall(run)
            t.append(ms)
        row = {"case": "eigsh", "solver": solver, "grid": g, "order": 1, "sigma": sigma, "nev": nev, "reps": reps,
               "ms": round(float(np.median(t[1:])), 3), "blocks": int(out["blocks"]), "solves": int(out["solves"]),
               "products": int(out["products"]), "converged": bool(out["converged"].all()), "resid_max": float(out["resid"].max()),
               "values": [float(v) for v in out["values"]]}
        if "below" in out:
            row["below"] = out["below"]
        split, total = split_run(F, run)
        row.update(split)
        row["split_run_ms"] = total
        emit(row)
        del F, A
        lib().csx_mem_trim()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="kernels,eigsh")
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eigsh_time.jsonl"))
    a = ap.parse_args()
    _csx.init(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if "eigsh" in a.only.split(","):
        eigsh_cases(a.reps, emit)
    if "kernels" in a.only.split(","):
        kernel_cases(a.rows, a.reps, emit)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
