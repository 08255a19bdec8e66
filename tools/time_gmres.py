#!/usr/bin/env python3
"""gmres() against refine() and against refactor-then-solve, and the four csx_gs_* kernels alone.

    python tools/time_gmres.py [--reps 3] [--only stale,kernels] [--rows 5000000] [--out FILE]

stale: cholsol_factor of the 300 x 300 grid Laplacian K at order 1; the matrix to solve is A = K + 50 sum e_i e_i' at 8 nodes.
At k = 1, 8, 128: gmres(b, A=A) on the stale factor, refine(b, A=A) on it, and refactor(A) followed by solve(b), wall clock to
a synchronise (median of --reps after one warm run), with omega and the step counts of each.  The ratios are reported, not
promised.
kernels: csx_gs_project / update / scale / combine at --rows x 128 columns with nv = 1, 8, 17 basis blocks, hipEvent-timed
(median of --reps after one warm call), as GB/s on their algorithmic bytes N = 8 rows nrhs: project (nv + ceil(nv / GS_GROUP)) N,
update (nv + 2) N, scale 2 N, combine (nv + 1) N.  A call's time includes its staging copy and, for project and update, the small
download of the sums.
One JSON line per case on stdout and in --out (default profiles/gmres_time.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402
from time_refine import event_ms, lib, wall  # noqa: E402

EPS = 2.0 ** -52


def grid_upper(g, bumped=(), sigma=0.0):
    """the upper triangle of the five-point Laplacian of a g x g grid as a `cs`, `sigma` added on the diagonal at the nodes given"""
    n = g * g
    j = np.arange(n)
    north, west = j >= g, j % g != 0
    counts = 1 + north.astype(np.int64) + west.astype(np.int64)
    p = np.concatenate(([0], np.cumsum(counts)))
    i, x = np.empty(p[-1], np.int64), np.empty(p[-1])
    at = p[:-1].copy()
    i[at[north]], x[at[north]] = j[north] - g, -1.0
    at[north] += 1
    i[at[west]], x[at[west]] = j[west] - 1, -1.0
    at[west] += 1
    i[at], x[at] = j, 4.0
    x[at[np.asarray(bumped, dtype=np.int64)]] += sigma
    A = cs.cs_spalloc(n, n, int(p[-1]), True, False)
    A.p, A.i, A.x = p.tolist(), i.tolist(), x.tolist()
    return A


def stale_cases(reps, emit):
    g, r, sigma = 300, 8, 50.0
    n = g * g
    nodes = [(g + 1) * (g // (r + 1)) * (t + 1) for t in range(r)]
    K, A = grid_upper(g), cs.cs_pin(grid_upper(g, nodes, sigma))
    F = cs.cholsol_factor(K, 1)
    for k in (1, 8, 128):
        B = np.random.default_rng(k).uniform(-1.0, 1.0, (n, k))
        times = {"gmres": [], "refine": [], "refactor_solve": []}
        outs = {}
        for rep in range(reps + 1):
            outs["gmres"], ms = wall(lambda: F.gmres(cs.dvec(B), A=A))
            times["gmres"].append(ms)
            outs["refine"], ms = wall(lambda: F.refine(cs.dvec(B), A=A))
            times["refine"].append(ms)

            def again():
                assert F.refactor(A) is True
                d = cs.dvec(B)
                F.solve(d)
                w = F.backward_error(d, cs.dvec(B))
                assert F.refactor(K) is True           # back to the stale factor (not timed apart: halve for one refactor)
                return w
            outs["refactor_solve"], ms = wall(again)
            times["refactor_solve"].append(ms)
        row = {"case": "stale_cholsol", "grid": g, "order": 1, "bumped": r, "sigma": sigma, "k": k, "reps": reps}
        for f, t in times.items():
            row[f + "_ms"] = round(float(np.median(t[1:])), 3)
        row["refactor_solve_note"] = "two refactors, one solve and one backward error"
        row["gmres_omega_max_over_eps"] = float(np.max(outs["gmres"]["omega"]) / EPS)
        row["gmres_iters_max"], row["gmres_solves"] = int(outs["gmres"]["iters"].max()), int(outs["gmres"]["solves"])
        row["refine_omega_max_over_eps"] = float(np.max(outs["refine"]["omega"]) / EPS)
        row["refine_steps_max"] = int(outs["refine"]["steps"].max())
        row["refactor_solve_omega_max_over_eps"] = float(np.max(outs["refactor_solve"]) / EPS)
        row["gmres_over_refactor_solve"] = round(row["gmres_ms"] / row["refactor_solve_ms"], 3)
        emit(row)


def kernel_cases(rows, reps, emit):
    k, most = 128, 17
    L = _csx.gmres_limits()
    N = 8 * rows * k
    V = cs.dvec(rows * k * (most + 1))
    V.fill(2.0 ** -10)
    W, U = cs.dvec(rows, k), cs.dvec(rows, k)
    W.fill(1.0)
    work = cs.dvec(_csx.gs_work_len(rows, k, most + 1))
    m = _csx.i32(np.ones(k))
    pm = _csx.pi(m)
    for nv in (1, 8, 17):
        h, nrm2, s = np.full((nv, k), 2.0 ** -20), np.zeros(k), np.full(k, 3.0)
        ln = _csx.i32(np.full(k, nv))
        calls = {
            "project": (lambda: lib().csx_gs_project(V.handle, nv, W.handle, work.handle, rows, k, pm, 0, _csx.pd(np.empty((nv, k)))),
                        (nv + -(-nv // L["GS_GROUP"])) * N),
            "update": (lambda: lib().csx_gs_update(V.handle, nv, W.handle, work.handle, rows, k, pm, 0, _csx.pd(h), _csx.pd(nrm2)),
                       (nv + 2) * N),
            "scale": (lambda: lib().csx_gs_scale(W.handle, V.handle, nv, work.handle, rows, k, pm, _csx.pd(s)), 2 * N),
            "combine": (lambda: lib().csx_gs_combine(V.handle, nv, U.handle, work.handle, rows, k, pm, _csx.pd(h), _csx.pi(ln)),
                        (nv + 1) * N),
        }
        for name, (fn, nbytes) in calls.items():
            t = []
            for rep in range(reps + 1):
                t.append(event_ms(lambda: _csx.check(fn(), name)))
            ms = float(np.median(t[1:]))
            emit({"case": "kernel", "kernel": name, "rows": rows, "nrhs": k, "nv": nv, "reps": reps, "ms": round(ms, 3),
                  "algorithmic_bytes": nbytes, "GBs": round(nbytes / (ms * 1e-3) / 1e9, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="stale,kernels")
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmres_time.jsonl"))
    a = ap.parse_args()
    _csx.init(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if "stale" in a.only.split(","):
        stale_cases(a.reps, emit)
        lib().csx_mem_trim()
    if "kernels" in a.only.split(","):
        kernel_cases(a.rows, a.reps, emit)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
