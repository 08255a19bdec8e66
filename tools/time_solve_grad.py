#!/usr/bin/env python3
"""csx_pattern_outer against csx_residual_block(trans), and solve_grad() against two solve() calls.

    python tools/time_solve_grad.py [--reps 10] [--only spd,grand,w] [--out FILE]

spd / grand: csx_pattern_outer (general, and sym on G-spd) beside csx_residual_block(trans = 1, R stored) on the same matrix and
the same k (8 and 128) in the same run, on config 5's G-spd (78 125 dense blocks of 64, n = 5M) and the bench G-rand (5M x 5M,
64 per column) -- the matrices and the harness of tools/time_refine.py: medians of --reps hipEvent-timed calls after two warm
calls, the forms taken in turn inside every repetition.  The transposed residual is the yardstick because it performs the same
row gathers down the same stored columns.  GB/s on the algorithmic bytes of each call: 12 nnz + 4 (n + 1) + 8 (m + n) k for the
outer product, 12 nnz + 4 (n + 1) + 24 n k + 16 k for the residual.  ratio = pattern_outer / residual_trans, as measured.
w: solve_grad() against two solve() calls on lusol_factor of W (1 493 components of 67 rows), k = 8 and 128; wall clock to a
synchronise.  One JSON line per case on stdout and in --out (default profiles/solve_grad_time.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402
from time_refine import event_ms, gen, lib, wall  # noqa: E402


def outer_case(name, hA, n, nnz, k, reps, sym):
    U = gen("csx_gen_vec", n * k, 7, -1.0, 1.0)
    V = gen("csx_gen_vec", n * k, 8, -1.0, 1.0)
    R, out = cs.dvec(n, k), cs.dvec(nnz)
    omega, rnorm = np.empty(k), np.empty(k)
    bytes_outer = 12 * nnz + 4 * (n + 1) + 8 * (n + n) * k
    bytes_residual = 12 * nnz + 4 * (n + 1) + 8 * n * k + 16 * n * k + 16 * k
    forms = {"residual_trans": lambda: _csx.check(lib().csx_residual_block(hA, U, V, R.handle, k, 1, _csx.pd(omega),
                                                                           _csx.pd(rnorm)), "csx_residual_block"),
             "pattern_outer": lambda: _csx.check(lib().csx_pattern_outer(hA, U, V, k, 0, -1.0, out.handle), "csx_pattern_outer")}
    if sym:
        forms["pattern_outer_sym"] = lambda: _csx.check(lib().csx_pattern_outer(hA, U, V, k, 1, -1.0, out.handle),
                                                        "csx_pattern_outer")
    times = {f: [] for f in forms}
    for r in range(reps + 2):
        for f, fn in forms.items():
            ms = event_ms(fn)
            if r >= 2:
                times[f].append(ms)
    row = {"matrix": name, "n": n, "nnz": nnz, "k": k, "reps": reps, "device": _csx.device_info()[0],
           "pattern_outer_bytes": bytes_outer, "residual_trans_bytes": bytes_residual}
    for f, t in times.items():
        row[f + "_ms"] = round(float(np.median(t)), 4)
    row["pattern_outer_GBs"] = round(bytes_outer / (row["pattern_outer_ms"] * 1e-3) / 1e9, 1)
    row["residual_trans_GBs"] = round(bytes_residual / (row["residual_trans_ms"] * 1e-3) / 1e9, 1)
    row["ratio_ms"] = round(row["pattern_outer_ms"] / row["residual_trans_ms"], 4)
    if sym:
        row["ratio_sym_ms"] = round(row["pattern_outer_sym_ms"] / row["residual_trans_ms"], 4)
    for h in (U, V):
        _csx.free(h)
    return row


def grad_case(name, sol, n, k, reps):
    B = np.random.default_rng(k).uniform(-1, 1, (n, k))
    GX = np.random.default_rng(k + 1).uniform(-1, 1, (n, k))
    two, grad = [], []
    for r in range(reps + 1):
        dB, dG = cs.dvec(B), cs.dvec(GX)

        def solves():
            sol.solve(dB)
            sol.solve(dG, trans=True)

        _, ms = wall(solves)
        dG = cs.dvec(GX)
        _, ms2 = wall(lambda: sol.solve_grad(dB, dG))
        if r:
            two.append(ms)
            grad.append(ms2)
    row = {"matrix": name, "n": n, "k": k, "reps": reps, "device": _csx.device_info()[0],
           "two_solves_ms": round(float(np.median(two)), 3), "solve_grad_ms": round(float(np.median(grad)), 3)}
    row["ratio"] = round(row["solve_grad_ms"] / row["two_solves_ms"], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="spd,grand,w")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_grad_time.jsonl"))
    a = ap.parse_args()
    only = a.only.split(",")
    _csx.init(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for name, fn, args in (("spd", "csx_gen_gspd", (78125, 64, 20240606)), ("grand", "csx_gen_grand", (5_000_000, 64, 20240601))):
        if name not in only:
            continue
        hA = gen(fn, *args)
        A = cs._from_device(hA, lambda nnz: max(nnz, 1))
        _, n, nnz, _ = A._dev.info()
        for k in (8, 128):
            emit(outer_case(name, hA, n, nnz, k, a.reps, name == "spd"))
        del A
        lib().csx_mem_trim()
    if "w" in only:
        from time_refactor import device, w_matrix
        W = w_matrix(1493, 20240604)
        sol = cs.lusol_factor(device(W), 0, 0.1)
        for k in (8, 128):
            emit(grad_case("W", sol, W.shape[0], k, a.reps))
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
