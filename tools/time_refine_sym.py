#!/usr/bin/env python3
"""residual_block(sym=True) against residual_block forward, and cholsol_factor's refine() against solve().

    python tools/time_refine_sym.py [--reps 10] [--only residual,refine,condest] [--out FILE]

residual: csx_residual_sym_block beside csx_residual_block (forward) on the same matrix in the same run, at k = 8 and 128, with
the store of R: on config 5's G-spd (78 125 dense blocks of 64, n = 5M) as the bench stores it -- in full -- and on the same
matrix cut to its upper triangle (csx_symperm with no permutation), where the general call measures another operator and is
timed only for its traffic.  Medians of --reps hipEvent-timed calls after two warm calls, the forms taken in turn inside every
repetition.  ratio = symmetric / general on the same storage; ratio_upper_over_full = symmetric on the upper triangle /
symmetric on the full storage.  Expected, not gated: the symmetric call reads the columns AND the row gather, 24 nnz bytes of
entries, and uses half of each on a fully stored matrix; on the upper triangle that is 12 bytes per entry of the operator.
refine: cholsol_factor(G-spd).refine() against solve() at k = 8 and 128, wall clock to a synchronise, with omega0, omega, steps.
condest: one condest() on that solver, wall clock (its solves are single right-hand sides from host lists).
One JSON line per case on stdout and in --out (default profiles/refine_sym_time.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402
from time_refine import PEAK_GBS, event_ms, gen, lib, refine_case, wall  # noqa: E402


def residual_case(name, hA, n, nnz, k, reps):
    X = gen("csx_gen_vec", n * k, 7, -1.0, 1.0)
    B = gen("csx_gen_vec", n * k, 8, -1.0, 1.0)
    R = cs.dvec(n, k)
    omega, rnorm = np.empty(k), np.empty(k)
    blocks = 8 * n * k + 16 * n * k + 16 * k
    forms = {"general": lambda: _csx.check(lib().csx_residual_block(hA, X, B, R.handle, k, 0, _csx.pd(omega), _csx.pd(rnorm)),
                                           "csx_residual_block"),
             "sym": lambda: _csx.check(lib().csx_residual_sym_block(hA, X, B, R.handle, k, _csx.pd(omega), _csx.pd(rnorm)),
                                       "csx_residual_sym_block")}
    times = {f: [] for f in forms}
    for r in range(reps + 2):
        for f, fn in forms.items():
            ms = event_ms(fn)
            if r >= 2:
                times[f].append(ms)
    row = {"matrix": name, "n": n, "nnz": nnz, "k": k, "reps": reps,
           "general_algorithmic_bytes": 12 * nnz + 4 * (n + 1) + blocks, "sym_algorithmic_bytes": 24 * nnz + 8 * (n + 1) + blocks}
    for f, t in times.items():
        row[f + "_ms"] = round(float(np.median(t)), 4)
    row["sym_frac_of_8TBs"] = round(row["sym_algorithmic_bytes"] / (row["sym_ms"] * 1e-3) / (PEAK_GBS * 1e9), 3)
    row["ratio"] = round(row["sym_ms"] / row["general_ms"], 3)
    for h in (X, B):
        _csx.free(h)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="residual,refine,condest")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_sym_time.jsonl"))
    a = ap.parse_args()
    only = a.only.split(",")
    _csx.init(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    hA = gen("csx_gen_gspd", 78125, 64, 20240606)
    A = cs.cs_pin(cs._from_device(hA, lambda nnz: max(nnz, 1)))
    _, n, nnz, _ = A._dev.info()
    if "residual" in only:
        full = {}
        for k in (8, 128):
            full[k] = residual_case("spd_full", hA, n, nnz, k, a.reps)
            emit(full[k])
        U = cs.cs_pin(cs.cs_symperm(A, None, True))
        unz = U._dev.info()[2]
        for k in (8, 128):
            row = residual_case("spd_upper", U._dev.handle, n, unz, k, a.reps)
            row["ratio_upper_over_full"] = round(row["sym_ms"] / full[k]["sym_ms"], 3)
            emit(row)
        del U
        lib().csx_mem_trim()
    if "refine" in only or "condest" in only:
        sol = cs.cholsol_factor(A)
        if "refine" in only:
            for k in (8, 128):
                emit(refine_case("spd_cholsol", sol, n, k, max(a.reps // 2, 2)))
        if "condest" in only:
            est, ms = wall(sol.condest)
            emit({"matrix": "spd_cholsol", "n": n, "condest": est, "condest_ms": round(ms, 1)})
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
