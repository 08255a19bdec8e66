#!/usr/bin/env python3
"""residual_block against gaxpy_block EXACT, and refine() against solve().

    python tools/time_refine.py [--reps 10] [--only spd,grand,gen1m,w] [--out FILE]

spd / grand: csx_residual_block forward and transposed, with and without the store of R, beside csx_gaxpy_block EXACT at the
same k (8 and 128) in the same run, on config 5's G-spd (78 125 dense blocks of 64, n = 5M) and the bench G-rand (5M x 5M, 64
per column): medians of --reps hipEvent-timed calls after two warm calls, the forms taken in turn inside every repetition.
ratio_forward = residual forward / gaxpy_block EXACT: the forward residual does gaxpy_block's gathers plus two VALU
operations per term, so a ratio far above 1 needs an explanation from a counter pass (a run of its own).  Algorithmic bytes
12 nnz + 4 (rows + 1) + 8 cols k + 16 rows k + 16 k against 8 TB/s.
gen1m / w: refine() against solve() on the 1M-row generated reducible matrix through btf_factor and on W (1 493 components of
67 rows) through lusol_factor, both after a refactor() to values perturbed by 1e-3 (the pivots hold: refinement has little
to do, which is the common case whose cost matters), k = 8 and 128; wall clock to a synchronise, with omega0, omega, steps.
One JSON line per case on stdout and in --out (default profiles/refine_time.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402

PEAK_GBS = 8000.0


def lib():
    return _csx.lib()


def gen(fn, *args):
    h = _csx.new_handle()
    _csx.check(getattr(lib(), fn)(*args, h), fn)
    return h


def event_ms(fn):
    _csx.check(lib().csx_timer_start(), "timer")
    fn()
    t = C.c_double()
    _csx.check(lib().csx_timer_stop(t), "timer")
    return t.value


def residual_case(name, hA, n, nnz, k, reps):
    X = gen("csx_gen_vec", n * k, 7, -1.0, 1.0)
    B = gen("csx_gen_vec", n * k, 8, -1.0, 1.0)
    R, Y = cs.dvec(n, k), cs.dvec(n, k)
    omega, rnorm = np.empty(k), np.empty(k)
    algo = 12 * nnz + 4 * (n + 1) + 8 * n * k + 16 * n * k + 16 * k

    def residual(trans, store):
        return lambda: _csx.check(lib().csx_residual_block(hA, X, B, R.handle if store else 0, k, trans, _csx.pd(omega),
                                                           _csx.pd(rnorm)), "csx_residual_block")

    forms = {"gaxpy_block_exact": lambda: _csx.check(lib().csx_gaxpy_block(hA, X, Y.handle, k, cs.GAXPY_EXACT), "csx_gaxpy_block"),
             "residual_forward": residual(0, True), "residual_forward_no_store": residual(0, False),
             "residual_trans": residual(1, True), "residual_trans_no_store": residual(1, False)}
    times = {f: [] for f in forms}
    for r in range(reps + 2):
        for f, fn in forms.items():
            ms = event_ms(fn)
            if r >= 2:
                times[f].append(ms)
    row = {"matrix": name, "n": n, "nnz": nnz, "k": k, "algorithmic_bytes": algo, "reps": reps}
    for f, t in times.items():
        row[f + "_ms"] = round(float(np.median(t)), 4)
    row["residual_forward_frac_of_8TBs"] = round(algo / (row["residual_forward_ms"] * 1e-3) / (PEAK_GBS * 1e9), 3)
    row["ratio_forward"] = round(row["residual_forward_ms"] / row["gaxpy_block_exact_ms"], 3)
    row["ratio_trans"] = round(row["residual_trans_ms"] / row["gaxpy_block_exact_ms"], 3)
    for h in (X, B):
        _csx.free(h)
    return row


def wall(fn):
    _csx.sync()
    t0 = time.perf_counter()
    out = fn()
    _csx.sync()
    return out, 1e3 * (time.perf_counter() - t0)


def refine_case(name, sol, n, k, reps):
    B = np.random.default_rng(k).uniform(-1, 1, (n, k))
    solve, refine, out = [], [], None
    for r in range(reps + 1):
        dB = cs.dvec(B)
        _, ms = wall(lambda: sol.solve(dB))
        dB = cs.dvec(B)
        out, ms2 = wall(lambda: sol.refine(dB))
        if r:
            solve.append(ms)
            refine.append(ms2)
    row = {"matrix": name, "n": n, "k": k, "reps": reps, "solve_ms": round(float(np.median(solve)), 3),
           "refine_ms": round(float(np.median(refine)), 3), "solves": int(out["solves"]), "steps_max": int(out["steps"].max()),
           "omega0_max_eps": float(np.max(out["omega0"]) * 2.0 ** 52), "omega_max_eps": float(np.max(out["omega"]) * 2.0 ** 52)}
    row["ratio"] = round(row["refine_ms"] / row["solve_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="spd,grand,gen1m,w")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_time.jsonl"))
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
            emit(residual_case(name, hA, n, nnz, k, a.reps))
        del A
        lib().csx_mem_trim()
    if "gen1m" in only:
        import btf_oracle
        from time_refactor import device
        S = btf_oracle.reducible(btf_oracle.block_sizes(1_000_000, 11), 8, 11)[0]
        sol = cs.btf_factor(device(S))
        assert sol.refactor(S.data * (1.0 + 1e-3 * np.random.default_rng(31).uniform(-1, 1, S.nnz)))
        for k in (8, 128):
            emit(refine_case("gen1m", sol, S.shape[0], k, max(a.reps // 2, 2)))
    if "w" in only:
        from time_refactor import device, w_matrix
        W, W2 = w_matrix(1493, 20240604), w_matrix(1493, 77)
        sol = cs.lusol_factor(device(W), 0, 0.1)
        assert sol.refactor(W2.data)
        for k in (8, 128):
            emit(refine_case("W", sol, W.shape[0], k, a.reps))
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
