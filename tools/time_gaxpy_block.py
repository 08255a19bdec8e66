#!/usr/bin/env python3
"""Device times of csx_gaxpy_block (Y += A X, X n-by-k) on config 5's G-spd (78 125 dense blocks of 64, n = 5M) and the
bench G-rand (5M x 5M, 64 uniform rows per column), beside k single-vector csx_gaxpy AUTO calls on contiguous vectors
(what a caller can do without the block call).

    python tools/time_gaxpy_block.py [--reps 20] [--ks 1,2,4,8,32,128] [--only spd,grand] [--no-baseline] [--out FILE]

Per case: EXACT, AUTO, and on G-rand both AUTO routes forced (the block kernel, the column route), median and min of
--reps hipEvent-timed calls after two warm-up calls.  Algorithmic bytes 12 nnz + 4 (m + 1) + 8 n k + 16 m k against
8 TB/s.  One JSON line per case on stdout and in --out (default profiles/gaxpy_block_time.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402

PEAK_GBS = 8000.0


def lib():
    return _csx.lib()


def gen(fn, *args):
    h = _csx.new_handle()
    _csx.check(getattr(lib(), fn)(*args, h), fn)
    return h


def timed(fn, reps):
    fn()
    fn()
    ms = []
    for _ in range(reps):
        _csx.check(lib().csx_timer_start())
        fn()
        t = C.c_double()
        _csx.check(lib().csx_timer_stop(t))
        ms.append(t.value)
    return float(np.median(ms)), float(min(ms))


def wrap(ptr, length):
    h = _csx.new_handle()
    _csx.check(lib().csx_vec_wrap(C.c_void_p(ptr), length, h))
    return h


def case(name, hA, n, nnz, k, reps, baseline):
    X = gen("csx_gen_vec", n * k, 7, -1.0, 1.0)
    Y = cs.dvec(n, k)
    algo = 12 * nnz + 4 * (n + 1) + 8 * n * k + 16 * n * k
    row = {"matrix": name, "n": n, "nnz": nnz, "k": k, "algorithmic_bytes": algo, "reps": reps}

    def block(mode):
        return lambda: _csx.check(lib().csx_gaxpy_block(hA, X, Y.handle, k, mode), "csx_gaxpy_block")

    forms = [("exact", block(cs.GAXPY_EXACT), None), ("auto", block(cs.GAXPY_AUTO), None)]
    if name == "grand" and k > 1:
        forms += [("route_block", block(cs.GAXPY_AUTO), 1), ("route_columns", block(cs.GAXPY_AUTO), 2)]
    for label, fn, route in forms:
        if route is None:
            med, mn = timed(fn, reps)
        else:
            with _csx.option("gaxpy.block_route", route):
                med, mn = timed(fn, reps)
        row[label + "_ms_median"], row[label + "_ms_min"] = round(med, 4), round(mn, 4)
        row[label + "_frac_of_8TBs"] = round(algo / (med * 1e-3) / (PEAK_GBS * 1e9), 3)
    if baseline:
        # k calls of csx_gaxpy AUTO on k contiguous vectors (views into two buffers)
        Xc, Yc = cs.dvec(n * k), cs.dvec(n * k)
        px, py = Xc.device_ptr(), Yc.device_ptr()
        hx = [wrap(px + 8 * n * c, n) for c in range(k)]
        hy = [wrap(py + 8 * n * c, n) for c in range(k)]

        def singles():
            for c in range(k):
                _csx.check(lib().csx_gaxpy(hA, hx[c], hy[c], cs.GAXPY_AUTO), "csx_gaxpy")

        med, mn = timed(singles, max(5, reps // 2) if k >= 32 else reps)
        row["k_single_auto_ms_median"], row["k_single_auto_ms_min"] = round(med, 4), round(mn, 4)
        row["auto_speedup_vs_k_single"] = round(med / row["auto_ms_median"], 2)
        for h in hx + hy:
            _csx.free(h)
        del Xc, Yc
    _csx.free(X)
    del Y
    _csx.check(lib().csx_mem_trim())
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", default="1,2,4,8,32,128")
    ap.add_argument("--only", default="spd,grand")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaxpy_block_time.jsonl"))
    a = ap.parse_args()
    _csx.init(0)
    ks = [int(v) for v in a.ks.split(",")]
    rows = []
    for name in a.only.split(","):
        if name == "spd":
            hA, n, nnz = gen("csx_gen_gspd", 78125, 64, 20240606), 78125 * 64, 78125 * 64 * 64
        else:
            hA, n, nnz = gen("csx_gen_grand_uniform", 5000000, 64, 20240601 + 1), 5000000, 5000000 * 64
        _csx.check(lib().csx_gaxpy_prepare(hA, cs.GAXPY_AUTO))
        _csx.check(lib().csx_gaxpy_prepare(hA, cs.GAXPY_EXACT))
        for k in ks:
            row = case(name, hA, n, nnz, k, a.reps, not a.no_baseline)
            print(json.dumps(row), flush=True)
            rows.append(row)
        _csx.free(hA)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
