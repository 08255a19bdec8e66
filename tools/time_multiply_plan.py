#!/usr/bin/env python3
"""multiply_plan against the route it replaces.

    python tools/time_multiply_plan.py [--reps 5] [--scale 1.0] [--cases aat,normal,ladder]
                                       [--out profiles/multiply_plan_time.jsonl]

aat     A A' of BASELINE config 4's matrix S (csx_gen_grand_uniform, 32 entries per column, n = 1M x --scale): a .update()
        step against cs_multiply by default and against cs_multiply under "spgemm.ordered" = 1 (the only other route to the
        plan's bits), in the same run, interleaved call by call.  Records the host build time and the plan's bytes.
normal  a tall matrix A (5M x 1M at --scale 1, 8 entries per row): A' diag(d) A, scaled and unscaled, against cs_multiply of
        the same operands (which cannot scale: the parent route rebuilds B on the host first, not timed here).
ladder  2^22 products in slots of L products each, L = 8 .. 1024, every slot folded by one lane ("multiply.long" above L) and
        by a wave of its own (below L): the measurement that places the threshold.

Every figure is the median of --reps calls after one warm call: the kernel between two events (info()["kernel_us"]) and host
wall-clock per call ending in a synchronise.  plan_bytes = 8 products + 4 (nnz + 1) + 4 nnz(B) beside the pattern.
step_bytes = 8 products + 4 (nnz + 1) + 8 nnz + 16 products of gathers (an upper estimate: the gathers hit cache).  One JSON
line per case goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd")]


def wall(fn):
    import _csx
    _csx.sync()
    t0 = time.perf_counter()
    out = fn()
    _csx.sync()
    return out, 1e3 * (time.perf_counter() - t0)


def interleaved(fns, reps):
    """{name: median wall ms} of the calls, run one after another reps times after one warm round"""
    t = {name: [] for name in fns}
    for r in range(reps + 1):
        for name, fn in fns.items():
            ms = wall(fn)[1]
            if r:
                t[name].append(ms)
    return {name: float(np.median(v)) for name, v in t.items()}


def device_cs(h):
    import csparse as cs
    return cs._from_device(h, lambda k: k)


def upload(m, n, p, i, x):
    import _csx
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(m, n, _csx.pi(_csx.i32(p)), _csx.pi(_csx.i32(i)), _csx.pd(_csx.f64(x)), h), "csx_csc_upload")
    return device_cs(h)


def transpose(A):
    import _csx
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_transpose(A._dev.handle, 1, h), "csx_transpose")
    return device_cs(h)


def plan_record(label, A, B):
    import csparse as cs
    P, plan_ms = wall(lambda: cs.multiply_plan(A, B))
    info = P.info()
    nnz, products, bnz = info["nnz"], info["products"], cs._meta(B)[0]
    rec = {"case": label, "m": info["m"], "k": A.n, "n": info["n"], "nnz_a": cs._meta(A)[0], "nnz_b": bnz, "nnz": nnz,
           "products": products, "max_products": info["max_products"], "long_slots": info["long_slots"],
           "plan_wall_ms": plan_ms, "plan_host_build_ms": info["build_us"] / 1e3,
           "plan_bytes": 8 * products + 4 * (nnz + 1) + 4 * bnz,
           "step_bytes_estimate": 24 * products + 4 * (nnz + 1) + 8 * nnz}
    return P, rec


def kernel_ms(P, fn, reps):
    t = []
    for r in range(reps + 1):
        wall(fn)
        if r:
            t.append(P.info()["kernel_us"] / 1e3)
    return float(np.median(t))


def multiply_routes(A, B):
    import _csx
    import csparse as cs

    def default():
        cs.cs_multiply(A, B)

    def ordered():
        with _csx.option("spgemm.ordered", 1):
            cs.cs_multiply(A, B)

    return default, ordered


def aat(a):
    import _csx
    n = max(1000, int(1_000_000 * a.scale))
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_gen_grand_uniform(n, 32, 20240605, h), "csx_gen_grand_uniform")
    S = device_cs(h)
    ST = transpose(S)
    P, rec = plan_record("aat", S, ST)
    P.matrix
    default, ordered = multiply_routes(S, ST)
    t = interleaved({"update": lambda: P.update(), "cs_multiply_default": default, "cs_multiply_ordered": ordered}, a.reps)
    rec["update_wall_ms"] = t["update"]
    rec["cs_multiply_default_wall_ms"] = t["cs_multiply_default"]
    rec["cs_multiply_ordered_wall_ms"] = t["cs_multiply_ordered"]
    rec["update_kernel_ms"] = kernel_ms(P, lambda: P.update(), a.reps)
    rec["multiply_new_dvec_wall_ms"] = interleaved({"multiply": lambda: P.multiply()}, a.reps)["multiply"]
    rec["default_over_update"] = t["cs_multiply_default"] / t["update"]
    rec["ordered_over_update"] = t["cs_multiply_ordered"] / t["update"]
    with _csx.option("spgemm.ordered", 1):
        import csparse as cs
        C = cs.cs_multiply(S, ST)
    x = np.empty(max(rec["nnz"], 1))
    _csx.check(_csx.lib().csx_csc_download(C._dev.handle, None, None, _csx.pd(x)), "csx_csc_download")
    rec["bytes_equal_to_ordered"] = bool(P.multiply().numpy().tobytes() == x[:rec["nnz"]].tobytes())
    return [rec]


def normal(a):
    import csparse as cs
    rows, cols = max(5000, int(5_000_000 * a.scale)), max(1000, int(1_000_000 * a.scale))
    rng = np.random.default_rng(7)
    # A' as CSC: one column per row of A, 8 entries each
    AT = upload(cols, rows, 8 * np.arange(rows + 1, dtype=np.int64), rng.integers(0, cols, 8 * rows), rng.uniform(0.5, 1.5, 8 * rows))
    A = transpose(AT)
    P, rec = plan_record("normal", AT, A)
    P.matrix
    d = cs.dvec(rng.uniform(0.5, 2.0, rows))
    default, ordered = multiply_routes(AT, A)
    t = interleaved({"unscaled": lambda: P.update(), "scaled": lambda: P.update(scale=d), "cs_multiply_default": default,
                     "cs_multiply_ordered": ordered}, a.reps)
    rec["update_wall_ms"], rec["update_scaled_wall_ms"] = t["unscaled"], t["scaled"]
    rec["cs_multiply_default_wall_ms"], rec["cs_multiply_ordered_wall_ms"] = t["cs_multiply_default"], t["cs_multiply_ordered"]
    rec["update_kernel_ms"] = kernel_ms(P, lambda: P.update(), a.reps)
    rec["update_scaled_kernel_ms"] = kernel_ms(P, lambda: P.update(scale=d), a.reps)
    return [rec]


def ladder(a):
    import _csx
    import csparse as cs
    k = max(1 << 12, int((1 << 22) * a.scale))
    rng = np.random.default_rng(9)
    out = []
    rows = 1 << 10
    for L in (8, 16, 32, 64, 128, 256, 1024):
        slots = k // L
        kk = slots * L
        slot_of = rng.permutation(np.repeat(np.arange(slots, dtype=np.int64), L))   # inner index -> its slot
        ncols = (slots + rows - 1) // rows
        order = np.argsort(slot_of // rows, kind="stable")                          # B(:,j): the inner indices of column j
        A = upload(rows, kk, np.arange(kk + 1), slot_of % rows, rng.uniform(-1.0, 1.0, kk))
        Bp = np.concatenate([[0], np.cumsum(np.bincount(slot_of // rows, minlength=ncols))])
        B = upload(kk, ncols, Bp, order, rng.uniform(-1.0, 1.0, kk))
        rec = {"case": "ladder", "products_per_slot": L, "slots": slots, "products": kk}
        for name, thr in (("lane", 1 << 30), ("wave", L - 1)):
            with _csx.option("multiply.long", thr):
                P = cs.multiply_plan(A, B)
                info = P.info()
                assert info["long_slots"] == (0 if name == "lane" else slots) and info["max_products"] == L
                rec[name + "_kernel_ms"] = kernel_ms(P, lambda: P.multiply(), a.reps)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every case (rehearsals, or a box the full size does not fit)")
    ap.add_argument("--cases", default="aat,normal,ladder")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiply_plan_time.jsonl"))
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    cases = {"aat": aat, "normal": normal, "ladder": ladder}
    for name in a.cases.split(","):
        for rec in cases[name](a):
            rec["device"] = cs.device_name()
            rec["reps"] = a.reps
            rec["scale"] = a.scale
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
