#!/usr/bin/env python3
"""add_plan against the route it replaces, cs_add.

    python tools/time_add_plan.py [--reps 5] [--scale 1.0] [--cases pencil2,pencil3,shift,grand]
                                  [--out profiles/add_plan_time.jsonl]

pencil2  K + sigma M on the block-SPD matrix of the benchmark (csx_gen_gspd, blocks of 64, 5M rows at --scale 1), M another
         matrix on the same pattern: the aligned class, k = 2.
pencil3  K + sigma M + tau M2 on the same pattern: the aligned class, k = 3; cs_add is the chain of two calls.
shift    K + sigma I on the same K: the general class (every diagonal slot has two terms, every other slot one).
grand    A + A' of G-rand (csx_gen_grand, 64 entries per column, 5M x 5M at --scale 1): the general class; the case
         bench_configs.py times for cs_add at its own size.

Per case: the plan's build (wall clock, and the host rule's share from info()), then, interleaved call by call in the same run
after one warm round, .add (a new dvec), .update (into .matrix) and cs_add on the same device-resident operands; every figure
is the median of --reps calls: host wall-clock ending in a synchronise, and for the plan's steps the kernel between the plan's
two events (info()["kernel_us"]).  step_bytes is what a step must move: 8 (k + 1) nnz for the aligned class, 12 terms + 12 nnz
for the general one (4 bytes of src, 8 of the value per term; 8 bytes out, 4 of sp per slot); frac_of_peak is step_bytes over
the kernel time over the 8 TB/s of the chip.  cs_add_over_update is the one condition fixed in advance: a step does strictly
less work than cs_add, so the ratio must not be below 1; a case that violates it is marked "slower_than_cs_add".  One JSON line
per case goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd")]

HBM_PEAK_GBS = 8000.0


def wall(fn):
    import _csx
    _csx.sync()
    t0 = time.perf_counter()
    out = fn()
    _csx.sync()
    return out, 1e3 * (time.perf_counter() - t0)


def interleaved(fns, reps, after=None):
    """{name: median wall ms} of the calls, run one after another reps times after one warm round; after(name): a figure read
    after each timed call (the plan's kernel time), its median under name + "_kernel" """
    t = {name: [] for name in fns}
    k = {name: [] for name in fns}
    for r in range(reps + 1):
        for name, fn in fns.items():
            ms = wall(fn)[1]
            if r:
                t[name].append(ms)
                if after is not None and after(name) is not None:
                    k[name].append(after(name))
    out = {name: float(np.median(v)) for name, v in t.items()}
    out.update({name + "_kernel": float(np.median(v)) for name, v in k.items() if v})
    return out


def device_cs(h):
    import csparse as cs
    return cs._from_device(h, lambda k: k)


def gspd(nb, seed):
    import _csx
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_gen_gspd(nb, 64, seed, h), "csx_gen_gspd")
    return device_cs(h)


def identity(n):
    import _csx
    h = _csx.new_handle()
    idx = np.arange(n + 1, dtype=np.int32)
    _csx.check(_csx.lib().csx_csc_upload(n, n, _csx.pi(idx), _csx.pi(idx[:n]), _csx.pd(np.ones(n)), h), "csx_csc_upload")
    return device_cs(h)


def values_of(M, nnz):
    import _csx
    x = np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, None, None, _csx.pd(x)), "csx_csc_download")
    return x[:nnz].tobytes()


def run_case(label, ops, coef, reps):
    import csparse as cs
    k = len(ops)

    def chain():
        C = cs.cs_add(ops[0], ops[1], coef[0], coef[1])
        for r in range(2, k):
            C = cs.cs_add(C, ops[r], 1.0, coef[r])
        return C

    P, plan_ms = wall(lambda: cs.add_plan(*ops, coef=coef))
    info = P.info()
    nnz, terms, aligned = info["nnz"], info["terms"], info["aligned"]
    step_bytes = 8 * (k + 1) * nnz if aligned else 12 * terms + 12 * nnz
    rec = {"case": label, "k": k, "m": info["m"], "n": info["n"], "nnz": nnz, "terms": terms, "max_terms": info["max_terms"],
           "long_slots": info["long_slots"], "aligned": aligned, "plan_wall_ms": plan_ms,
           "plan_host_build_ms": info["build_us"] / 1e3, "step_bytes": step_bytes}
    P.matrix
    t = interleaved({"add": lambda: P.add(), "update": lambda: P.update(), "cs_add": chain}, reps,
                    after=lambda name: None if name == "cs_add" else P.info()["kernel_us"] / 1e3)
    rec["add_wall_ms"], rec["update_wall_ms"], rec["cs_add_wall_ms"] = t["add"], t["update"], t["cs_add"]
    rec["add_kernel_ms"], rec["update_kernel_ms"] = t["add_kernel"], t["update_kernel"]
    for name in ("add", "update"):
        ms = rec[name + "_kernel_ms"]
        rec[name + "_GBps"] = step_bytes / ms / 1e6 if ms > 0 else None
        rec[name + "_frac_of_peak"] = step_bytes / ms / 1e6 / HBM_PEAK_GBS if ms > 0 else None
    rec["cs_add_over_add"] = t["cs_add"] / t["add"]
    rec["cs_add_over_update"] = t["cs_add"] / t["update"]
    rec["slower_than_cs_add"] = bool(t["add"] > t["cs_add"] or t["update"] > t["cs_add"])
    rec["bytes_equal_to_cs_add"] = bool(P.add().numpy().tobytes() == values_of(chain(), nnz))
    return rec


def pencil(a, k):
    nb = max(16, int(5_000_000 * a.scale) // 64)
    ops = [gspd(nb, 20240601 + 5 + r) for r in range(k)]
    return run_case("pencil%d" % k, ops, [1.0, 0.1 + 1e-9, -2.5 / 3.0][:k], a.reps)


def shift(a):
    nb = max(16, int(5_000_000 * a.scale) // 64)
    return run_case("shift", [gspd(nb, 20240601 + 5), identity(64 * nb)], [1.0, 0.1 + 1e-9], a.reps)


def grand(a):
    import _csx
    n = max(1000, int(5_000_000 * a.scale))
    h, ht = _csx.new_handle(), _csx.new_handle()
    _csx.check(_csx.lib().csx_gen_grand(n, 64, 20240607, h), "csx_gen_grand")
    _csx.check(_csx.lib().csx_transpose(h, 1, ht), "csx_transpose")
    return run_case("grand", [device_cs(h), device_cs(ht)], [1.0, 1.0], a.reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every case (rehearsals, or a box the full size does not fit)")
    ap.add_argument("--cases", default="pencil2,pencil3,shift,grand")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add_plan_time.jsonl"))
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    cases = {"pencil2": lambda: pencil(a, 2), "pencil3": lambda: pencil(a, 3), "shift": lambda: shift(a), "grand": lambda: grand(a)}
    for name in a.cases.split(","):
        rec = cases[name]()
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
