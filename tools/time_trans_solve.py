#!/usr/bin/env python3
"""Transposed solves against forward solves on the same factors, and condest().

    python tools/time_trans_solve.py [--reps 5] [--only w,gen1m]

W (config 3: 1 493 components of 67 rows, lusol_factor in both orders) at k = 1 / 64 / 1 024, and btf_factor on the
1M-row generated reducible matrix of tools/time_btf.py at k = 1 / 8 / 128.  Forward and transposed solves alternate in
one process; each is the median of --reps warm calls timed with hipEvents on the library's stream (the block is
rewritten before every call, outside the timing).  condest() is host wall-clock.  One JSON line per case goes to
profiles/trans_solve_time.jsonl."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import synth  # noqa: E402
from conftest import golden  # noqa: E402


def w_matrix(nb=1493):
    g = golden("west0067")
    bp, bi, bx = g["C_p"].astype(np.int64), g["C_i"].astype(np.int64), g["C_x"]
    u = synth.vec(nb, 20240604, 0.0, 1.0)
    Ai = (bi[None, :] + (np.arange(nb) * 67)[:, None]).reshape(-1).astype(np.int32)
    Ax = (bx[None, :] * (1.0 + 1e-3 * u)[:, None]).reshape(-1)
    Ap = np.concatenate([[0], np.cumsum(np.tile(np.diff(bp), nb))]).astype(np.int32)
    return nb * 67, Ap, Ai, Ax


def alternate(solve, n, k, reps):
    """median ms of forward and of transposed solves of one n-by-k block, taken alternately"""
    import _csx
    import csparse as cs
    B = np.random.default_rng(k).uniform(-1, 1, (n, k))
    dB = cs.dvec(B)
    times = {False: [], True: []}
    for r in range(reps + 1):
        for trans in (False, True):
            dB.assign(B)
            _csx.sync()
            _csx.check(_csx.lib().csx_timer_start(), "timer")
            solve(dB, trans)
            ms = _csx.C.c_double(0)
            _csx.check(_csx.lib().csx_timer_stop(_csx.C.byref(ms)), "timer")
            if r:
                times[trans].append(ms.value)
    fwd, tr = float(np.median(times[False])), float(np.median(times[True]))
    return {"k": k, "forward_ms": fwd, "trans_ms": tr, "ratio": tr / fwd}


def wall(fn):
    t0 = time.perf_counter()
    v = fn()
    return v, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="w,gen1m")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    recs = []
    if "w" in a.only.split(","):
        n, Ap, Ai, Ax = w_matrix()
        A = cs.cs_spalloc(n, n, len(Ai), True, False)
        A.p, A.i, A.x = Ap.tolist(), Ai.tolist(), Ax.tolist()
        for label, exact in (("exact", True), ("rounding_equal", False)):
            F = cs.lusol_factor(A, 0, 1.0, exact=exact)
            for k in (1, 64, 1024):
                fused = {}

                def solve(dB, trans):
                    F.solve(dB, trans=trans)
                    fused[trans] = F.last_fused

                rec = {"matrix": "W", "n": n, "solver": "lusol_factor", "order": label}
                rec.update(alternate(solve, n, k, a.reps))
                rec["fused"] = {"forward": fused[False], "trans": fused[True]}
                recs.append(rec)
                print(json.dumps(rec), flush=True)
        F = cs.lusol_factor(A, 0, 1.0)
        est, ms = wall(F.condest)
        est2, ms2 = wall(F.condest)
        rec = {"matrix": "W", "n": n, "solver": "lusol_factor", "condest": est, "condest_ms_first": ms, "condest_ms": ms2,
               "repeatable": est == est2}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if "gen1m" in a.only.split(","):
        import btf_oracle
        from time_btf import device
        S = btf_oracle.reducible(btf_oracle.block_sizes(1_000_000, 11), 8, 11)[0]
        n = S.shape[0]
        A = device(S)
        sol = cs.btf_factor(A)
        _, first_ms = wall(lambda: sol.solve(cs.dvec(n, 1), trans=True))   # builds the transposed programs
        for k in (1, 8, 128):
            rec = {"matrix": "gen1m", "n": n, "solver": "btf_factor", "first_trans_call_ms": first_ms}
            rec.update(alternate(lambda dB, trans: sol.solve(dB, trans=trans), n, k, a.reps))
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        est, ms = wall(sol.condest)
        est2, ms2 = wall(sol.condest)
        rec = {"matrix": "gen1m", "n": n, "solver": "btf_factor", "condest": est, "condest_ms_first": ms, "condest_ms": ms2,
               "repeatable": est == est2}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    with open(os.path.join(ROOT, "profiles", "trans_solve_time.jsonl"), "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
