#!/usr/bin/env python3
"""refactor() against a fresh factor.

    python tools/time_refactor.py [--reps 5] [--out profiles/refactor_time.jsonl]

gen1m: the 1M-row generated reducible matrix of tests/test_gpu_btf.py (btf_oracle.block_sizes(1_000_000, 11), 8 levels)
and the same pattern with entries x (1 + 1e-3 u).  Times: the first refactor (maps and schedule included), a steady-state
refactor (A2 and A alternated; as a device-resident matrix, and as values in a numpy array or a dvec), forward solves at
k = 1 / 8 / 128 before and after a refactor, and a fresh btf_factor of A2.  W: config 3's 1 493 blocks of west0067 at tol 0.1, new block scales: lusol_factor(W).refactor(W2) with the first
solve after it (the triangular plans are rebuilt there), against a fresh lusol_factor(W2) and its first solve.
A refactor or a solve is timed with hipEvents on the library's stream around the call (the calls synchronise), the median
of --reps warm calls; factors and first solves are host wall-clock.  One JSON line per matrix goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]

import btf_oracle  # noqa: E402
import synth  # noqa: E402


def device(S):
    import _csx
    import csparse as cs
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(S.shape[0], S.shape[1], _csx.pi(_csx.i32(S.indptr)), _csx.pi(_csx.i32(S.indices)),
                                         _csx.pd(_csx.f64(S.data)), h), "upload")
    return cs._from_device(h, lambda nnz: max(nnz, 1))


def event_ms(fn):
    import _csx
    _csx.sync()
    _csx.check(_csx.lib().csx_timer_start(), "timer")
    fn()
    ms = _csx.C.c_double(0)
    _csx.check(_csx.lib().csx_timer_stop(_csx.C.byref(ms)), "timer")
    return ms.value


def solve_ms(sol, n, k, reps):
    import csparse as cs
    B = np.random.default_rng(k).uniform(-1, 1, (n, k))
    out = []
    for r in range(reps + 1):
        dB = cs.dvec(B)
        ms = event_ms(lambda: sol.solve(dB))
        if r:
            out.append(ms)
    return float(np.median(out))


def wall(fn):
    import _csx
    _csx.sync()
    t0 = time.perf_counter()
    out = fn()
    _csx.sync()
    return out, 1e3 * (time.perf_counter() - t0)


def gen1m(reps):
    import csparse as cs
    S = btf_oracle.reducible(btf_oracle.block_sizes(1_000_000, 11), 8, 11)[0]
    n = S.shape[0]
    S2 = sp.csc_matrix((S.data * (1.0 + 1e-3 * np.random.default_rng(31).uniform(-1, 1, S.nnz)), S.indices, S.indptr),
                       shape=S.shape)
    dA, dA2 = device(S), device(S2)
    sol = cs.btf_factor(dA)
    rec = {"matrix": "gen1m", "n": n, "nnz": int(S.nnz), "blocks": sol.info()["blocks"]}
    before = {k: solve_ms(sol, n, k, reps) for k in (1, 8, 128)}
    ok, first = wall(lambda: sol.refactor(dA2))
    assert ok
    rec["first_refactor_ms"] = first
    rec["refactor_info"] = sol.refactor_info()
    steady, fresh = [], []
    for r in range(reps + 1):
        a = dA if r % 2 == 0 else dA2
        ms = event_ms(lambda: sol.refactor(a))
        f, fms = wall(lambda: cs.btf_factor(a))
        del f
        if r:
            steady.append(ms)
            fresh.append(fms)
    # A2 as values in A's storage order: a numpy array (uploaded by the call) and a dvec (copied on the device); wall-clock
    for label, pair in (("numpy", (S.data.copy(), S2.data.copy())), ("dvec", (cs.dvec(S.data), cs.dvec(S2.data)))):
        t = []
        for r in range(reps + 1):
            ok, ms = wall(lambda: sol.refactor(pair[r % 2]))
            assert ok
            if r:
                t.append(ms)
        rec["steady_refactor_%s_ms" % label] = float(np.median(t))
    assert sol.refactor(dA2)
    after = {k: solve_ms(sol, n, k, reps) for k in (1, 8, 128)}
    rec["steady_refactor_ms"] = float(np.median(steady))
    rec["fresh_btf_factor_ms"] = float(np.median(fresh))
    rec["speedup"] = rec["fresh_btf_factor_ms"] / rec["steady_refactor_ms"]
    rec["solve_ms_before"] = before
    rec["solve_ms_after"] = after
    return rec


def w_matrix(nb, seed):
    from conftest import golden
    g = golden("west0067")
    bp, bi, bx = g["C_p"].astype(np.int64), g["C_i"].astype(np.int64), g["C_x"]
    u = synth.vec(nb, seed, 0.0, 1.0)
    Ai = (bi[None, :] + (np.arange(nb) * 67)[:, None]).reshape(-1)
    Ax = (bx[None, :] * (1.0 + 1e-3 * u)[:, None]).reshape(-1)
    Ap = np.concatenate([[0], np.cumsum(np.tile(np.diff(bp), nb))])
    return sp.csc_matrix((Ax, Ai, Ap), shape=(nb * 67, nb * 67))


def w(reps):
    import csparse as cs
    W, W2 = w_matrix(1493, 20240604), w_matrix(1493, 77)
    n = W.shape[0]
    dW, dW2 = device(W), device(W2)
    b = np.linspace(-1, 1, n)
    sol = cs.lusol_factor(dW, 0, 0.1)
    sol.solve(cs.dvec(b))
    assert sol.refactor(dW2)                        # the first refactor builds the plan: timed apart
    rec = {"matrix": "W", "n": n, "nnz": int(W.nnz), "first_refactor_ms": sol.refactor_info()["ms"]}
    ref, ref_solve, fresh, fresh_solve = [], [], [], []
    for r in range(reps + 1):
        a = dW if r % 2 == 0 else dW2
        ms = event_ms(lambda: sol.refactor(a))
        ms_solve = event_ms(lambda: sol.solve(cs.dvec(b)))
        f, fms = wall(lambda: cs.lusol_factor(a, 0, 0.1))
        fs = event_ms(lambda: f.solve(cs.dvec(b)))
        del f
        if r:
            ref.append(ms)
            ref_solve.append(ms_solve)
            fresh.append(fms)
            fresh_solve.append(fs)
    rec["refactor_info"] = sol.refactor_info()
    rec["steady_refactor_ms"] = float(np.median(ref))
    rec["first_solve_after_refactor_ms"] = float(np.median(ref_solve))
    rec["warm_solve_ms"] = solve_ms(sol, n, 1, reps)
    rec["fresh_lusol_factor_ms"] = float(np.median(fresh))
    rec["fresh_first_solve_ms"] = float(np.median(fresh_solve))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refactor_time.jsonl"))
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for fn in (gen1m, w):
        rec = fn(a.reps)
        rec["device"] = cs.device_name()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
