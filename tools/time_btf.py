#!/usr/bin/env python3
"""btf_factor: factor steps and solve times, with lusol_factor and scipy's splu as baselines.

    python tools/time_btf.py [--reps 5] [--limit S] [--only NAME,...]

Matrices: a generated reducible matrix of 1M rows (more than 100 000 strongly connected blocks of 1 to 64 rows, 8
levels; tests/test_gpu_btf.py's scale test), the natural-order block lower bidiagonal chain of 20 000 2 x 2 blocks
(one level per block) and an irreducible matrix (a 20 000-row tridiagonal with a corner entry closing the cycle).
Factor steps are host wall-clock (every step ends with a copy to the host); a solve is the median of --reps warm
calls timed with hipEvents on the library's stream.  The baselines run in child processes and are recorded as
"limit" when they take longer than --limit seconds.  One JSON line per matrix goes to profiles/btf_time.jsonl."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]

import btf_oracle  # noqa: E402

PEAK = 8e12


def matrix(name):
    if name == "gen1m":
        return btf_oracle.reducible(btf_oracle.block_sizes(1_000_000, 11), 8, 11)[0]
    if name == "chain20k":
        nbk = 20000
        rows, cols, vals = [], [], []
        a = 2 * np.arange(nbk)
        rows = np.concatenate([a, a + 1, a, a + 1, a[1:]])
        cols = np.concatenate([a, a, a + 1, a + 1, a[1:] - 1])
        vals = np.concatenate([np.full(nbk, 4.0), np.ones(nbk), np.ones(nbk), np.full(nbk, 5.0), -np.ones(nbk - 1)])
        return sp.csc_matrix((vals, (rows, cols)), shape=(2 * nbk, 2 * nbk))
    if name == "irreducible20k":
        n = 20000
        S = sp.diags([np.full(n - 1, -1.0), np.full(n, 4.0), np.full(n - 1, -1.0)], [-1, 0, 1], format="lil")
        S[0, n - 1] = -1.0
        return S.tocsc()
    raise ValueError(name)


def device(S):
    import _csx
    import csparse as cs
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(S.shape[0], S.shape[1], _csx.pi(_csx.i32(S.indptr)), _csx.pi(_csx.i32(S.indices)),
                                         _csx.pd(_csx.f64(S.data)), h), "upload")
    return cs._from_device(h, lambda nnz: max(nnz, 1))


def timed_solves(solve, n, k, reps):
    import _csx
    import csparse as cs
    B = np.random.default_rng(k).uniform(-1, 1, (n, k))
    out = []
    for r in range(reps + 1):
        dB = cs.dvec(B)
        _csx.sync()
        _csx.check(_csx.lib().csx_timer_start(), "timer")
        solve(dB)
        ms = _csx.C.c_double(0)
        _csx.check(_csx.lib().csx_timer_stop(_csx.C.byref(ms)), "timer")
        if r:
            out.append(ms.value)
    return float(np.median(out))


def child(kind, name, reps):
    """One baseline in this (child) process; prints one JSON line."""
    import time
    S = matrix(name)
    n = S.shape[0]
    if kind == "splu":
        from scipy.sparse.linalg import splu
        t0 = time.perf_counter()
        lu = splu(S.tocsc(), permc_spec="NATURAL")
        f = time.perf_counter() - t0
        res = {"factor_ms": 1e3 * f}
        for k in (1, 8, 128):
            B = np.random.default_rng(k).uniform(-1, 1, (n, k))
            t0 = time.perf_counter()
            lu.solve(B)
            res["solve_ms_k%d" % k] = 1e3 * (time.perf_counter() - t0)
    else:
        import _csx
        import csparse as cs
        _csx.init(0)
        A = device(S)
        t0 = time.perf_counter()
        sol = cs.lusol_factor(A)
        res = {"factor_ms": 1e3 * (time.perf_counter() - t0)}
        for k in (1, 8, 128):
            res["solve_ms_k%d" % k] = timed_solves(sol.solve, n, k, reps)
    print(json.dumps(res))


def baseline(kind, name, reps, limit):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--only", name, "--reps", str(reps)],
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return {"status": "limit", "limit_s": limit}
    if r.returncode != 0:
        return {"status": "error", "rc": r.returncode, "tail": r.stderr[-400:]}
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out["status"] = "ok"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--only", default="gen1m,chain20k,irreducible20k")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.only, a.reps)
        return
    import _csx
    import csparse as cs
    _csx.init(0)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out_path = os.path.join(ROOT, "profiles", "btf_time.jsonl")
    with open(out_path, "w") as fout:
        for name in a.only.split(","):
            S = matrix(name)
            n = S.shape[0]
            A = device(S)
            cs.btf_factor(A)                  # warm-up: code objects, allocator
            sol = cs.btf_factor(A)
            info = sol.info()
            rec = {"matrix": name, "n": n, "nnz": int(S.nnz), "info": info, "factor_ms": sol.factor_ms}
            for k in (1, 8, 128):
                ms = timed_solves(sol.solve, n, k, a.reps)
                # algorithmic bytes: 12 per entry of L, U, F (value + index), b read and x written once
                # (16 n k), p, q, pinv and the three row pointers (24 n)
                nbytes = 12 * (info["lnz"] + info["unz"] + info["fnz"]) + 16 * n * k + 24 * n
                rec["solve_ms_k%d" % k] = ms
                rec["peak_frac_k%d" % k] = nbytes / (ms * 1e-3) / PEAK
            rec["launches_per_solve"] = info["launches"]
            rec["lusol_factor"] = baseline("lusol", name, a.reps, a.limit)
            rec["scipy_splu_natural"] = baseline("splu", name, a.reps, a.limit)
            line = json.dumps(rec)
            print(line, flush=True)
            fout.write(line + "\n")


if __name__ == "__main__":
    main()
