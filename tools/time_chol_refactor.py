#!/usr/bin/env python3
"""refactor() of cholsol_factor against a fresh factor.

    python tools/time_chol_refactor.py [--reps 5] [--out profiles/chol_refactor_time.jsonl] [--only NAME]

Matrices: the five-point Laplacian on a 300 x 300 and a 700 x 700 grid at order 1; bcsstk16 (tests/golden) at orders 0 and 1; the
block-SPD matrix of the benchmark (csx_gen_gspd: 78 125 dense blocks of 64, 5M rows: the forest route).  New values are
A2 = D A D + 1e-3 diag(A), D = diag(1 + 1e-3 u): positive definite whatever A's condition number (the 5M-row matrix: A2 =
1.0005 A, made on the device).
Per matrix: the first refactor (the plan is made there); a steady refactor, A2 and A alternated, given as a device-resident
matrix and as a dvec of values; the first solve after a refactor, apart (the solve plan is rebuilt there); a fresh
cholsol_factor(A2, order) with its first solve, and csx_chol_info's numeric_ms of that fresh factor.
A refactor or a solve is timed with hipEvents on the library's stream around the call (the calls synchronise), the median of
--reps warm calls; factors are host wall-clock.  One JSON line per matrix goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]


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
    out = fn()
    ms = _csx.C.c_double(0)
    _csx.check(_csx.lib().csx_timer_stop(_csx.C.byref(ms)), "timer")
    return out, ms.value


def wall(fn):
    import _csx
    _csx.sync()
    t0 = time.perf_counter()
    out = fn()
    _csx.sync()
    return out, 1e3 * (time.perf_counter() - t0)


def congruent(S, seed):
    """D S D + 1e-3 diag(S) on S's stored entries"""
    n = S.shape[0]
    d = 1.0 + 1e-3 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    cols = np.repeat(np.arange(n), np.diff(S.indptr))
    x = d[S.indices] * S.data * d[cols]
    diag = S.indices == cols
    x[diag] += 1e-3 * S.data[diag]
    return sp.csc_matrix((x, S.indices.copy(), S.indptr.copy()), shape=S.shape)


def grid(g):
    """upper triangle of the five-point Laplacian on a g x g grid"""
    n = g * g
    j = np.arange(n)
    east = j[(j % g) != 0]
    north = j[j >= g]
    rows = np.concatenate([j, east - 1, north - g])
    cols = np.concatenate([j, east, north])
    vals = np.concatenate([np.full(n, 4.0), np.full(len(east), -1.0), np.full(len(north), -1.0)])
    S = sp.csc_matrix((vals, (rows, cols)), shape=(n, n))
    S.sort_indices()
    return S


def bcsstk16():
    from conftest import golden
    g = golden("bcsstk16")
    n = int(g["C_mn"][1])
    p = g["C_p"].astype(np.int64)
    return sp.csc_matrix((g["C_x"][:p[n]], g["C_i"][:p[n]], p), shape=(n, n))


def chol_numeric_ms():
    import _csx
    path, ms = _csx.C.c_int32(-1), _csx.C.c_double(0.0)
    _csx.check(_csx.lib().csx_chol_info(path, ms), "csx_chol_info")
    return path.value, ms.value


def measure(name, dA, dA2, values, order, reps):
    """dA, dA2: device-resident `cs`; values: (A's, A2's) value arrays, or None to read them off the device matrices"""
    import _csx
    import csparse as cs
    n = dA.n
    b = np.linspace(-1.0, 1.0, n)
    rec = {"matrix": name, "order": order, "n": n, "nnz": int(dA._dev.info()[2])}
    sol, rec["factor_ms"] = wall(lambda: cs.cholsol_factor(dA, order))
    rec["lnz"] = int(sol.L._dev.info()[2])
    _, rec["factor_first_solve_ms"] = event_ms(lambda: sol.solve(cs.dvec(b)))
    ok, rec["first_refactor_ms"] = wall(lambda: sol.refactor(dA2))
    assert ok
    rec["first_refactor_info"] = sol.refactor_info()
    steady, numeric, resolve, warm, fresh, fresh_solve, fresh_numeric = [], [], [], [], [], [], []
    for r in range(reps + 1):
        a = dA if r % 2 == 0 else dA2
        ok, ms = event_ms(lambda: sol.refactor(a))
        assert ok
        num = sol.refactor_info()["numeric_ms"]
        _, rs = event_ms(lambda: sol.solve(cs.dvec(b)))        # the solve plan is rebuilt here
        _, ws = event_ms(lambda: sol.solve(cs.dvec(b)))
        f, fms = wall(lambda: cs.cholsol_factor(a, order))
        fnum = chol_numeric_ms()
        _, fs = event_ms(lambda: f.solve(cs.dvec(b)))
        del f
        if r:
            steady.append(ms)
            numeric.append(num)
            resolve.append(rs)
            warm.append(ws)
            fresh.append(fms)
            fresh_solve.append(fs)
            fresh_numeric.append(fnum[1])
            rec["fresh_chol_path"] = fnum[0]
    if values is None:
        def vals(d):
            x = np.empty(rec["nnz"], np.float64)
            _csx.check(_csx.lib().csx_csc_download(d._dev.handle, None, None, _csx.pd(x)), "csx_csc_download")
            return x
        values = (vals(dA), vals(dA2))
    pair = (cs.dvec(values[0]), cs.dvec(values[1]))
    as_dvec = []
    for r in range(reps + 1):
        ok, ms = event_ms(lambda: sol.refactor(pair[r % 2]))
        assert ok
        if r:
            as_dvec.append(ms)
    med = lambda v: float(np.median(v))   # noqa: E731
    rec["refactor_info"] = sol.refactor_info()
    rec["steady_refactor_ms"] = med(steady)
    rec["steady_refactor_numeric_ms"] = med(numeric)
    rec["steady_refactor_dvec_ms"] = med(as_dvec)
    rec["first_solve_after_refactor_ms"] = med(resolve)
    rec["warm_solve_ms"] = med(warm)
    rec["fresh_cholsol_factor_ms"] = med(fresh)
    rec["fresh_first_solve_ms"] = med(fresh_solve)
    rec["fresh_chol_numeric_ms"] = med(fresh_numeric)
    rec["fresh_over_refactor"] = rec["fresh_cholsol_factor_ms"] / rec["steady_refactor_ms"]
    return rec


def case_scipy(name, S, order, reps):
    S2 = congruent(S, 31)
    return measure(name, device(S), device(S2), (S.data, S2.data), order, reps)


def case_gspd(reps):
    """the benchmark's block-SPD matrix, made on the device; A2 = 1.0005 A by cs_add on the device (same pattern, SPD): 320M
    entries never visit the host except as the two value vectors of the dvec form"""
    import _csx
    import csparse as cs
    nb, bs = 78125, 64
    hA = _csx.new_handle()
    _csx.check(_csx.lib().csx_gen_gspd(nb, bs, 20240601 + 5, hA), "gen_gspd")
    dA = cs.cs_pin(cs._from_device(hA, lambda nnz: max(nnz, 1)))
    dA2 = cs.cs_pin(cs.cs_add(dA, dA, 0.5, 0.5005))
    return measure("gspd-5M", dA, dA2, None, 0, reps)


CASES = {
    "grid300": lambda reps: case_scipy("grid300", grid(300), 1, reps),
    "grid700": lambda reps: case_scipy("grid700", grid(700), 1, reps),
    "bcsstk16-natural": lambda reps: case_scipy("bcsstk16", bcsstk16(), 0, reps),
    "bcsstk16-ordered": lambda reps: case_scipy("bcsstk16", bcsstk16(), 1, reps),
    "gspd-5M": case_gspd,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chol_refactor_time.jsonl"))
    ap.add_argument("--only", action="append", choices=sorted(CASES), help="run this case only (may be repeated)")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for name in (a.only or list(CASES)):
        rec = CASES[name](a.reps)
        rec["device"] = cs.device_name()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
