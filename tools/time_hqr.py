#!/usr/bin/env python3
"""hqrsol_factor against the host QR loop on the same analysis, and against slusol_factor and lusol_factor on the square
matrix.

    python tools/time_hqr.py [--grid 300] [--tall-grid G] [--reps 3] [--out profiles/hqr_time.jsonl] [--only plain] [--no-lu] [--no-host]

Matrices: convection-diffusion on the g x g grid (4 on the diagonal, -1 -+ 0.3 to the west / east, -1 north and south) at
order 3, `plain` and `shifted` by 3.7; `tall`: the shifted grid with the plain one stacked under it (2 g^2 x g^2, least squares).
  hqrsol_factor  factor, refactor, solve at k = 1 / 8 / 128, refine at k = 8 (square matrices); fill: entries of V and of R
                 against the Cholesky pattern of A + A' that slusol_factor factors on (order 1).
  csx_qr_host    the host loop (what cs_qr runs for a connected matrix) on the solver's own analysis, one core, in the same run.
  slusol_factor, lusol_factor   the square matrix in the same run (order 1): factor, refactor, the same solves.
New values are A2 = D1 A D2, D = diag(1 + 1e-3 u).  Factors are host wall-clock around the call (analysis included), with the
numeric kernels' own time beside them (kernel_us); refactors, solves and refine are timed with events on the library's stream,
the right-hand sides already on the device; every figure is the median of the warm calls.  One JSON line per matrix goes to
--out; the ratios in it are reported, not promised, and a loss is reported as a loss."""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from time_chol_refactor import device, event_ms, wall  # noqa: E402
from time_ldl import med  # noqa: E402
from time_slu import CONVECTION, SIGMA, convection_diffusion  # noqa: E402,F401

BLOCKS = (1, 8, 128)


def scaled(A, seed):
    rng = np.random.default_rng(seed)
    d1 = 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, A.shape[0])
    d2 = 1.0 + 1e-3 * rng.uniform(-1.0, 1.0, A.shape[1])
    cols = np.repeat(np.arange(A.shape[1]), np.diff(A.indptr))
    return sp.csc_matrix((d1[A.indices] * A.data * d2[cols], A.indices.copy(), A.indptr.copy()), shape=A.shape)


def solves(sol, rows, reps):
    import csparse as cs
    out = {}
    for k in BLOCKS:
        B = cs.dvec(np.random.default_rng(k).uniform(-1.0, 1.0, (rows, k)))
        ms = []
        for _ in range(reps + 1):
            X = B.copy()                                  # on the device, outside the timed region
            ms.append(event_ms(lambda: sol.solve(X))[1])
        out["solve_ms_k%d" % k] = med(ms[1:])
    return out


def time_factor(make, dA, dA2, reps, keys):
    rec, fac, ker = {}, [], []
    for _ in range(reps + 1):
        sol, ms = wall(lambda: make(dA))
        assert sol is not None
        fac.append(ms)
        ker.append(sol.info()["kernel_us"] / 1e3)
    rec["factor_ms"], rec["factor_kernel_ms"] = med(fac[1:]), med(ker[1:])
    ref, rker = [], []
    for r in range(reps + 1):
        ok, ms = event_ms(lambda: sol.refactor(dA2 if r % 2 == 0 else dA))
        assert ok
        ref.append(ms)
        rker.append(sol.info()["kernel_us"] / 1e3)
    rec["refactor_ms"], rec["refactor_kernel_ms"] = med(ref[1:]), med(rker[1:])
    i = sol.info()
    rec.update({k: i[k] for k in keys})
    return sol, rec


def host_loop(sol, A):
    """csx_qr_host on the solver's own analysis with A's values: (wall ms, max |R.x - the device's| / max |R.x|)"""
    import _csx
    S, i = sol.symbolic, sol.info()
    n, vnz, rnz = i["n"], i["vnz"], i["rnz"]
    Vp, Rp = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    Vi, Ri, Vx, Rx, beta = np.zeros(vnz, np.int32), np.zeros(rnz, np.int32), np.zeros(vnz), np.zeros(rnz), np.zeros(n)
    q = None if S.q is None else _csx.i32(S.q)
    args = (i["m"], n, i["m2"], _csx.pi(_csx.i32(A.indptr)), _csx.pi(_csx.i32(A.indices)), _csx.pd(_csx.f64(A.data)), _csx.pi(q),
            _csx.pi(_csx.i32(S.parent)), _csx.pi(_csx.i32(S.pinv)), _csx.pi(_csx.i32(S.leftmost)), vnz, rnz, _csx.pi(Vp), _csx.pi(Vi),
            _csx.pd(Vx), _csx.pi(Rp), _csx.pi(Ri), _csx.pd(Rx), _csx.pd(beta))
    t0 = time.perf_counter()
    _csx.check(_csx.load().csx_qr_host(*args), "csx_qr_host")
    ms = 1e3 * (time.perf_counter() - t0)
    got = np.empty(rnz)
    _csx.check(_csx.lib().csx_csc_download(sol.factors.U._dev.handle, None, None, _csx.pd(got)), "csx_csc_download")
    return ms, float(np.max(np.abs(got - Rx)) / np.max(np.abs(Rx)))


def measure(name, g, reps, with_lu, with_host):
    import csparse as cs
    square = name != "tall"
    A = convection_diffusion(g, 0.0 if name == "plain" else SIGMA)
    if not square:
        A = sp.csc_matrix(sp.vstack([A, convection_diffusion(g, 0.0)]))
        A.sort_indices()
    A2 = scaled(A, 41)
    m, n = A.shape
    rec = {"matrix": "convection-diffusion grid%d %s" % (g, name), "order": 3, "m": m, "n": n}
    sol, hqr = time_factor(lambda d: cs.hqrsol_factor(d, 3), device(A), device(A2), reps,
                           ("vnz", "rnz", "levels", "launches", "level_launches", "run_launches", "long_columns", "zero_diagonals",
                            "min_abs_r", "max_abs_r"))
    hqr.update(solves(sol, m, reps))
    if square:
        dB = cs.dvec(np.random.default_rng(8).uniform(-1.0, 1.0, (n, 8)))
        out, ms = None, []
        for _ in range(reps + 1):
            X = dB.copy()
            out, t = event_ms(lambda: sol.refine(X))
            ms.append(t)
        hqr["refine_ms_k8"] = med(ms[1:])
        hqr["refine_over_solve_k8"] = hqr["refine_ms_k8"] / hqr["solve_ms_k8"]
        hqr["refine_omega0_eps"], hqr["refine_omega_eps"] = float(out["omega0"].max() / 2.0 ** -52), float(out["omega"].max() / 2.0 ** -52)
        hqr["refine_steps"] = int(out["steps"].max())
    rec["hqrsol"] = hqr
    if with_host:
        ms, diff = host_loop(sol, A2 if reps % 2 == 0 else A)        # (the values of the last refactor)
        rec["qr_host"] = {"factor_ms": ms, "max_rel_diff_R": diff}
        rec["qr_host_over_hqr"] = {"numeric": ms / hqr["refactor_ms"]}
    del sol
    if square:
        dA, dA2 = device(A), device(A2)
        sol, slu = time_factor(lambda d: cs.slusol_factor(d, 1), dA, dA2, reps, ("lnz", "levels", "launches", "max_abs_l"))
        slu.update(solves(sol, n, reps))
        rec["slusol"] = slu
        rec["hqr_over_slu"] = {k: hqr[k] / slu[k] for k in slu if k.endswith("_ms") or "_ms_" in k}
        rec["fill"] = {"R_over_chol": hqr["rnz"] / slu["lnz"], "V_plus_R_over_L_plus_U": (hqr["vnz"] + hqr["rnz"]) / (2.0 * slu["lnz"])}
        del sol
        if with_lu:
            lu = {}
            sol, lu["factor_ms"] = wall(lambda: cs.lusol_factor(dA, 1))
            assert sol is not None
            ok, lu["refactor_ms"] = event_ms(lambda: sol.refactor(dA2))
            assert ok
            lu.update(solves(sol, n, reps))
            rec["lusol"] = lu
            rec["lu_over_hqr"] = {k: lu[k] / hqr[k] for k in lu}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--tall-grid", type=int, default=None, help="grid of the tall case (default: --grid)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hqr_time.jsonl"))
    ap.add_argument("--only", action="append", choices=["plain", "shifted", "tall"], help="run this matrix only (may be repeated)")
    ap.add_argument("--no-lu", action="store_true", help="leave lusol_factor out")
    ap.add_argument("--no-host", action="store_true", help="leave csx_qr_host out")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for name in (a.only or ["plain", "shifted", "tall"]):
        rec = measure(name, a.tall_grid if name == "tall" and a.tall_grid else a.grid, a.reps, not a.no_lu, not a.no_host)
        rec["device"] = cs.device_name()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
