#!/usr/bin/env python3
"""slusol_factor against lusol_factor on the same matrix, and against ldlsol_factor on its symmetric part.

    python tools/time_slu.py [--reps 3] [--lu-reps 1] [--out profiles/slu_time.jsonl] [--only plain] [--no-lu]

Matrix: convection-diffusion on the 300 x 300 grid (4 on the diagonal, -1 -+ 0.3 to the west / east, -1 north and south) at
order 1, plain and shifted by 3.7 (indefinite).
  slusol_factor  factor, refactor, solve at k = 1 / 8 / 128, refine at k = 8; host_rule_equal: L.x and Ut.x after the last
                 refactor byte-equal to csx_slu_host on the same pattern (one core, seconds).
  lusol_factor   the same matrix in the same run (factor, refactor, the same solves): the route without this solver.
  ldlsol_factor  the symmetric part (A + A') / 2 on the same pattern: factor and refactor, for the price of the second triangle.
New values are A2 = D A D, D = diag(1 + 1e-3 u).  Factors are host wall-clock around the call (analysis included), with the
numeric kernels' own time beside them (kernel_us); refactors, solves and refine are timed with hipEvents on the library's stream
around the call, the right-hand sides already on the device; every figure is the median of the warm calls (--reps; --lu-reps for
lusol_factor, whose factor takes tens of seconds).  One JSON line per matrix goes to --out; the ratios in it are reported, not
promised."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from time_chol_refactor import device, event_ms, wall  # noqa: E402
from time_ldl import congruent, med, solves  # noqa: E402

SIGMA, CONVECTION, GRID = 3.7, 0.3, 300


def convection_diffusion(g, sigma):
    n = g * g
    k = np.arange(n)
    west, north = k[k % g != 0], k[k >= g]
    rows = np.concatenate([k, west, west - 1, north, north - g])
    cols = np.concatenate([k, west - 1, west, north - g, north])
    vals = np.concatenate([np.full(n, 4.0 - sigma), np.full(len(west), -1.0 - CONVECTION), np.full(len(west), -1.0 + CONVECTION),
                           np.full(len(north), -1.0), np.full(len(north), -1.0)])
    A = sp.csc_matrix((vals, (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A


def host_rule_equal(sol, A):
    """L.x and Ut.x of the solver, as they stand, against csx_slu_host on the solver's own pattern and permutations with A's values"""
    import _csx
    f = sol.factors
    n, nnz = A.shape[0], sol.info()["lnz"]
    Lp, Li = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32)
    got = [np.empty(max(nnz, 1)), np.empty(max(nnz, 1))]
    for M, x in zip((f.L, f.U), got):
        _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(Lp), _csx.pi(Li), _csx.pd(x)), "csx_csc_download")
    Lx, Ux, info = np.zeros(max(nnz, 1)), np.zeros(max(nnz, 1)), (_csx.C.c_int64 * 4)()
    prow = None if f.prow is None else _csx.i32(f.prow)
    pinv = None if f.pinv is None else _csx.i32(f.pinv)
    _csx.check(_csx.load().csx_slu_host(n, _csx.pi(_csx.i32(A.indptr)), _csx.pi(_csx.i32(A.indices)), _csx.pd(_csx.f64(A.data)),
                                        _csx.pi(prow), _csx.pi(pinv), _csx.pi(Lp), _csx.pi(Li), 0.0, _csx.pd(Lx), _csx.pd(Ux), info),
               "csx_slu_host")
    return bool(info[3] == -1 and got[0].tobytes() == Lx.tobytes() and got[1].tobytes() == Ux.tobytes())


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


def measure(name, sigma, reps, lu_reps, with_lu):
    import csparse as cs
    A = convection_diffusion(GRID, sigma)
    A2 = congruent(A, 41)
    n = A.shape[0]
    rec = {"matrix": "convection-diffusion grid%d %s" % (GRID, name), "order": 1, "n": n, "sigma": sigma}
    sol, slu = time_factor(lambda d: cs.slusol_factor(d, 1), device(A), device(A2), reps,
                           ("lnz", "levels", "launches", "level_launches", "run_launches", "long_columns", "min_abs_d", "max_abs_d",
                            "max_abs_l", "max_abs_u", "neg", "perturbed"))
    slu["host_rule_equal"] = host_rule_equal(sol, A2 if reps % 2 == 0 else A)   # (the values of the last refactor)
    slu.update(solves(sol, n, reps))
    dB = cs.dvec(np.random.default_rng(8).uniform(-1.0, 1.0, (n, 8)))
    out, ms = None, []
    for _ in range(reps + 1):
        X = dB.copy()
        out, t = event_ms(lambda: sol.refine(X))
        ms.append(t)
    slu["refine_ms_k8"] = med(ms[1:])
    slu["refine_over_solve_k8"] = slu["refine_ms_k8"] / slu["solve_ms_k8"]
    slu["refine_omega0_eps"], slu["refine_omega_eps"] = float(out["omega0"].max() / 2.0 ** -52), float(out["omega"].max() / 2.0 ** -52)
    slu["refine_steps"] = int(out["steps"].max())
    rec["slusol"] = slu
    del sol
    # ---- the symmetric part on the same pattern: L D L' ----
    H, H2 = sp.csc_matrix(sp.triu((A + A.T) * 0.5)), sp.csc_matrix(sp.triu((A2 + A2.T) * 0.5))
    H.sort_indices()
    H2.sort_indices()
    sol, ldl = time_factor(lambda d: cs.ldlsol_factor(d, 1), device(H), device(H2), reps, ("lnz", "levels", "launches"))
    rec["ldlsol_symmetric_part"] = ldl
    rec["slu_over_ldl"] = {k: slu[k] / ldl[k] for k in ("factor_ms", "factor_kernel_ms", "refactor_ms", "refactor_kernel_ms")}
    del sol
    # ---- the pivoting LU of the same matrix ----
    if with_lu:
        dA, dA2 = device(A), device(A2)
        lu = {}
        sol, lu["factor_ms"] = wall(lambda: cs.lusol_factor(dA, 1))
        assert sol is not None
        ref = []
        for r in range(lu_reps + 1):
            ok, ms1 = event_ms(lambda: sol.refactor(dA2 if r % 2 == 0 else dA))
            assert ok
            ref.append(ms1)
        lu["refactor_ms"] = med(ref[1:])
        lu.update(solves(sol, n, reps))
        rec["lusol"] = lu
        rec["lu_over_slu"] = {k: lu[k] / slu[k] for k in lu}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lu-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slu_time.jsonl"))
    ap.add_argument("--only", action="append", choices=["plain", "shifted"], help="run this matrix only (may be repeated)")
    ap.add_argument("--no-lu", action="store_true", help="leave lusol_factor out")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for name in (a.only or ["plain", "shifted"]):
        rec = measure(name, SIGMA if name == "shifted" else 0.0, a.reps, a.lu_reps, not a.no_lu)
        rec["device"] = cs.device_name()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
