#!/usr/bin/env python3
"""ldlsol_factor against what a symmetric indefinite system needs today, and against cholsol_factor.

    python tools/time_ldl.py [--reps 3] [--out profiles/ldl_time.jsonl] [--only grid300] [--no-lu]

Matrices: the five-point Laplacian K on a 300 x 300 and a 700 x 700 grid at order 1.
  shifted   K - 3.7 I (indefinite): ldlsol_factor -- factor, refactor, solve at k = 1 / 8 / 128, refine at k = 8 -- against
            lusol_factor on the same matrix in full storage (factor, refactor, the same solves): the route without this solver.
  spd       K itself: ldlsol_factor's factor and refactor against cholsol_factor's: the price of having no supernodes or bands.
New values are A2 = D A D, D = diag(1 + 1e-3 u).  Factors are host wall-clock around the call (analysis included), with the
numeric kernels' own time beside them (csx_ldl_info's kernel_us, csx_chol_info's numeric_ms); refactors, solves and refine are
timed with hipEvents on the library's stream around the call, the right-hand sides already on the device (a solve under an
ordering still allocates its permuted block inside the call); every figure is the median of --reps warm calls.  One JSON line
per matrix goes to --out; the ratios in it are reported, not promised."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from time_chol_refactor import device, event_ms, grid, wall  # noqa: E402

SIGMA = 3.7
BLOCKS = (1, 8, 128)


def med(v):
    return float(np.median(v))


def congruent(S, seed):
    n = S.shape[0]
    d = 1.0 + 1e-3 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)
    cols = np.repeat(np.arange(n), np.diff(S.indptr))
    return sp.csc_matrix((d[S.indices] * S.data * d[cols], S.indices.copy(), S.indptr.copy()), shape=S.shape)


def full(U):
    F = sp.csc_matrix(U + sp.triu(U, 1).T)
    F.sort_indices()
    return F


def solves(sol, n, reps):
    import csparse as cs
    out = {}
    for k in BLOCKS:
        B = cs.dvec(np.random.default_rng(k).uniform(-1.0, 1.0, (n, k)))
        ms = []
        for _ in range(reps + 1):
            X = B.copy()                                  # on the device, outside the timed region
            ms.append(event_ms(lambda: sol.solve(X))[1])
        out["solve_ms_k%d" % k] = med(ms[1:])
    return out


def time_ldl(U, U2, reps):
    import csparse as cs
    dA, dA2 = device(U), device(U2)
    n = U.shape[0]
    rec, fac, ker = {}, [], []
    for _ in range(reps + 1):
        sol, ms = wall(lambda: cs.ldlsol_factor(dA, 1))
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
    rec.update({k: i[k] for k in ("lnz", "levels", "launches", "level_launches", "run_launches", "long_columns", "neg", "max_abs_l")})
    return sol, rec


def measure(g, reps, with_lu):
    import csparse as cs
    K = grid(g)
    n = K.shape[0]
    S = sp.csc_matrix(K - SIGMA * sp.identity(n, format="csc"))
    S.sort_indices()
    rec = {"matrix": "grid%d" % g, "order": 1, "n": n, "sigma": SIGMA}
    # ---- shifted: LDL' ----
    sol, ldl = time_ldl(S, congruent(S, 31), reps)
    ldl.update(solves(sol, n, reps))
    B = np.random.default_rng(8).uniform(-1.0, 1.0, (n, 8))
    out = None
    ms = []
    dB = cs.dvec(B)
    for _ in range(reps + 1):
        X = dB.copy()
        out, t = event_ms(lambda: sol.refine(X))
        ms.append(t)
    ldl["refine_ms_k8"] = med(ms[1:])
    ldl["refine_over_solve_k8"] = ldl["refine_ms_k8"] / ldl["solve_ms_k8"]
    ldl["refine_omega0_eps"], ldl["refine_omega_eps"] = float(out["omega0"].max() / 2.0 ** -52), float(out["omega"].max() / 2.0 ** -52)
    ldl["refine_steps"] = int(out["steps"].max())
    rec["ldl_shifted"] = ldl
    del sol
    # ---- shifted: LU on the full matrix ----
    if with_lu:
        F, F2 = full(S), full(congruent(S, 31))
        dF, dF2 = device(F), device(F2)
        lu = {}
        sol, lu["factor_ms"] = wall(lambda: cs.lusol_factor(dF, 1))
        assert sol is not None
        ref = []
        for r in range(reps + 1):
            ok, ms1 = event_ms(lambda: sol.refactor(dF2 if r % 2 == 0 else dF))
            assert ok
            ref.append(ms1)
        lu["refactor_ms"] = med(ref[1:])
        lu.update(solves(sol, n, reps))
        rec["lusol_shifted"] = lu
        rec["lu_over_ldl"] = {k: lu[k] / ldl[k] for k in lu}
        del sol
    # ---- unshifted SPD: LDL' against Cholesky ----
    sol, spd = time_ldl(K, congruent(K, 32), reps)
    rec["ldl_spd"] = spd
    del sol
    dK, dK2 = device(K), device(congruent(K, 32))
    ch, fac, num = {}, [], []
    for _ in range(reps + 1):
        sol, ms1 = wall(lambda: cs.cholsol_factor(dK, 1))
        fac.append(ms1)
    ch["factor_ms"] = med(fac[1:])
    ref = []
    for r in range(reps + 2):
        ok, ms1 = event_ms(lambda: sol.refactor(dK2 if r % 2 == 0 else dK))
        assert ok
        ref.append(ms1)
        num.append(sol.refactor_info()["numeric_ms"])
    ch["refactor_ms"], ch["refactor_numeric_ms"] = med(ref[2:]), med(num[2:])      # (the first refactor makes the plan)
    rec["cholsol_spd"] = ch
    rec["ldl_over_chol"] = {"factor_ms": spd["factor_ms"] / ch["factor_ms"], "refactor_ms": spd["refactor_ms"] / ch["refactor_ms"],
                            "numeric_ms": spd["refactor_kernel_ms"] / ch["refactor_numeric_ms"]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldl_time.jsonl"))
    ap.add_argument("--only", action="append", choices=["grid300", "grid700"], help="run this matrix only (may be repeated)")
    ap.add_argument("--no-lu", action="store_true", help="leave lusol_factor out")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for name in (a.only or ["grid300", "grid700"]):
        rec = measure(int(name[4:]), a.reps, not a.no_lu)
        rec["device"] = cs.device_name()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
