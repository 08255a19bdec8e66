#!/usr/bin/env python3
"""schur_factor against the only route to the same Schur complement without it.

    python tools/time_schur.py [--reps 3] [--out profiles/schur_time.jsonl] [--only line] [--grid 300]

Matrix: K - 3.7 I, K the five-point Laplacian on a g x g grid (g = 300), for two kept sets:
  line    the middle grid line (ns = g): two subdomains
  cross   the middle grid line and the middle grid column (ns = 2 g - 1): four
schur_factor at order 1: factor (host wall-clock around the call, analysis included, with the numeric kernels' own time from
info()["kernel_us"] beside it), refactor (new values A2 = D A D), condense and expand at k = 1 / 8 / 128 with the right-hand sides
on the device (hipEvents on the library's stream around the call).
Baseline, in the same run: ldlsol_factor(A11) at order 1, solve() of the ns columns of A12 as one n1-by-ns device block, then
S = A22 - A21 X by gaxpy_block with -A21 -- factor, solve and product timed apart and summed.  S of the two routes is compared
(normwise, reported).  Every figure is the median of --reps warm calls; one JSON line per kept set goes to --out; the ratios in
it are reported, not promised."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from time_chol_refactor import device, event_ms, grid, wall  # noqa: E402
from time_ldl import congruent, med  # noqa: E402

SIGMA = 3.7
BLOCKS = (1, 8, 128)


def kept(g, which):
    mid = g // 2
    line = [mid * g + c for c in range(g)]
    if which == "line":
        return line
    return line + [r * g + mid for r in range(g) if r != mid]


def time_schur(U, U2, keep, reps):
    import csparse as cs
    dA, dA2 = device(U), device(U2)
    n, ns = U.shape[0], len(keep)
    rec, fac, ker = {}, [], []
    for _ in range(reps + 1):
        sol, ms = wall(lambda: cs.schur_factor(dA, keep, 1))
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
    assert sol.refactor(dA)
    rec["refactor_ms"], rec["refactor_kernel_ms"] = med(ref[1:]), med(rker[1:])
    for k in BLOCKS:
        B = cs.dvec(np.random.default_rng(k).uniform(-1.0, 1.0, (n, k)))
        X2 = cs.dvec(np.random.default_rng(100 + k).uniform(-1.0, 1.0, (ns, k)))
        con, ex = [], []
        for _ in range(reps + 1):
            (g, state), ms = event_ms(lambda: sol.condense(B))
            con.append(ms)
            ex.append(event_ms(lambda: sol.expand(state, X2))[1])
        rec["condense_ms_k%d" % k], rec["expand_ms_k%d" % k] = med(con[1:]), med(ex[1:])
    i = sol.info()
    rec.update({k: i[k] for k in ("n1", "ns", "lnz", "levels", "launches", "level_launches", "run_launches", "schur_chunks",
                                  "long_columns", "neg", "max_abs_l")})
    return sol, rec


def time_baseline(S, keep, reps):
    """ldlsol_factor(A11), solve of the columns of A12, S = A22 - A21 X"""
    import csparse as cs
    n = S.shape[0]
    inside = np.ones(n, bool)
    inside[keep] = False
    interior = np.flatnonzero(inside)
    F = sp.csc_matrix(S + sp.triu(S, 1).T)
    A11 = sp.csc_matrix(sp.triu(F[interior][:, interior]))
    A11.sort_indices()
    A12 = np.ascontiguousarray(F[interior][:, keep].toarray())
    A21m = sp.csc_matrix(-F[keep][:, interior])
    A21m.sort_indices()
    A22 = np.ascontiguousarray(F[keep][:, keep].toarray())
    d11, d21, dB = device(A11), device(A21m), cs.dvec(A12)
    rec, fac, sol_ms, mul = {}, [], [], []
    Y = None
    for _ in range(reps + 1):
        sol, ms = wall(lambda: cs.ldlsol_factor(d11, 1))
        assert sol is not None
        fac.append(ms)
        X = dB.copy()
        sol_ms.append(event_ms(lambda: sol.solve(X))[1])
        Y = cs.dvec(A22)
        mul.append(event_ms(lambda: cs.gaxpy_block(d21, X, Y))[1])
    rec["factor_ms"], rec["solve_ms"], rec["product_ms"] = med(fac[1:]), med(sol_ms[1:]), med(mul[1:])
    rec["total_ms"] = rec["factor_ms"] + rec["solve_ms"] + rec["product_ms"]
    return rec, Y.numpy().reshape(len(keep), len(keep))


def measure(g, which, reps):
    K = grid(g)
    n = K.shape[0]
    S = sp.csc_matrix(K - SIGMA * sp.identity(n, format="csc"))
    S.sort_indices()
    keep = kept(g, which)
    rec = {"matrix": "grid%d" % g, "keep": which, "order": 1, "n": n, "sigma": SIGMA}
    sol, rec["schur"] = time_schur(S, congruent(S, 31), keep, reps)
    mine = sol.schur.numpy().reshape(len(keep), len(keep))
    rec["baseline"], theirs = time_baseline(S, keep, reps)
    rec["S_difference_1norm_relative"] = float(np.linalg.norm(mine - theirs, 1) / np.linalg.norm(theirs, 1))
    rec["baseline_over_schur"] = {"factor": rec["baseline"]["total_ms"] / rec["schur"]["factor_ms"],
                                  "refactor": rec["baseline"]["total_ms"] / rec["schur"]["refactor_ms"]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grid", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_time.jsonl"))
    ap.add_argument("--only", action="append", choices=["line", "cross"], help="run this kept set only (may be repeated)")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for which in (a.only or ["line", "cross"]):
        rec = measure(a.grid, which, a.reps)
        rec["device"] = cs.device_name()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
