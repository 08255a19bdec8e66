#!/usr/bin/env python3
"""hqrsol_factor(...).batch() against B calls of refactor(), and its solves against B single solves.

    python tools/time_hqr_batch.py [--grid 100] [--tall-grid G] [--reps 2] [--out profiles/hqr_batch_time.jsonl]
                                   [--members 1,8,64] [--only plain]

Matrices: tools/time_hqr.py's convection-diffusion grids at order 3, `plain` (g^2 x g^2) and `stacked` (the shifted grid with the
plain one under it, 2 g^2 x g^2: least squares).  Member m has the values D1 A D2, D = diag(1 + 1e-3 u) from seed 41 + m.  For
every B:
  batch_refactor_ms   one batch.refactor(V) of all B members, V on the device (median of the warm calls), with the kernels' own
                      time beside it (batch_kernel_ms: the whole walk between two events)
  single_refactor_ms  B calls of the single factor's refactor(), one per member, values on the device, in the same run (one
                      pass, after a warm call), with the sum of their kernel times
  solve_*_r1 / _r8    batch.solve of an m x (B r) block against B solves of m x r blocks on the single factor refactored to the
                      last member (the same work per member; its last block must equal the batch's last member byte for byte)
  launches            level and walker launches of the batch's run and of one single refactor (equal by construction), and the
                      kernel launches of one batched solve
All times are host wall-clock around the call with the device synchronised before and after, so the host's share of a call is
in both sides.  One JSON line per (matrix, B) goes to --out; the ratios in it are reported, not promised, and a loss is reported
as a loss."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from time_chol_refactor import device, wall  # noqa: E402
from time_hqr import scaled  # noqa: E402
from time_ldl import med  # noqa: E402
from time_slu import SIGMA, convection_diffusion  # noqa: E402
from time_slu_batch import values_of  # noqa: E402

MEMORY_CAP = 16e9
SOLVE_R = (1, 8)


def matrix(name, g):
    if name == "plain":
        return convection_diffusion(g, 0.0)
    A = sp.csc_matrix(sp.vstack([convection_diffusion(g, SIGMA), convection_diffusion(g, 0.0)]))
    A.sort_indices()
    return A


def measure(name, g, members, reps):
    import csparse as cs
    A = matrix(name, g)
    m, n = A.shape
    sol = cs.hqrsol_factor(device(A), 3)
    assert sol is not None
    i0 = sol.info()
    rng = np.random.default_rng(8)
    for B in members:
        while B > 1 and 1.0 * B * (i0["vnz"] + i0["rnz"]) * 8 > MEMORY_CAP:
            B //= 2
        rec = {"matrix": "convection-diffusion grid%d %s" % (g, name), "order": 3, "m": m, "n": n, "vnz": i0["vnz"],
               "rnz": i0["rnz"], "levels": i0["levels"], "B": B}
        vals = [scaled(A, 41 + k).data for k in range(B)]
        dV = cs.dvec(np.ascontiguousarray(np.stack(vals, axis=1)))
        dv = [cs.dvec(v) for v in vals]
        # ---- B single refactors, one pass after a warm call ----
        assert sol.refactor(dv[0])
        one, ker = [], []
        for k in range(B):
            ok, ms = wall(lambda: sol.refactor(dv[k]))
            assert ok
            one.append(ms)
            ker.append(sol.info()["kernel_us"] / 1e3)
        single = sol.info()
        rec["single_refactor_ms"], rec["single_kernel_ms"], rec["one_refactor_ms"] = float(np.sum(one)), float(np.sum(ker)), med(one)
        # ---- the batch ----
        batch, first = wall(lambda: sol.batch(dV))
        assert batch.ok.all()
        rec["batch_factor_ms"] = first
        t, k_ = [], []
        for _ in range(reps + 1):
            ok, ms = wall(lambda: batch.refactor(dV))
            assert ok.all()
            t.append(ms)
            k_.append(batch.info()["kernel_us"] / 1e3)
        rec["batch_refactor_ms"], rec["batch_kernel_ms"] = med(t[1:]), med(k_[1:])
        rec["batch_over_single"] = rec["batch_refactor_ms"] / rec["single_refactor_ms"]
        rec["batch_over_single_kernels"] = rec["batch_kernel_ms"] / rec["single_kernel_ms"]
        i = batch.info()
        rec["launches"] = {"batch_level": i["level_launches"], "batch_walker": i["run_launches"],
                           "single_level": single["level_launches"], "single_walker": single["run_launches"]}
        Vx, Rx, beta = batch.member(B - 1)
        f = sol.factors                                            # (the single factor holds the last member's values)
        rec["last_member_equal"] = bool(values_of(f.L).tobytes() == Vx.tobytes() and values_of(f.U).tobytes() == Rx.tobytes()
                                        and np.asarray(f.B).tobytes() == beta.tobytes())
        # ---- solves ----
        for r in SOLVE_R:
            X = rng.uniform(-1.0, 1.0, (m, B * r))
            dX = cs.dvec(X)
            t, out = [], None
            for _ in range(reps + 1):
                out, ms = wall(lambda: batch.solve(dX))
                t.append(ms)
            rec["solve_batch_ms_r%d" % r] = med(t[1:])
            rec["launches"]["batch_solve_r%d" % r] = batch.info()["solve_launches"]
            blocks = [cs.dvec(np.ascontiguousarray(X[:, k * r:(k + 1) * r])) for k in range(B)]
            sol.solve(blocks[0])                                   # warm: the plans of the new values
            res = [wall(lambda: sol.solve(blocks[k])) for k in range(B)]
            rec["solve_single_ms_r%d" % r] = float(np.sum([ms for _, ms in res]))
            rec["solve_batch_over_single_r%d" % r] = rec["solve_batch_ms_r%d" % r] / rec["solve_single_ms_r%d" % r]
            last = out.numpy().reshape(n, B * r)[:, (B - 1) * r:]
            rec["solve_last_member_equal_r%d" % r] = bool(last.tobytes() == res[B - 1][0].numpy().reshape(n, r).tobytes())
        del batch, dV, dv
        yield rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--tall-grid", type=int, default=None, help="grid of the stacked case (default: --grid)")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hqr_batch_time.jsonl"))
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--only", action="append", choices=["plain", "stacked"], help="run this matrix only (may be repeated)")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for name in (a.only or ["plain", "stacked"]):
        g = a.tall_grid if name == "stacked" and a.tall_grid else a.grid
        for rec in measure(name, g, [int(b) for b in a.members.split(",")], a.reps):
            rec["device"] = cs.device_name()
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
