#!/usr/bin/env python3
"""ldlsol_factor(...).batch() against B calls of refactor(), and its solves against B single exact solves.

    python tools/time_ldl_batch.py [--reps 2] [--out profiles/ldl_batch_time.jsonl] [--members 1,8,64] [--no-d-pass]

Matrix: tools/time_ldl.py's K - 3.7 I of the five-point Laplacian on the 300 x 300 grid at order 1.  Member m has the values
D A D, D = diag(1 + 1e-3 u) from seed 41 + m (a congruence: every member has A's inertia).  For every B:
  batch_refactor_ms   one batch.refactor(V) of all B members, V on the device (median of the warm calls), with the kernels' own
                      time beside it (batch_kernel_ms: the whole walk between two events)
  single_refactor_ms  B calls of the single factor's refactor(), one per member, values on the device, in the same run (one
                      pass, after a warm call), with the sum of their kernel times
  solve_*_r1 / _r8    batch.solve of an n x (B r) block (the division by D fused into the backward sweep) against B exact-order
                      solves of n x r blocks on the single factor refactored to the last member
  solve_d_pass_ms_r*  the pass over X that the fused division removes, timed alone: csx_block_div_rows -- the kernel the single
                      solver runs for D -- on the same n x (B r) block, one launch that reads and writes X once.  A solve with
                      D as a pass of its own is the fused solve less n B r divisions at the head of the backward chains plus
                      this pass; solve_unfused_over_fused_r* = (batch + pass) / batch.  The driver of this tool does the
                      timing (--no-d-pass leaves it out); the library has no option for it.
  launches            level and walker launches of the batch's run and of one single refactor: equal by construction
All times are host wall-clock around the call with the device synchronised before and after, so the host's share of a call is
in both sides.  One JSON line per B goes to --out; the ratios in it are reported, not promised."""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from time_chol_refactor import device, grid, wall  # noqa: E402
from time_ldl import SIGMA, congruent, med  # noqa: E402
from time_slu_batch import values_of  # noqa: E402

GRID = 300
MEMORY_CAP = 16e9
SOLVE_R = (1, 8)


def measure(members, reps, d_pass):
    import _csx
    import csparse as cs
    K = grid(GRID)
    n = K.shape[0]
    A = sp.csc_matrix(K - SIGMA * sp.identity(n, format="csc"))
    A.sort_indices()
    sol = cs.ldlsol_factor(device(A), 1, exact=True)
    assert sol is not None
    lnz = sol.info()["lnz"]
    rng = np.random.default_rng(8)
    for B in members:
        while B > 1 and 1.0 * B * lnz * 8 > MEMORY_CAP:
            B //= 2
        rec = {"matrix": "grid%d shifted" % GRID, "order": 1, "n": n, "sigma": SIGMA, "lnz": lnz, "B": B}
        vals = [congruent(A, 41 + m).data for m in range(B)]
        dV = cs.dvec(np.ascontiguousarray(np.stack(vals, axis=1)))
        dv = [cs.dvec(v) for v in vals]
        # ---- B single refactors, one pass after a warm call ----
        assert sol.refactor(dv[0])
        one, ker = [], []
        for m in range(B):
            ok, ms = wall(lambda: sol.refactor(dv[m]))
            assert ok
            one.append(ms)
            ker.append(sol.info()["kernel_us"] / 1e3)
        single = sol.info()
        rec["single_refactor_ms"], rec["single_kernel_ms"], rec["one_refactor_ms"] = float(np.sum(one)), float(np.sum(ker)), med(one)
        # ---- the batch ----
        batch, first = wall(lambda: sol.batch(dV))
        assert batch.ok.all()
        rec["batch_factor_ms"] = first
        t, k = [], []
        for _ in range(reps + 1):
            ok, ms = wall(lambda: batch.refactor(dV))
            assert ok.all()
            t.append(ms)
            k.append(batch.info()["kernel_us"] / 1e3)
        rec["batch_refactor_ms"], rec["batch_kernel_ms"] = med(t[1:]), med(k[1:])
        rec["batch_over_single"] = rec["batch_refactor_ms"] / rec["single_refactor_ms"]
        rec["batch_over_single_kernels"] = rec["batch_kernel_ms"] / rec["single_kernel_ms"]
        i = batch.info()
        rec["launches"] = {"batch_level": i["level_launches"], "batch_walker": i["run_launches"],
                           "single_level": single["level_launches"], "single_walker": single["run_launches"]}
        rec["neg"] = [int(i["neg"].min()), int(i["neg"].max()), int(single["neg"])]
        gl, gd = batch.member(B - 1)
        f = sol.factors                                            # (the single factor holds the last member's values)
        rec["last_member_equal"] = bool(values_of(f.L).tobytes() == gl.tobytes() and f.D.numpy().tobytes() == gd.tobytes())
        # ---- solves ----
        for r in SOLVE_R:
            X = rng.uniform(-1.0, 1.0, (n, B * r))
            t = []
            for _ in range(reps + 1):
                dX = cs.dvec(X)
                t.append(wall(lambda: batch.solve(dX))[1])
            rec["solve_batch_ms_r%d" % r] = med(t[1:])
            blocks = [cs.dvec(np.ascontiguousarray(X[:, m * r:(m + 1) * r])) for m in range(B)]
            sol.solve(cs.dvec(np.ascontiguousarray(X[:, :r])))    # warm: the plans of the new values
            t = [wall(lambda: sol.solve(blocks[m]))[1] for m in range(B)]
            rec["solve_single_ms_r%d" % r] = float(np.sum(t))
            rec["solve_batch_over_single_r%d" % r] = rec["solve_batch_ms_r%d" % r] / rec["solve_single_ms_r%d" % r]
            last = dX.numpy().reshape(n, B * r)[:, (B - 1) * r:]
            rec["solve_last_member_equal_r%d" % r] = bool(last.tobytes() == blocks[B - 1].numpy().reshape(n, r).tobytes())
            if d_pass:
                dW, hd = cs.dvec(X), f.D.handle
                t = [wall(lambda: _csx.check(_csx.lib().csx_block_div_rows(dW.handle, hd, n, B * r), "csx_block_div_rows"))[1]
                     for _ in range(reps + 1)]
                rec["solve_d_pass_ms_r%d" % r] = med(t[1:])
                rec["solve_unfused_over_fused_r%d" % r] = 1.0 + rec["solve_d_pass_ms_r%d" % r] / rec["solve_batch_ms_r%d" % r]
        del batch, dV, dv
        yield rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ldl_batch_time.jsonl"))
    ap.add_argument("--members", default="1,8,64")
    ap.add_argument("--no-d-pass", action="store_true", help="do not time the separate pass over X for D")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for rec in measure([int(b) for b in a.members.split(",")], a.reps, not a.no_d_pass):
        rec["device"] = cs.device_name()
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
