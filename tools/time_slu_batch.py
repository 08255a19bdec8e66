#!/usr/bin/env python3
"""slusol_factor(...).batch() against B calls of refactor(), and its solves against B single exact solves.

    python tools/time_slu_batch.py [--reps 2] [--out profiles/slu_batch_time.jsonl] [--only plain] [--members 1,8,64]

Matrix: tools/time_slu.py's convection-diffusion on the 300 x 300 grid at order 1, plain and shifted by 3.7.  Member m has the
values D A D, D = diag(1 + 1e-3 u) from seed 41 + m.  For every B (the largest kept below 16 GB for 2 B lnz doubles):
  batch_refactor_ms   one batch.refactor(V) of all B members, V on the device (median of the warm calls), with the kernels' own
                      time beside it (batch_kernel_ms: the whole walk between two events)
  single_refactor_ms  B calls of the single factor's refactor(), one per member, values on the device, in the same run (one
                      pass, after a warm call), with the sum of their kernel times
  solve_*_r1 / _r8    batch.solve of an n x (B r) block against B exact-order solves of n x r blocks on the single factor
                      refactored to the last member (same work per call, the values do not change the time)
  launches            level and walker launches of the batch's run and of one single refactor: equal by construction
All times are host wall-clock around the call with the device synchronised before and after, so the host's share of a call is
in both sides.  One JSON line per matrix and B goes to --out; the ratios in it are reported, not promised."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from time_chol_refactor import device, wall  # noqa: E402
from time_ldl import congruent, med  # noqa: E402
from time_slu import GRID, SIGMA, convection_diffusion  # noqa: E402

MEMORY_CAP = 16e9
SOLVE_R = (1, 8)


def values_of(M):
    import _csx
    _, n, nnz, _ = M._dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1))
    _csx.check(_csx.lib().csx_csc_download(M._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return x[:nnz]


def measure(name, sigma, members, reps):
    import csparse as cs
    A = convection_diffusion(GRID, sigma)
    n = A.shape[0]
    sol = cs.slusol_factor(device(A), 1, exact=True)
    assert sol is not None
    lnz = sol.info()["lnz"]
    rng = np.random.default_rng(8)
    for B in members:
        while B > 1 and 2.0 * B * lnz * 8 > MEMORY_CAP:
            B //= 2
        rec = {"matrix": "convection-diffusion grid%d %s" % (GRID, name), "order": 1, "n": n, "sigma": sigma, "lnz": lnz, "B": B}
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
        gl, gu = batch.member(B - 1)
        f = sol.factors                                            # (the single factor holds the last member's values)
        rec["last_member_equal"] = bool(values_of(f.L).tobytes() == gl.tobytes() and values_of(f.U).tobytes() == gu.tobytes())
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
        del batch, dV, dv
        yield rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slu_batch_time.jsonl"))
    ap.add_argument("--only", action="append", choices=["plain", "shifted"], help="run this matrix only (may be repeated)")
    ap.add_argument("--members", default="1,8,64")
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    for name in (a.only or ["shifted", "plain"]):
        for rec in measure(name, SIGMA if name == "shifted" else 0.0, [int(b) for b in a.members.split(",")], a.reps):
            rec["device"] = cs.device_name()
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
