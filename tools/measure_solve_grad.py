"""Where tests/grad_tol.py's GRAD_EPS_UNITS comes from: for every system of tests/grad_tol.py (the matrices the refine, static-LU,
LDL', Cholesky and Householder-QR tests already factor) and every direction, the largest error of solve_grad()'s gA against
-(Aop^-T GX) X' on the pattern computed by numpy's dense float64 solve, in units of 2^-52 condest() (|Lambda| |X|')[i, j]
(grad_tol.eps_units).  The reference is numpy, never this code's earlier output.  Needs an MI355X.

    python tools/measure_solve_grad.py [--out FILE]      # default: profiles/solve_grad_edges.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("csparse.py_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

import grad_tol as GT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_grad_edges.jsonl"))
    args = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init()
    rows = []
    for s in GT.SYSTEMS:
        for trans in s.directions:
            gA, cond = GT.device_gradient(cs, s, trans)
            rows.append({"system": s.name, "solver": s.solver, "n": s.n, "nnz": int(len(s.i)), "k": GT.K, "trans": bool(trans),
                         "sym": bool(s.sym), "condest": cond, "device": _csx.device_info()[0],
                         "eps_units": GT.eps_units(s, trans, gA, cond)})
            print(json.dumps(rows[-1]), flush=True)
    worst = max(rows, key=lambda r: r["eps_units"])
    print("largest: %.6g (%s, trans=%s); GRAD_EPS_UNITS = 8 x that" % (worst["eps_units"], worst["system"], worst["trans"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
