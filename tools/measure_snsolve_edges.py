#!/usr/bin/env python3
"""Measure the supernodal solve against the oracle on every case of tests/sn_cases.py (needs an MI355X):

    python tools/measure_snsolve_edges.py

runs all the checks of tests/test_gpu_snsolve.py case by case, stops at the first one that fails, and -- only when none did --
writes one line per case to profiles/snsolve_edges.jsonl: the largest |x - ref| / (eps * terms) over the compared columns.
tests/tol.py's SN_EPS_UNITS is 8 x the largest of them over the cases on the near side of the growth guard."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conftest  # noqa: E402,F401  (the package and oracle paths)
import _csx  # noqa: E402
import csparse  # noqa: E402
import sn_cases as SC  # noqa: E402
from test_gpu_snsolve import run_case  # noqa: E402


def main():
    _csx.init()
    lines = []
    for c in SC.CASES:
        units = run_case(csparse, c.name)           # an AssertionError ends the run: nothing is written
        n, Lp, _, _, growth = SC.built(c.name)[:5]
        lines.append({"case": c.name, "n": n, "lnz": int(Lp[n]), "mode": c.mode, "ks": list(c.ks),
                      "guard_measure": round(growth, 3), "eps_units": round(units, 4)})
        print(json.dumps(lines[-1]), flush=True)
    with open(os.path.join(ROOT, "profiles", "snsolve_edges.jsonl"), "w") as f:
        f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
