"""Where tests/tol.py's CHOL_EPS_UNITS comes from: for every case of tests/chol_cases.py that runs on a rounding route, the
plain-C oracle's own distance from a factorisation of the same matrix in numpy.longdouble, as the largest
|l_ij - exact_ij| / (EPS * terms_ij) (tol.chol_terms), and the smallest update of the case in the same units.  No device.

    python tools/measure_chol_edges.py            # writes profiles/chol_edges.jsonl, prints the largest figure
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("csparse.py_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

import numpy as np  # noqa: E402

import chol_cases as CC  # noqa: E402


def measure(name, which="A"):
    case = CC.BY_NAME[name]
    Lp, Li, Lx = CC.oracle(name, which)
    t0 = time.perf_counter()
    exact = CC.longdouble_factor(case, CC.values(case, which), Lp, Li)
    units = CC.rounding_units(name, which, exact)
    small, seen, total = CC.smallest_update(name, which)
    return {"case": name, "values": which, "n": case.n, "lnz": int(Lp[case.n]), "oracle_eps_units": units,
            "smallest_update_eps_units": small, "updates_seen": seen, "updates": total, "seconds": round(time.perf_counter() - t0, 2)}


def main():
    out = os.path.join(ROOT, "profiles", "chol_edges.jsonl")
    rows = []
    for name in CC.ROUNDING:
        for which in ("A", 0, 1):
            rows.append(measure(name, which))
            print(json.dumps(rows[-1]), flush=True)
    with open(out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    worst = max(rows, key=lambda r: r["oracle_eps_units"])
    print("largest oracle distance: %.4f eps units (%s, values %s); CHOL_EPS_UNITS = 4 x that" %
          (worst["oracle_eps_units"], worst["case"], worst["values"]))
    print("smallest update: %.3e eps units" % min(r["smallest_update_eps_units"] for r in rows))


if __name__ == "__main__":
    main()
