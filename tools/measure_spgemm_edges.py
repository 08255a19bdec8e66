"""For the record beside tests/test_gpu_multiply_edges.py (needs a GPU): runs that file once in this process and writes, one JSON
object a line, the wall time of the file and per case family the largest |x - exact| / (gamma_c sum|a b|) of the mixed-value
runs in the default mode -- the figure the tests hold to 1 (plus half an ulp of the exact sum).  The bound is derived, not
tuned: nothing reads this file.

    python tools/measure_spgemm_edges.py [--out FILE]      # default: profiles/spgemm_edges.jsonl
"""
import argparse
import json
import os
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm_edges.jsonl"))
    args = ap.parse_args()
    t0 = time.time()
    rc = pytest.main(["-m", "gpu", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_multiply_edges.py")])
    wall = time.time() - t0
    import test_gpu_multiply_edges as G
    import _csx
    rows = [{"file": "tests/test_gpu_multiply_edges.py", "exit": int(rc), "wall_s": round(wall, 2), "device": _csx.device_info()[0].strip(),
             "cus": _csx.device_info()[1]}]
    rows += [{"family": fam, "max_err_over_gamma_sum_abs": ratio} for fam, ratio in sorted(G.RATIOS.items())]
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("\n".join(json.dumps(r) for r in rows))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
