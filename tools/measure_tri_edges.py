"""Where tests/tol.py's TRI_EPS_UNITS comes from: for every case of tests/tri_cases.py that runs in a rounding-equal order -- the
matrix-core sweep (ROUNDING), the fused pair of them in csx_lusol_solve and cholsol_factor(exact=False) on a band (PAIRS) -- the
plain-C oracle's own distance from the same substitutions in numpy.longdouble, as the largest |x_i - exact_i| / (EPS * terms_i)
over the block (tri_cases.substitution: terms_i = (|b_i| + sum_j |t_ij x_j|) / |t_ii| of the last substitution).  That column
needs no device and sets the bound.  With --device (on a machine with a GPU) the second field is filled as well: the device's
distance from the ORACLE in the same units, the figure the tests hold to the bound (tests/test_gpu_tri_edges.py prints the same
figures); without it the figures of an earlier run are kept.

    python tools/measure_tri_edges.py [--device] [--out FILE]      # default: profiles/trisolve_edges.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("csparse.py_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

import tri_cases as TC  # noqa: E402


def device_units(rid):
    import _csx
    import csparse as cs
    _csx.init()
    if rid in TC.PAIRS:
        import test_gpu_tri_edges as G
        return G.pair_on_device(cs, rid)[0]
    r = TC.ROUNDING_BY_ID[rid]
    n, Tp, Ti, Tx = TC.rounding_matrix(rid)
    A = cs.cs_spalloc(n, n, len(Ti), True, False)
    A.p, A.i, A.x = Tp.tolist(), Ti.tolist(), Tx.tolist()
    cs.cs_pin(A)
    plan = cs._plan(A._dev, TC.KIND_ID[r.kind])
    _csx.check(_csx.lib().csx_tri_set_order(plan, 0), "csx_tri_set_order")
    X = cs.dvec(TC.rounding_rhs(r))
    _csx.check(_csx.lib().csx_tri_solve(plan, X.handle, r.nrhs), "csx_tri_solve")
    assert _csx.tri_launches(plan) == {"ragged": 1}, rid
    return TC.eps_units(rid, X.numpy().reshape(n, r.nrhs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trisolve_edges.jsonl"))
    args = ap.parse_args()
    kept = {}
    committed = os.path.join(ROOT, "profiles", "trisolve_edges.jsonl")
    if os.path.exists(committed):
        kept = {r["case"]: r.get("device_eps_units") for r in map(json.loads, open(committed))}
    rows = []
    for rid in TC.ROUNDING_MEASURED + list(TC.PAIRS):
        if rid in TC.PAIRS:
            row = {"case": rid, "oracle_eps_units": TC.pair_oracle_units(rid)}
        else:
            r = TC.ROUNDING_BY_ID[rid]
            n, Tp = TC.rounding_matrix(rid)[:2]
            row = {"case": rid, "n": n, "nnz": int(Tp[n]), "nrhs": r.nrhs, "oracle_eps_units": TC.oracle_eps_units(rid)}
        row["device_eps_units"] = device_units(rid) if args.device else kept.get(rid)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    worst = max(rows, key=lambda row: row["oracle_eps_units"])
    print("largest oracle distance: %.4f eps units (%s); TRI_EPS_UNITS = 4 x that" % (worst["oracle_eps_units"], worst["case"]))


if __name__ == "__main__":
    main()
