#!/usr/bin/env python3
"""Times of ldlsol_factor(...).inverse() and slusol_factor(...).inverse() (csx_ldl_inverse, csx_slu_inverse) by
the method of tools/time_sparseinv.py: wall median of --reps calls after one warm-up (every call ends with a download of its
flag, so it is synchronised), the launches' time between two events beside it.

    python tools/time_sparseinv_ldlu.py [--reps 5] [--only grid_ldl,grid_lu,forest] [--forest-blocks 78125] [--out FILE]

grid_ldl  K - 3.7 I of the 300 x 300 grid Laplacian at order 1; beside it cholsol_factor(K).inverse() on the same pattern in the
          same run (the lookups are the same: the LDL' call should cost what the Cholesky call costs).
grid_lu   the convection-diffusion operator on the 300 x 300 grid (tests/slu_cases.py's) at order 1; beside it the LDL' call on
          the symmetric part's pattern (the lookups are shared by the two sums: well under twice).
forest    --forest-blocks dense blocks of 64 columns (5M rows by default), every other block negated, both kinds; beside them
          solve() of ONE block of 128 unit vectors times the number of such blocks.
One JSON line per case on stdout and in --out (default profiles/sparseinv_ldlu_time.jsonl)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402

NRHS = 128


def lib():
    return _csx.lib()


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def dev_matrix(n, p, i, x):
    h = _csx.new_handle()
    p, i, x = np.asarray(p, np.int32), np.asarray(i, np.int32), np.asarray(x, np.float64)
    _csx.check(lib().csx_csc_upload(n, n, _csx.pi(p), _csx.pi(i), _csx.pd(x), h), "csx_csc_upload")
    A = cs._from_device(h, lambda z: max(z, 1))
    A._pinned = True
    return A


def times(call, reps):
    """(wall median, event median, info) of `call` (which leaves its figures in sparseinv_info)"""
    wall, kern, info = [], [], None
    for r in range(reps + 1):
        Z = call()
        info = cs.sparseinv_info()
        del Z
        if r:
            wall.append(info["wall_ms"])
            kern.append(info["kernel_ms"])
    return float(np.median(wall)), float(np.median(kern)), info


def record(name, kind, F, reps):
    wall, kern, info = times(F.inverse, reps)
    assert info["kind"] == kind
    return {"case": name, "kind": kind, "n": info["n"], "depths": info["depths"], "widest": info["widest"], "terms": info["terms"],
            "call_ms": wall, "kernel_ms": kern}


def laplacian(g):
    T = sp.diags([-1, 2, -1], [-1, 0, 1], shape=(g, g))
    A = (sp.kron(sp.identity(g), T) + sp.kron(T, sp.identity(g)) + 0.5 * sp.identity(g * g)).tocsc()
    A.sort_indices()
    return A


def unit_block_ms(F, n, reps):
    """solve() of a block of NRHS unit vectors from the middle of the identity, events around the solve alone"""
    first = (n // NRHS // 2) * NRHS
    rows = min(NRHS, n - first)
    eye = np.zeros((rows, NRHS))
    eye[np.arange(rows), np.arange(rows)] = 1.0
    B = cs.dvec(n, NRHS)
    ms = []
    for r in range(reps + 1):
        B.fill(0.0)
        h = _csx.new_handle()
        _csx.check(lib().csx_vec_wrap(C.c_void_p(B.device_ptr() + 8 * first * NRHS), rows * NRHS, h), "csx_vec_wrap")
        _csx.check(lib().csx_vec_write(h, _csx.pd(eye), eye.size), "csx_vec_write")
        _csx.free(h)
        with _csx.Timer() as t:
            F.solve(B)
        if r:
            ms.append(t.ms)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="grid_ldl,grid_lu,forest")
    ap.add_argument("--forest-blocks", type=int, default=78125)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparseinv_ldlu_time.jsonl"))
    a = ap.parse_args()
    _csx.init(0)
    g = 300
    with open(a.out, "w") as out:
        for name in a.only.split(","):
            if name == "grid_ldl":
                K = laplacian(g)
                S = (K - 3.7 * sp.identity(g * g)).tocsc()
                S.sort_indices()
                F = cs.ldlsol_factor(dev_matrix(g * g, S.indptr, S.indices, S.data), order=1)
                rec = record("grid300_shifted", "ldl", F, a.reps)
                rec["max_abs_l"] = F.info()["max_abs_l"]
                Fc = cs.cholsol_factor(dev_matrix(g * g, K.indptr, K.indices, K.data), order=1)
                wall, kern, _ = times(Fc.inverse, a.reps)
                rec.update({"chol_call_ms": wall, "chol_kernel_ms": kern, "ratio_to_chol": rec["kernel_ms"] / kern})
                emit(rec, out)
            elif name == "grid_lu":
                import slu_cases
                n, p, i, x = slu_cases.grid(g)
                F = cs.slusol_factor(dev_matrix(n, p, i, x), order=1)
                rec = record("convection_grid300", "lu", F, a.reps)
                M = sp.csc_matrix((np.asarray(x, float), np.asarray(i), np.asarray(p)), shape=(n, n))
                M = ((M + M.T) * 0.5).tocsc()
                M.sort_indices()
                G = cs.ldlsol_factor(dev_matrix(n, M.indptr, M.indices, M.data), order=1)
                wall, kern, _ = times(G.inverse, a.reps)
                rec.update({"ldl_call_ms": wall, "ldl_kernel_ms": kern, "ratio_to_ldl": rec["kernel_ms"] / kern})
                emit(rec, out)
            elif name == "forest":
                nb, bs = a.forest_blocks, 64
                n = nb * bs
                h = _csx.new_handle()
                _csx.check(lib().csx_gen_gspd(nb, bs, 20240606, h), "csx_gen_gspd")
                A = cs._from_device(h, lambda z: max(z, 1))
                _, _, nnz, _ = A._dev.info()
                p, i, x = np.empty(n + 1, np.int32), np.empty(nnz, np.int32), np.empty(nnz)
                _csx.check(lib().csx_csc_download(A._dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
                del A
                x[(np.repeat(np.arange(n, dtype=np.int32), np.diff(p)) // bs) % 2 == 1] *= -1.0
                A = dev_matrix(n, p, i, x)
                del p, i, x
                for kind, factor in (("ldl", cs.ldlsol_factor), ("lu", cs.slusol_factor)):
                    F = factor(A)
                    rec = record("signed_forest_blocks_of_64", kind, F, a.reps)
                    one = unit_block_ms(F, n, a.reps)
                    blocks = (n + NRHS - 1) // NRHS
                    rec.update({"unit_block_ms": one, "unit_blocks": blocks, "unit_route_ms": one * blocks,
                                "speedup": one * blocks / rec["call_ms"]})
                    emit(rec, out)
                    del F
                    _csx.check(lib().csx_mem_trim(), "csx_mem_trim")
            else:
                raise SystemExit("unknown case " + name)
            _csx.check(lib().csx_mem_trim(), "csx_mem_trim")


if __name__ == "__main__":
    main()
