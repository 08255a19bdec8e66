#!/usr/bin/env python3
"""assembly_plan against the route it replaces.

    python tools/time_assemble.py [--reps 5] [--scale 1.0] [--cases mesh,nodup,skew,refactor,ladder]
                                  [--out profiles/assemble_time.jsonl]

mesh      a structured mesh of trilinear hexahedra (116^3 elements at --scale 1), scalar unknown, 64 triplets per element in
          element order: 1.0e8 triplets, at most 8 per slot.
nodup     the headline G-rand shape, 5M x 5M with 64 entries per column (nz == nnz == 3.2e8), the triplets listed by ROW, as a
          row-wise assembly lists them: the permuted copy.
skew      the mesh plus one slot that receives 1e6 extra duplicates (a wave of its own folds it).
refactor  the 1M-row generated matrix of tools/time_refactor.py, its values split three ways into triplets:
          assemble + btf_factor.refactor against compress + dupl + refactor.
ladder    2^24 triplets in slots of L terms each, L = 8 .. 1024, every slot folded by one lane ("assemble.long" above L) and
          by a wave of its own (below L): the measurement that places the threshold.

Per case: `assemble` (values in a dvec -> a new dvec) and `update` (into .matrix in place) -- the kernel between two events
(info()["kernel_us"]) and host wall-clock per call ending in a synchronise; `assemble` from a numpy array (the 8 bytes per
triplet cross PCIe); and, in the same run, the route of the parent commit to the same values: csx_compress of the triplets
(16 bytes per triplet cross PCIe, a radix sort) + csx_dupl (a product with the identity), the two library calls behind
cs_compress of a pinned T and cs_dupl, handed numpy arrays (no list conversion: the library's time alone).  Every figure is
the median of --reps calls after one warm call.  fraction_of_peak = (12 nz + 8 nnz + 4 (nnz + 1)) bytes / kernel time /
8 TB/s.  One JSON line per case goes to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]

PEAK = 8.0e12


def wall(fn):
    import _csx
    _csx.sync()
    t0 = time.perf_counter()
    out = fn()
    _csx.sync()
    return out, 1e3 * (time.perf_counter() - t0)


def median_ms(fn, reps, also=None):
    """median wall ms of reps calls after one warm call; also(): a figure read after every call (its median too)"""
    t, extra = [], []
    for r in range(reps + 1):
        _, ms = wall(fn)
        if r:
            t.append(ms)
            if also:
                extra.append(also())
    return (float(np.median(t)), float(np.median(extra))) if also else float(np.median(t))


def triplet(m, n, Ti, Tj, Tx):
    """a triplet `cs` on numpy arrays (no lists at these sizes)"""
    import csparse as cs
    T = cs.cs_spalloc(m, n, 1, True, True)
    T.i, T.p, T.x = Ti, Tj, Tx
    T.nz = T.nzmax = len(Ti)
    return T


def parent_route(m, n, Ti, Tj, Tx):
    """csx_compress + csx_dupl: a new matrix handle with the same values up to the order of the additions"""
    import _csx
    lib = _csx.lib()
    hc, hd = _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_compress(m, n, len(Ti), _csx.pi(Ti), _csx.pi(Tj), _csx.pd(Tx), hc), "csx_compress")
    _csx.check(lib.csx_dupl(hc, hd), "csx_dupl")
    _csx.free(hc)
    return hd


def measure(label, m, n, Ti, Tj, Tx, reps, with_parent=True):
    import _csx
    import csparse as cs
    Ti, Tj, Tx = _csx.i32(Ti), _csx.i32(Tj), _csx.f64(Tx)
    P, plan_ms = wall(lambda: cs.assembly_plan(triplet(m, n, Ti, Tj, None)))
    info = P.info()
    nz, nnz = info["nz"], info["nnz"]
    rec = {"case": label, "m": m, "n": n, "nz": nz, "nnz": nnz, "max_dup": info["max_dup"], "long_slots": info["long_slots"],
           "plan_wall_ms": plan_ms, "plan_host_build_ms": info["build_us"] / 1e3,
           "algorithmic_bytes": 12 * nz + 8 * nnz + 4 * (nnz + 1)}
    dv = cs.dvec(Tx)
    kernel = lambda: P.info()["kernel_us"] / 1e3  # noqa: E731
    rec["assemble_wall_ms"], rec["assemble_kernel_ms"] = median_ms(lambda: P.assemble(dv), reps, kernel)
    rec["assemble_numpy_wall_ms"] = median_ms(lambda: P.assemble(Tx), reps)
    P.update(dv)        # the first update of the pattern-only matrix gives it its values
    rec["update_wall_ms"], rec["update_kernel_ms"] = median_ms(lambda: P.update(dv), reps, kernel)
    rec["fraction_of_peak"] = rec["algorithmic_bytes"] / (rec["assemble_kernel_ms"] * 1e-3) / PEAK
    if with_parent:
        def parent():
            _csx.free(parent_route(m, n, Ti, Tj, Tx))
        rec["parent_compress_dupl_wall_ms"] = median_ms(parent, reps)
        rec["parent_over_assemble_wall"] = rec["parent_compress_dupl_wall_ms"] / rec["assemble_wall_ms"]
        rec["parent_over_assemble_numpy_wall"] = rec["parent_compress_dupl_wall_ms"] / rec["assemble_numpy_wall_ms"]
        # the same values: the parent's sums are rounding-equal (atomic arrival order), the plan's are the reference's bits
        h = parent_route(m, n, Ti, Tj, Tx)
        x = np.empty(max(nnz, 1))
        _csx.check(_csx.lib().csx_csc_download(h, None, None, _csx.pd(x)), "csx_csc_download")
        _csx.free(h)
        mine = P.assemble(dv).numpy()
        scale = np.maximum(np.abs(mine), 1e-300)
        rec["max_rel_difference_to_parent"] = float(np.max(np.abs(x[:nnz] - mine) / scale)) if nnz else 0.0
    return rec, P, dv


def hex_mesh(ne):
    """(nodes, Ti, Tj): trilinear hexahedra on an ne^3 grid, 64 triplets per element in element order"""
    e = np.arange(ne, dtype=np.int64)
    ex, ey, ez = np.meshgrid(e, e, e, indexing="ij")
    n1 = ne + 1
    base = ((ex * n1 + ey) * n1 + ez).ravel()
    corner = np.array([(a * n1 + b) * n1 + c for a in (0, 1) for b in (0, 1) for c in (0, 1)], dtype=np.int64)
    nodes = (base[:, None] + corner[None, :]).astype(np.int32)           # (elements, 8)
    return n1 ** 3, np.repeat(nodes, 8, axis=1).ravel(), np.tile(nodes, (1, 8)).ravel()


def mesh(a):
    ne = max(2, int(round(116 * a.scale ** (1.0 / 3.0))))
    n, Ti, Tj = hex_mesh(ne)
    Tx = np.random.default_rng(1).uniform(-1.0, 1.0, len(Ti))
    rec = measure("mesh", n, n, Ti, Tj, Tx, a.reps)[0]
    rec["elements"] = ne ** 3
    return [rec]


def nodup(a):
    import _csx
    lib = _csx.lib()
    n = max(64, int(5_000_000 * a.scale))
    h, ht = _csx.new_handle(), _csx.new_handle()
    _csx.check(lib.csx_gen_grand(n, 64, 20240601, h), "csx_gen_grand")
    _csx.check(lib.csx_transpose(h, 1, ht), "csx_transpose")     # the rows of G, one after another: the row-wise listing
    _csx.free(h)
    p, j, x = np.empty(n + 1, np.int32), np.empty(64 * n, np.int32), np.empty(64 * n)
    _csx.check(lib.csx_csc_download(ht, _csx.pi(p), _csx.pi(j), _csx.pd(x)), "csx_csc_download")
    _csx.free(ht)
    i = np.repeat(np.arange(n, dtype=np.int32), np.diff(p))
    return [measure("nodup", n, n, i, j, x, a.reps)[0]]


def skew(a):
    ne = max(2, int(round(116 * a.scale ** (1.0 / 3.0))))
    n, Ti, Tj = hex_mesh(ne)
    extra = max(1000, int(1_000_000 * a.scale))
    mid = n // 2
    Ti = np.concatenate([Ti, np.full(extra, mid, np.int32)])
    Tj = np.concatenate([Tj, np.full(extra, mid, np.int32)])
    Tx = np.random.default_rng(2).uniform(-1.0, 1.0, len(Ti))
    rec = measure("skew", n, n, Ti, Tj, Tx, a.reps)[0]
    rec["extra_duplicates"] = extra
    return [rec]


def refactor(a):
    import scipy.sparse as sp
    import _csx
    import btf_oracle
    import csparse as cs
    rows = max(2000, int(1_000_000 * a.scale))
    S = sp.csc_matrix(btf_oracle.reducible(btf_oracle.block_sizes(rows, 11), 8, 11)[0])
    n, nnz = S.shape[0], int(S.nnz)
    col = np.repeat(np.arange(n, dtype=np.int32), np.diff(S.indptr))
    rng = np.random.default_rng(5)
    order = rng.permutation(2 * nnz)
    Ti = _csx.i32(np.concatenate([S.indices, np.concatenate([S.indices, S.indices])[order]]))
    Tj = _csx.i32(np.concatenate([col, np.concatenate([col, col])[order]]))

    def values(seed):
        r = np.random.default_rng(seed)
        d = S.data * (1.0 + 1e-3 * r.uniform(-1, 1, nnz))
        u, v = d * r.uniform(0.2, 0.5, nnz), d * r.uniform(-0.3, 0.4, nnz)
        return np.concatenate([u, np.concatenate([v, d - u - v])[order]])

    v = [values(31), values(32)]
    rec, P, _ = measure("refactor", n, n, Ti, Tj, v[0], a.reps)
    P.update(v[0])
    sol = cs.btf_factor(P.matrix)
    dv = [cs.dvec(v[0]), cs.dvec(v[1])]
    assert sol.refactor(P.assemble(dv[1]))     # the first refactor builds the maps and the schedule
    step = [0]

    def mine():
        step[0] += 1
        assert sol.refactor(P.assemble(dv[step[0] % 2]))

    def parent():
        step[0] += 1
        h = parent_route(n, n, Ti, Tj, v[step[0] % 2])
        A2 = cs._from_device(h, lambda k: k)
        assert sol.refactor(A2)

    rec["assemble_refactor_wall_ms"] = median_ms(mine, a.reps)
    rec["parent_compress_dupl_refactor_wall_ms"] = median_ms(parent, a.reps)
    rec["refactor_info"] = sol.refactor_info()
    rec["parent_over_assemble_refactor"] = rec["parent_compress_dupl_refactor_wall_ms"] / rec["assemble_refactor_wall_ms"]
    return [rec]


def ladder(a):
    import _csx
    import csparse as cs
    nz = max(1 << 12, int((1 << 24) * a.scale))
    rng = np.random.default_rng(9)
    Tx = rng.uniform(-1.0, 1.0, nz)
    dv = cs.dvec(Tx)
    out = []
    for L in (8, 16, 32, 64, 128, 256, 1024):
        slots = nz // L
        rows = 1 << 10
        s = rng.permutation(np.repeat(np.arange(slots, dtype=np.int64), L))     # every slot's terms spread over the list
        Ti, Tj = _csx.i32(s % rows), _csx.i32(s // rows)
        rec = {"case": "ladder", "terms_per_slot": L, "slots": slots, "nz": slots * L}
        for name, thr in (("lane", 1 << 30), ("wave", L - 1)):
            with _csx.option("assemble.long", thr):
                P = cs.assembly_plan(triplet(rows, (slots + rows - 1) // rows, Ti, Tj, None))
                assert P.info()["long_slots"] == (0 if name == "lane" else slots)
                rec[name + "_kernel_ms"] = median_ms(lambda: P.assemble(dv), a.reps, lambda: P.info()["kernel_us"] / 1e3)[1]
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every case (rehearsals)")
    ap.add_argument("--cases", default="mesh,nodup,skew,refactor,ladder")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_time.jsonl"))
    a = ap.parse_args()
    import _csx
    import csparse as cs
    _csx.init(0)
    cases = {"mesh": mesh, "nodup": nodup, "skew": skew, "refactor": refactor, "ladder": ladder}
    for name in a.cases.split(","):
        for rec in cases[name](a):
            rec["device"] = cs.device_name()
            rec["reps"] = a.reps
            line = json.dumps(rec)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
