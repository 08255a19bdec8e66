#!/usr/bin/env python3
"""Per-stage device times and end-to-end call times of cs_dmperm, with scipy's maximum_bipartite_matching plus
strong connected_components on the host CPU as the baseline.

    python tools/time_dmperm.py [--reps 3] [--skip-scipy] [--scipy-limit S] [--only NAME,...]

Matrices: the bench G-rand (5M x 5M, 64 per column), config 5's block-SPD matrix, the 1M planted-structure matrix
of tests/test_gpu_dmperm.py, a randomly permuted upper bidiagonal chain (200 000 rows) and a natural-order block lower
bidiagonal chain of 20 000 2 x 2 blocks.  The scipy baseline runs in a child process (no GPU) and is reported as not
measured when it takes longer than --scipy-limit seconds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "csparse.py_amd"), os.path.join(ROOT, "tests")]

import _csx  # noqa: E402
import csparse as cs  # noqa: E402


def gen(fn, *args):
    h = _csx.new_handle()
    _csx.check(getattr(_csx.lib(), fn)(*args, h), fn)
    return cs._from_device(h, lambda nnz: max(nnz, 1))


def upload(n, p, i):
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(n, n, _csx.pi(_csx.i32(p)), _csx.pi(_csx.i32(i)), None, h), "upload")
    return cs._from_device(h, lambda nnz: max(nnz, 1))


def host_arrays(A):
    m, n, nnz, _ = A._dev.info()
    p = np.empty(n + 1, np.int32)
    i = np.empty(max(nnz, 1), np.int32)
    _csx.check(_csx.lib().csx_csc_download(A._dev.handle, _csx.pi(p), _csx.pi(i), None), "download")
    return p, i[:nnz]


def chain(n, seed):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    r = np.concatenate([np.arange(n), np.arange(n - 1)])
    c = np.concatenate([np.arange(n), np.arange(1, n)])
    pr, pc = rng.permutation(n), rng.permutation(n)
    S = sp.csc_matrix((np.ones(len(r)), (pr[r], pc[c])), shape=(n, n))
    S.sort_indices()
    return S.indptr, S.indices


SCIPY_CHILD = """
import sys, time, numpy as np, scipy.sparse as sp
from scipy.sparse import csgraph
z = np.load(sys.argv[1])
S = sp.csc_matrix((np.ones(len(z["i"])), z["i"], z["p"]), shape=tuple(z["shape"]))
t0 = time.perf_counter()
match = csgraph.maximum_bipartite_matching(S, perm_type="row")
ncomp, _ = csgraph.connected_components(S, directed=True, connection="strong")
print((time.perf_counter() - t0) * 1e3, int(np.sum(match >= 0)), int(ncomp))
"""


def scipy_baseline(A, limit):
    """scipy's maximum_bipartite_matching + strong connected_components of A on the host, in a child process that
    never touches the GPU; None when it runs past `limit` seconds."""
    p, i = host_arrays(A)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, "a.npz")
        np.savez(f, p=p, i=i, shape=np.array([A.m, A.n]))
        try:
            r = subprocess.run([sys.executable, "-c", SCIPY_CHILD, f], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            return None
    ms, rank, ncomp = r.stdout.split()
    return dict(scipy_match_scc_ms=float(ms), scipy_sprank=int(rank), scipy_scc=int(ncomp))


def block_lower_bidiagonal(k):
    b = np.arange(k)
    r = np.concatenate([2 * b, 2 * b + 1, 2 * b, 2 * b + 1, 2 * b[1:]])
    c = np.concatenate([2 * b, 2 * b, 2 * b + 1, 2 * b + 1, 2 * b[:-1]])
    import scipy.sparse as sp
    S = sp.csc_matrix((np.ones(len(r)), (r, c)), shape=(2 * k, 2 * k))
    S.sort_indices()
    return S.indptr, S.indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-scipy", action="store_true")
    ap.add_argument("--scipy-limit", type=float, default=120.0, help="seconds before the scipy baseline is given up")
    ap.add_argument("--only", default="", help="comma-separated matrix names")
    a = ap.parse_args()
    _csx.init(0)
    import test_gpu_dmperm as T
    cases = [
        ("grand_5M_64", lambda: gen("csx_gen_grand_uniform", 5_000_000, 64, 20240601 + 1)),
        ("gspd_config5", lambda: gen("csx_gen_gspd", 78125, 64, 20240601 + 5)),
        ("planted_1M", lambda: (lambda m, n, S, e: upload(n, S.indptr, S.indices))(*T.planted(1_000_000, 11))),
        ("chain_200k", lambda: upload(200_000, *chain(200_000, 5))),
        ("block_lower_chain_20k", lambda: upload(40_000, *block_lower_bidiagonal(20_000))),
    ]
    for name, make in cases:
        if a.only and name not in a.only.split(","):
            continue
        A = make()
        n = A.n
        cs.dmperm_arrays(A, 0)                      # warm: row view cached, code loaded
        calls = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            d = cs.dmperm_arrays(A, 0)
            calls.append((time.perf_counter() - t0) * 1e3)
            st = cs.dmperm_times()
        out = dict(matrix=name, n=n, nnz=A._dev.info()[2], nb=d["nb"], sprank=int(d["rr"][3]),
                   call_ms=min(calls), device_ms=st, rounds=cs.dmperm_rounds())
        print(json.dumps(out), flush=True)
        if not a.skip_scipy:
            b = scipy_baseline(A, a.scipy_limit)
            b = b or dict(scipy_match_scc_ms="not measured (over %g s)" % a.scipy_limit)
            print(json.dumps(dict(matrix=name, **b)), flush=True)


if __name__ == "__main__":
    main()
