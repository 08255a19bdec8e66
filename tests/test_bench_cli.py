"""bench.py's two kinds of run: a plain one does the headline alone (set up, warm up, time the steps, dump, print
the line); --full adds every check and leg beside it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup",
            "config", "roofline")
FULL_ONLY = ("parity_on_the_timed_matrix", "headline_trials", "gaxpy_grand_other_row_draw", "gaxpy_gspd",
             "other_configs", "cpu_baseline", "cpu_baseline_c", "exchange_preflight")


def _bench(args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, text=True, timeout=timeout)


def _line(r):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_force_sharded_without_full_is_refused():
    """The column-sharded SpMV is a leg of --full: asking for it in a plain run is an error, not a silent no-op."""
    r = _bench(["--force-sharded"], timeout=60)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_legs(tmp_path):
    n, steps, warmup = 200000, 3, 1
    d = _line(_bench(["--n", str(n), "--steps", str(steps), "--warmup", str(warmup), "--mode", "tiled",
                      "--dump-outputs", str(tmp_path / "plain")]))
    assert all(k in d for k in HEADLINE), sorted(d)
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "GB/s" and d["dtype"] == "f64"
    assert (d["n_gpus"], d["steps"], d["warmup"]) == (1, steps, warmup) and d["higher_is_better"] is True
    assert not [k for k in FULL_ONLY + ("cholsol",) if k in d], sorted(d)
    y = np.load(str(tmp_path / "plain" / "y.npy"))
    assert y.shape == (n,) and np.all(np.isfinite(y))

    f = _line(_bench(["--n", str(n), "--steps", str(steps), "--warmup", str(warmup), "--mode", "tiled",
                      "--nrhs", "64", "--full", "--skip-cpu", "--skip-configs", "--dump-outputs", str(tmp_path / "full")]))
    assert all(k in f for k in HEADLINE)
    assert f["parity_on_the_timed_matrix"]["ok"] is True
    assert len(f["headline_trials"]["ms_per_step"]) == 4
    assert "gaxpy_grand_other_row_draw" in f and "gaxpy_gspd" in f and f["cholsol"]["solves_per_s"] > 0
    # the timed steps and their inputs are the same in both kinds of run: y agrees to the kernel's rounding
    yf = np.load(str(tmp_path / "full" / "y.npy"))
    nz = y != 0
    assert np.all(yf[~nz] == 0) and np.max(np.abs(yf[nz] - y[nz]) / np.abs(y[nz])) < 1e-12
