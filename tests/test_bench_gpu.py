"""-m gpu: what a plain `bench.py --gpus 1 --steps K --warmup W` run does and what `--dump-outputs` writes.  The plain run times
its K steps and prints the line without the legs of `--full`; the dump holds the last timed step's results, and a second run
with the same arguments sees the same inputs and computes the same results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("sustained", "sustained_ms_per_step", "exact_split", "strict_b1", "micro_batched", "roofline",
             "roofline_scatter_reduce", "roofline_top_symbols", "cpu_baseline", "check_dp", "ranks")


def _plain_run(dump_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--points", "8192",
           "--optimize-every", "4", "--dump-outputs", str(dump_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.rstrip().endswith(lines[0])
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        lines.append(_plain_run(d))
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 4 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    assert line["config"]["optimizer_steps_in_timed_region"] == 1            # the 4th timed tile ends the optimizer step
    assert not [k for k in FULL_ONLY if k in line], "a plain run measures only its timed steps"
    assert "optimizer_boundary_ms" not in line["config"]

    files = dumps[0]
    assert sorted(files) == ["grad", "loss", "loss_ce", "loss_l1", "params"]
    assert sum(os.path.getsize(tmp_path / "run0" / f"{k}.npy") for k in files) <= 64_000_000
    for k, a in files.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), k
    assert files["loss"][0] > 0 and np.count_nonzero(files["grad"]) > files["grad"].size // 2

    # same arguments -> same inputs -> the same results (fp32 summation order at most)
    again = dumps[1]
    assert sorted(again) == sorted(files)
    for k in ("loss", "loss_l1", "loss_ce"):
        assert abs(again[k][0] - files[k][0]) <= 1e-6 * max(abs(files[k][0]), 1e-30), k
    g0, g1 = files["grad"], again["grad"]
    assert g0.shape == g1.shape and np.abs(g1 - g0).max() <= 1e-5 * np.abs(g0).max()
    # two AdamW steps of lr 1e-4: an element whose gradient lies within that noise may step the other way (2 lr apart at most)
    assert files["params"].shape == again["params"].shape and np.abs(again["params"] - files["params"]).max() <= 4e-4
