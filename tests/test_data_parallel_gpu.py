"""-m gpu: the HIP model + GradBucket + direct weight-gradient accumulation under torch.distributed on the hardware
(last row; reference trainer.py:69-89).  The box has ONE MI355X, so: (a) two ranks share cuda:0 and reduce
over gloo -- everything but the transport is the 8-GPU code path; (b) a 1-rank RCCL ("nccl") group runs the real
collective library on the flat bucket; (c) bench.py's own N > 1 path with --check-dp; (d) the multi-rank mosaic.
Ranks are fresh child processes (torch.distributed.run), started before they touch the GPU."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "dp_worker.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch(nproc, script_args, timeout=900):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port())] + script_args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"{' '.join(cmd)}\n--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    return r


@pytest.mark.gpu
def test_two_ranks_hip_model_equals_single_process(tmp_path):
    out = str(tmp_path / "dp.json")
    _launch(2, [WORKER, "dp", out])
    res = json.load(open(out))
    assert res["world"] == 2 and res["identical_replicas"]
    # 2 + 2 tiles summed per rank then across ranks vs 4 tiles summed in order: fp32 re-association only
    assert res["grad_max_rel"] <= 2e-5, res
    # AdamW, lr 1e-3: its first step moves every weight by lr * g / (|g| + eps), so where a gradient element lies within the
    # re-association noise above (the composed maps' gradients are back-propagated on per-rank sums, then reduced; the
    # convolutions sum in another order per rank count) the step itself is noise, up to 2 lr apart.  Where the gradient stands
    # 100 x clear of that noise the post-step weights agree to lr / 50; everywhere they stay within the 2 lr bound; a lost rank
    # contribution would move the significant weights by ~1e-3
    msg = {k: res[k] for k in ("param_max_abs", "param_max_abs_significant", "significant_fraction", "grad_max_rel",
                               "clear_fraction", "param_max_abs_clear")}
    assert res["significant_fraction"] > 0.02 and res["param_max_abs_significant"] <= 2e-5, msg
    # r05: per element (the 2 lr bound of r04 could never fail and is gone): every weight whose own gradient is 100 x clear of its
    # own re-association difference -- the large majority -- moves identically to lr / 100
    assert res["clear_fraction"] > 0.5 and res["param_max_abs_clear"] <= 1e-5, msg
    assert abs(res["loss_dp"] - res["loss_single"]) <= 1e-5 * abs(res["loss_single"])
    assert len(res["none_grad"]) == 8 and all("up_convs.3." in k for k in res["none_grad"])     # alto.py:241-242
    assert res["bucket"] == res["bucket_single"] >= res["live"] and res["bucket_views_aligned"]


@pytest.mark.gpu
def test_one_rank_rccl_group_is_bit_identical(tmp_path):
    out = str(tmp_path / "rccl1.json")
    _launch(1, [WORKER, "rccl1", out])
    res = json.load(open(out))
    assert res == {"backend": "nccl", "grad_equal": True, "param_equal": True, "loss_equal": True, "f64_ok": True}


@pytest.mark.gpu
def test_one_rank_rccl_with_the_trainer_defaults_over_two_optimizer_steps(tmp_path):
    """What eight real ranks run, on the one GPU a rank owns: tile pipeline + weight-gradient side streams + coalesced tiles + RCCL
    all-reduce + optimizer boundary, twice -- bit-identical to the loop without a process group (dp_worker.run_rccl1_full)."""
    out = str(tmp_path / "rccl1_full.json")
    _launch(1, [WORKER, "rccl1_full", out])
    res = json.load(open(out))
    assert res == {"backend": "nccl", "boundaries": 2, "grad_equal": [True, True], "grads_differ_between_steps": True,
                   "loss_equal": True, "param_equal": True,
                   "pipeline_and_side_streams_used": [[True, True, True], [True, True, True]]}, res


@pytest.mark.gpu
def test_multi_rank_mosaic_equals_single(tmp_path):
    out = str(tmp_path / "mosaic.json")
    _launch(2, [WORKER, "mosaic", out])
    res = json.load(open(out))
    assert not res["nan"] and res["max_abs"] <= 1e-12 * max(res["scale"], 1.0), res


@pytest.mark.gpu
def test_bench_two_ranks_check_dp_line_is_compact():
    r = _launch(2, [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--steps", "4",
                    "--warmup", "1", "--points", "8192", "--optimize-every", "4", "--profile-steps", "2", "--full",
                    "--kernel-table", os.path.join(ROOT, "gpurun_out", "bench_kernels_test.json")])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.rstrip().endswith(lines[0]), "the JSON line must be the last thing on stdout"
    assert len(lines[0]) <= 4096
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["optimizer_steps_in_timed_region"] == 2
    assert d["check_dp"]["max_rel_diff"] <= 2e-5 and d["check_dp"]["replicas_identical"]      # on by default for N > 1
    assert d["config"]["rccl_ranks"] == 0 and d["config"]["collective"] == "gloo"             # (RCCL needs one GPU per rank)
    assert "roofline" in d and d["roofline"]["frac"] > 0


@pytest.mark.gpu
def test_bench_gpus_two_without_a_launcher():
    """`python bench.py --gpus 2 ...` exactly as the round driver starts it (no torchrun on the command line): bench.py
    starts its own ranks as a child process and re-prints rank 0's line last."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--steps", "4",
           "--warmup", "1", "--points", "8192", "--optimize-every", "4", "--profile-steps", "2", "--sustain-s", "0", "--full",
           "--kernel-table", os.path.join(ROOT, "gpurun_out", "bench_kernels_test.json")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.rstrip().endswith(lines[0]) and len(lines[0]) <= 4096
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["check_dp"]["max_rel_diff"] <= 2e-5 and d["check_dp"]["replicas_identical"]
    assert d["config"]["optimizer_steps_in_timed_region"] == 2


@pytest.mark.gpu
def test_bench_eight_ranks_dry_run_on_one_gpu():
    """`python bench.py --gpus 8` as the driver will start it on an 8-GPU node, here with the eight ranks
    sharing the one GPU over gloo (everything but the transport and the device placement is the 8-GPU path): the launcher, the
    flat bucket + all-reduce per optimizer step (64 / 8 = 8 tiles per rank), check_dp, and what eight ranks cost the HOST
    (CPU time per rank and tile, reported in `sustained`)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("OMP_NUM_THREADS", None)                      # bench.py's launcher sets cores / ranks
    out = os.path.join(ROOT, "gpurun_out", "bench_8rank_dry_run.json")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--backend", "gloo", "--share-gpu", "--steps", "8",
           "--warmup", "2", "--profile-steps", "0", "--sustain-s", "2", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, f"--- stdout\n{r.stdout[-4000:]}\n--- stderr\n{r.stderr[-6000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.rstrip().endswith(lines[0]) and len(lines[0]) <= 4096
    d = json.loads(lines[0])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(lines[0] + "\n")
    assert d["n_gpus"] == 8 and d["config"]["parallelism"] == "dp8" and d["config"]["points_per_tile"] == 131072
    assert d["config"]["optimizer_steps_in_timed_region"] == 1                      # 8 tiles per rank = one 64-tile step
    assert d["check_dp"]["max_rel_diff"] <= 2e-5 and d["check_dp"]["replicas_identical"], d["check_dp"]
    assert d["sustained"]["host_cpu_ms_per_step"] > 0
    # r05: every rank bound to its own cores before it touched the GPU (bench.pin_rank), and the line says what each rank's host did
    ranks = d["ranks"]
    assert len(ranks["host_cpu_ms_per_step"]) == 8 and all(v > 0 for v in ranks["host_cpu_ms_per_step"])
    if (os.cpu_count() or 1) >= 8:
        assert ranks["affinity_disjoint"] and all(c >= 1 for c in ranks["cores_per_rank"]), ranks
