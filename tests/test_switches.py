"""-m gpu: the A/B switches of tomosar2height_amd/switches.py (the rows of scope "ab") FLIPPED: each of them is set to a value other
than its default by at least one group of GROUPS below, or by the GPU test its row names as `covered_by` -- which
tests/test_switches_cpu.py checks row by row, without a GPU (GPUTEST used to exercise the defaults only).
The "lab" and "env" rows are not flipped here.  The switches are read at import time or on first use, so each group runs in a fresh worker process
(tests/switch_worker.py): one forward + backward of the Berlin network and three pipelined Trainer steps.  Asserted per group:
heights within 1e-4 of the CPU oracle (north_star), every gradient finite and within the mask-flip resolution of the default
run (cosine similarity >= 0.9999: see _close_grads), the Trainer's accumulated loss / gradients likewise, and no
vendor-library fallback (except where the switch asks for one)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from detinit import det_init_, synth_cloud

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GROUPS = {
    "default": {},
    # the on-chip walks: no cell table in the matrix-core partials; fewer workgroups for the per-cell partials
    "walks_r04": {"T2H_CELLS_TABLE": "0"},
    "walks_blocks": {"T2H_CELLS_MIN_WGS": "1024"},
    # the hidden activations written out / kept / two-pass backward; the VALU partials
    "hidden_in_memory": {"T2H_ON_CHIP_HIDDEN": "0", "T2H_SIGN_BITS": "0", "T2H_FUSED_SAMPLE_BWD": "0"},
    "partials_valu": {"T2H_CELLS_MFMA": "0", "T2H_SAMPLE_ADJOINT": "0", "T2H_ON_CHIP_MIN_PTS": "2"},
    # trainer: no cache of the composed maps, autograd's own gradient accumulation, one stream, tiles one after the other
    "trainer_plain": {"T2H_COMPOSE_CACHE": "0", "T2H_DIRECT_ACCUM": "0", "T2H_OVERLAP_WGRAD": "0", "T2H_OVERLAP_CONV_WGRAD": "0",
                      "T2H_PIPELINE_TILES": "0"},
    "trainer_batched_reductions": {"T2H_OVERLAP_WGRAD": "0", "T2H_OVERLAP_CONV_WGRAD": "0", "T2H_BATCH_REDUCE": "1",
                                   "T2H_OVERLAP_CONV_MAX_PIXELS": "4096"},
    "trainer_unbatched": {"T2H_OVERLAP_WGRAD": "0", "T2H_OVERLAP_CONV_WGRAD": "0", "T2H_BATCH_REDUCE": "0"},
    # convolution arithmetics and kernel families
    "conv_bf16x3": {"T2H_CONV_PRECISION": "bf16x3", "T2H_BX3_NARROW": "0", "T2H_BX3_TILES8": "1000000", "T2H_BX3_ROWS_WGS": "128",
                    "T2H_BX3_WGRAD_WGS": "128", "T2H_BX3_UPWGRAD_WGS": "128"},
    "conv_fp32_mfma": {"T2H_CONV_PRECISION": "fp32", "T2H_CONV_ROWS_WGS_SMALL": "256", "T2H_CONV_ROWS_WGS_LARGE": "256",
                       "T2H_CONV_WGRAD_WGS": "128", "T2H_UPCONV_FWD_TILES": "64"},
    "conv_mixed": {"T2H_BX3_WGRAD": "0", "T2H_UPCONV_BX3": "0", "T2H_GEMM_BX3": "0", "T2H_BX3_MIN_PIXELS": "16384"},
    "gemm_bx3_wide": {"T2H_GEMM_BX3_MIN_N": "32", "T2H_GEMM_BX3_MIN_K": "64", "T2H_BX3_PERSIST_WGS": "512"},
    "gemm_bx3_wgrad_split": {"T2H_GEMM_BX3_WGRAD": "1", "T2H_GEMM_BX3_WGRAD_WGS": "1024"},        # r06: the wide weight gradients on the split TN form
    "head_rank1_off": {"T2H_HEAD_RANK1": "0"},                  # r06: the head writes its share of the decoder gradients, the data gradients accumulate
    "gemm_bx3_narrow": {"T2H_GEMM_BX3_MIN_N": "128", "T2H_BX3_PERSIST_N": "0"},            # (the default until r05's last day: 64-wide outputs on the fp32 kernels)
    # per-point GEMM families, trunk forms, grid-first / deferred thresholds
    "gemm_plain": {"T2H_GEMM_DMA": "0", "T2H_SKINNY": "0", "T2H_SMALLM_BK": "16", "T2H_KWAVES_MIN_K": "100000"},
    "gemm_kwaves": {"T2H_KWAVES_MIN_K": "64", "T2H_KWAVES_MAX_TILES": "100000", "T2H_KWAVES_WGRAD_MAX_ROWS": "100000"},
    "trunk_unfused": {"T2H_FUSED_TRUNK": "0"},
    # r06: the whole trunk forward in one launch (greedy work units per tile index; fixed-stride windows looked up in the launch),
    # coalescing off / eight tiles, micro-batches outside the tile pipeline
    "trunk_one_launch": {"T2H_TRUNK_FUSED": "1"},
    "trunk_five_launches": {"T2H_TRUNK_FUSED": "0"},
    "trunk_one_launch_strided": {"T2H_TRUNK_FUSED": "1", "T2H_TRUNK_UNIT_BOUNDS": "0", "T2H_TRUNK_FUSED_STRIDE": "112"},
    "trainer_tile_by_tile": {"T2H_COALESCE_TILES": "1"},
    "trainer_coalesce_two_unpipelined": {"T2H_COALESCE_TILES": "2", "T2H_PIPELINE_MICRO_BATCHES": "0"},
    "point_first": {"T2H_GRID_FIRST_MIN_RATIO": "1000000"},
    "no_deferred": {"T2H_DEFER_MIN_CHANNELS": "0", "T2H_SAMPLE_ADJOINT_MAX_ROWS": "0"},
    "deferred_wide_only": {"T2H_DEFER_MIN_CHANNELS": "512", "T2H_SAMPLE_ADJOINT_MAX_ROWS": "64"},
    # one row per cell in every sum matrix; one column group in the persistent split product; the split weight gradient from
    # narrower / shorter matrices on; every convolution on the vendor library
    "dense_sums": {"T2H_COMPACT_SUMS": "0"},
    "persist_one_group": {"T2H_BX3_PERSIST_MIN_GROUPS": "1"},
    "gemm_bx3_wgrad_low_thresholds": {"T2H_GEMM_BX3_WGRAD": "1", "T2H_GEMM_BX3_WGRAD_MIN_N": "64", "T2H_GEMM_BX3_WGRAD_MIN_M": "1024"},
    "library_convs": {"T2H_HIP_CONV": "0"},
}
FALLBACK_GROUPS = ("library_convs",)        # the switch asks for the vendor library: there fallbacks MUST be counted


def _run(name, tmp_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("T2H_")}
    env.update(GROUPS[name])
    out = str(tmp_path / f"{name}.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_worker.py"), out], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, f"[{name}] {GROUPS[name]}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-5000:]}"
    info = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return info, torch.load(out, weights_only=False)


@pytest.fixture(scope="module")
def baseline(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("switches")
    info, res = _run("default", tmp)
    from oracle import torch_ref
    from tomosar2height_amd.config import berlin_config
    ref = det_init_(torch_ref.TomoSAR2Height(berlin_config()), seed=41)
    with torch.no_grad():
        pa_ref, _ = ref(input_cloud=synth_cloud(40000, seed=5))
    return info, res, pa_ref


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / (np.abs(want).max() + 1e-30)


def _close_grads(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        a, b = got[k].double(), want[k].double()
        mx = _rel(a.numpy(), b.numpy())
        l2 = ((a - b).norm() / (b.norm() + 1e-30)).item()
        # This test is about COVERAGE of the alternative paths (do they run, do they compute the same function), not about their
        # arithmetic, which the per-path tests pin (test_hip_gemm / _conv / _deferred / _trunk / _masks).  Two fp32 runs with
        # different summation orders differ by ReLU / arg-max mask flips, most in the first trunk layers whose gradient has
        # passed every mask of the network (measured here: up to 4.6e-3 L2 on blocks.0.fc_0.weight); a wrong path is off by
        # order 1.  Bound: cosine similarity >= 0.9999 (L2 <= 1.4e-2) and 3e-2 max-normalised.
        assert mx <= 3e-2 and l2 <= 1.4e-2, f"{what} {k}: {mx:.2e} max-normalised, {l2:.2e} L2 vs the default run"


def test_default_run_matches_the_oracle(baseline):
    info, res, pa_ref = baseline
    assert info["finite"] and info["fallbacks"] == 0 and info["n_grads"] == 147
    assert _rel(res["heights"].numpy(), pa_ref.numpy()) <= 1e-4


@pytest.mark.parametrize("name", [k for k in GROUPS if k != "default"])
def test_flipped_switches(name, baseline, tmp_path):
    _, base, pa_ref = baseline
    info, res = _run(name, tmp_path)
    assert info["finite"] and info["n_grads"] == 147, info
    if name in FALLBACK_GROUPS:
        assert info["fallbacks"] > 0, f"{name}: no vendor-library fallback counted"
    else:
        assert info["fallbacks"] == 0, f"{name}: {info['fallbacks']} vendor-library fallback(s)"
    err = _rel(res["heights"].numpy(), pa_ref.numpy())
    assert err <= 1e-4, f"{name}: heights {err:.2e} vs the CPU oracle"
    _close_grads(res["grads"], base["grads"], name)
    assert abs(res["trainer_loss"] - base["trainer_loss"]) <= 1e-5 * abs(base["trainer_loss"])
    _close_grads(res["trainer_grads"], base["trainer_grads"], name + " (trainer)")
