"""The T2H_* environment switches of the package and its library: THE list, and their one parser (no torch, no _lib).
Row: kind ("flag" = 0 / 1, "int", "float", "str", or a tuple of accepted strings), default, owner (the one file of this package that
reads the name), doc (what 0 / the other value selects), scope ("ab" when absent: tests/test_switches.py flips it; "lab"; "env"),
library (True: libt2h_hip.so reads it at ``owner`` through env_flag / env_ll of csrc/t2h_common.h: a flag is off only when the value
starts with 0, a number is atoll), mirror (a Python module that reads a library switch too), covered_by (another GPU test that
flips it).  tests/test_switches_cpu.py holds the table to the sources."""
import os

SWITCHES = {
    # ---- where things are found, how they are built
    "T2H_LIBRARY": dict(kind="str", default=None, owner="_lib.py", scope="env",
        doc="path of another build of the same ABI (A/B runs of a kernel change; a site-specific install path)"),
    "T2H_ALLOW_LIBRARY_FALLBACK": dict(kind="flag", default=False, owner="_lib.py", scope="env",
        doc="1: shapes without a t2h kernel run on MIOpen / rocBLAS / ATen (counted) instead of raising"),
    "T2H_BUILD_JOBS": dict(kind="int", default=6, owner="csrc/build.py", scope="env", doc="sources compiled in parallel"),
    "T2H_LLVM_BIN": dict(kind="str", default="/opt/rocm/lib/llvm/bin", owner="csrc/build.py", scope="env",
        doc="clang / lld / clang-offload-bundler of compile_through_assembly"),
    # ---- lab only
    "T2H_CACHE_READY": dict(kind="flag", default=True, owner="_lib.py", scope="lab",
        doc="0: lazily filled cache entries are NOT waited for across streams -- the r04-r06 race, kept to show its tests catching it"),
    "T2H_POISON_LDS": dict(kind="flag", default=False, owner="_lib.py", scope="lab",
        doc="1: NaN patterns into every free CU's LDS before every entry point (t2h_debug_poison_lds)"),
    "T2H_SEAM_SYNC_CHECK": dict(kind="flag", default=False, owner="ops.py", scope="lab",
        doc="1 (debugging): every seam call waits for its own index check and raises at the call, like torch_scatter"),
    # ---- trainer.py: read when a Trainer is constructed (T2H_BATCH_REDUCE: in every backward)
    "T2H_DIRECT_ACCUM": dict(kind="flag", default=True, owner="trainer.py",
        doc="0: autograd's own gradient accumulation instead of kernels adding straight into the bucket"),
    "T2H_OVERLAP_WGRAD": dict(kind="flag", default=True, owner="trainer.py",
        doc="0: the weight-gradient GEMMs stay on the step's stream (1: a side stream, joined after the backward)"),
    "T2H_OVERLAP_CONV_WGRAD": dict(kind="flag", default=True, owner="trainer.py",
        doc="0: the convolutions' weight gradients stay on the step's stream (1: beside the next data gradients)"),
    "T2H_PIPELINE_TILES": dict(kind="flag", default=True, owner="trainer.py",
        doc="0: one tile after the other (1: tile i + 1's forward beside tile i's backward, two streams)"),
    "T2H_PIPELINE_MICRO_BATCHES": dict(kind="flag", default=True, owner="trainer.py", doc="0: a micro-batch of a window runs on the caller's stream alone"),
    "T2H_COALESCE_TILES": dict(kind="int", default=4, owner="trainer.py", covered_by="tests/test_launch_census.py",
        doc="single tiles issued as one ragged micro-batch of this many; 1: the strict B = 1 step"),
    "T2H_COMPOSE_CACHE": dict(kind="flag", default=True, owner="trainer.py",
        doc="0: the composed maps of the deferred levels are back-propagated per tile, not once per step"),
    "T2H_BATCH_REDUCE": dict(kind="flag", default=True, owner="trainer.py",
        doc="0: one slab reduction launch per layer instead of one batched launch per pass (only without the side streams)"),
    # ---- the grid side (grid.py, csrc/conv.hip, csrc/conv_bx3.hip)
    "T2H_HIP_CONV": dict(kind="flag", default=True, owner="grid.py",
        doc="0: every convolution stays on MIOpen (an explicit request, so it also allows the fallbacks)"),
    "T2H_CONV_PRECISION": dict(kind=("fp32", "bf16x3", "f16x2", "bf16"), default="f16x2", owner="grid.py",
        doc="arithmetic of the 3x3 / transposed convolutions and the wide grid-side products (grid.py, above CONV_PRECISION)"),
    "T2H_BX3_MIN_PIXELS": dict(kind="int", default=1024, owner="grid.py", doc="smaller planes stay on conv.hip"),
    "T2H_BX3_WGRAD": dict(kind="flag", default=True, owner="grid.py", doc="0: weight gradients stay on conv.hip"),
    "T2H_UPCONV_BX3": dict(kind="flag", default=True, owner="grid.py", doc="0: transposed convolutions stay on conv.hip (fp32 MFMA)"),
    "T2H_HEAD_RANK1": dict(kind="flag", default=True, owner="grid.py",
        doc="0: the 1 x 1 head writes its share of the decoder gradients, the data gradients accumulate onto it (bit-identical)"),
    "T2H_OVERLAP_CONV_MAX_PIXELS": dict(kind="int", default=512 * 512, owner="grid.py",
        doc="planes up to here send their weight gradients to the trainer's side stream"),
    "T2H_CONV_ROWS_WGS_SMALL": dict(kind="int", default=768, owner="csrc/conv.hip", library=True,
        doc="workgroups the split reduction aims at, up to 16384 output rows"),
    "T2H_CONV_ROWS_WGS_LARGE": dict(kind="int", default=512, owner="csrc/conv.hip", library=True,
        doc="workgroups the split reduction aims at, above 16384 output rows"),
    "T2H_UPCONV_FWD_TILES": dict(kind="int", default=256, owner="csrc/conv.hip", library=True,
        doc="the transposed convolution's column tiles narrow until there are this many tiles"),
    "T2H_CONV_WGRAD_WGS": dict(kind="int", default=0, owner="csrc/conv.hip", library=True,
        doc="workgroups the weight gradient aims at (0: 512 for planes up to 128 x 128, else 1024)"),
    "T2H_BX3_TILES8": dict(kind="int", default=1024, owner="csrc/conv_bx3.hip", library=True, doc="8-row tiles from this many tiles on"),
    "T2H_BX3_NARROW": dict(kind="flag", default=True, owner="csrc/conv_bx3.hip", library=True,
        doc="0: small planes with short reductions keep 128-column tiles and split the reduction"),
    "T2H_BX3_ROWS_WGS": dict(kind="int", default=512, owner="csrc/conv_bx3.hip", library=True, doc="workgroups the split reduction aims at"),
    "T2H_BX3_WGRAD_WGS": dict(kind="int", default=0, owner="csrc/conv_bx3.hip", library=True,
        doc="workgroups the split weight gradient aims at (0: 256 for planes up to 128 x 128, else 512)"),
    "T2H_BX3_UPWGRAD_WGS": dict(kind="int", default=0, owner="csrc/conv_bx3.hip", library=True,
        doc="workgroups the transposed convolution's weight gradient aims at (0: 256)"),
    # ---- the split per-pixel products (mlp.py, csrc/conv_bx3.hip, 1-tap form)
    "T2H_GEMM_BX3": dict(kind="flag", default=True, owner="mlp.py", doc="0: the grid-side products of the deferred point update stay on the fp32 MFMA kernels"),
    "T2H_GEMM_BX3_MIN_N": dict(kind="int", default=64, owner="mlp.py", doc="fewer output columns stay on the fp32 kernels"),
    "T2H_GEMM_BX3_MIN_K": dict(kind="int", default=128, owner="mlp.py", doc="shorter reductions stay on the fp32 kernels"),
    "T2H_GEMM_BX3_WGRAD": dict(kind="flag", default=False, owner="mlp.py",
        doc="1: the wide weight gradients dW = dY^T X on the split kernels too (t2h_gemm_bx3_wgrad)"),
    "T2H_GEMM_BX3_WGRAD_MIN_N": dict(kind="int", default=1024, owner="mlp.py", doc="... from this many columns of dY on"),
    "T2H_GEMM_BX3_WGRAD_MIN_M": dict(kind="int", default=4096, owner="mlp.py", doc="... and from this many rows on"),
    "T2H_GEMM_BX3_WGRAD_WGS": dict(kind="int", default=4096, owner="csrc/conv_bx3.hip", library=True,
        doc="workgroups that weight gradient's row split aims at"),
    "T2H_BX3_PERSIST_N": dict(kind="flag", default=True, owner="csrc/conv_bx3.hip", library=True, mirror="mlp.py",
        doc="0: no persistent form (rows staged and split once per workgroup, reused for all its column tiles) for one-chunk "
            "reductions into a wide matrix; mlp.py routes such shapes by it"),
    "T2H_BX3_PERSIST_WGS": dict(kind="int", default=2048, owner="csrc/conv_bx3.hip", library=True,
        doc="workgroups of the persistent form: column groups = this / row tiles"),
    "T2H_BX3_PERSIST_MIN_GROUPS": dict(kind="int", default=4, owner="csrc/conv_bx3.hip", library=True,
        doc="... but at least this many column groups however many row tiles there are"),
    # ---- the per-point GEMMs (csrc/gemm.hip)
    "T2H_GEMM_DMA": dict(kind="flag", default=True, owner="csrc/gemm.hip", library=True,
        doc="0: the register-staged kernels instead of the LDS-DMA ones (forward, data and TN weight gradient)"),
    "T2H_SKINNY": dict(kind="flag", default=True, owner="csrc/gemm.hip", library=True,
        doc="0: no 64 x 64 x 32 tiles for 33 .. 64 output columns from a long reduction"),
    "T2H_SMALLM_BK": dict(kind="int", default=64, owner="csrc/gemm.hip", library=True, doc="slab depth of the small-tile kernels for few rows (64 / 32 / 16)"),
    "T2H_KWAVES_MIN_K": dict(kind="int", default=256, owner="csrc/gemm.hip", library=True,
        doc="the four waves of a workgroup split reductions from this depth on"),
    "T2H_KWAVES_MAX_TILES": dict(kind="int", default=1024, owner="csrc/gemm.hip", library=True, doc="... for outputs of up to this many 32 x 32 tiles"),
    "T2H_KWAVES_WGRAD_MAX_ROWS": dict(kind="int", default=1024, owner="csrc/gemm.hip", library=True,
        doc="the weight gradient takes that one-launch form up to this many rows"),
    # ---- the point trunk and the grid-first / deferred point update (mlp.py, deferred.py, ops.py, csrc/point_grid.hip)
    "T2H_FUSED_TRUNK": dict(kind="flag", default=True, owner="mlp.py", doc="0: one GEMM launch per Linear + pool kernels"),
    "T2H_TRUNK_FUSED": dict(kind=("auto", "1", "0"), default="auto", owner="mlp.py",
        doc="auto and 1: the whole trunk forward in one launch from _TRUNK_FUSED_MIN_ROWS rows on; 0: one launch per block"),
    "T2H_TRUNK_FUSED_STRIDE": dict(kind="int", default=0, owner="mlp.py",
        doc="rows per fixed-stride window of the one launch without unit bounds (0: 96; at most 128)"),
    "T2H_TRUNK_UNIT_BOUNDS": dict(kind="flag", default=True, owner="mlp.py",
        doc="0: fixed-stride windows looked up in the kernel (1: greedy units built once per tile index)"),
    "T2H_GRID_FIRST_MIN_RATIO": dict(kind="float", default=4.0, owner="mlp.py", doc="points per pixel from which fc_comm.0 runs on the pixels; 0: never"),
    "T2H_DEFER_MIN_CHANNELS": dict(kind="int", default=128, owner="deferred.py", doc="deferral starts at the first level with this many channels; 0: off"),
    "T2H_FUSED_SAMPLE_BWD": dict(kind="flag", default=True, owner="deferred.py", doc="0: separate gather + sample adjoint"),
    "T2H_SIGN_BITS": dict(kind="flag", default=True, owner="deferred.py", doc="0: keep the hidden activations for the mask"),
    "T2H_ON_CHIP_HIDDEN": dict(kind="flag", default=True, owner="deferred.py", doc="0: sample kernel + per-cell sum kernel"),
    "T2H_ON_CHIP_MIN_PTS": dict(kind="float", default=8.0, owner="deferred.py",
        doc="points per cell from which the on-chip walk is taken (it is sequential inside a cell)"),
    "T2H_COMPACT_SUMS": dict(kind="flag", default=True, owner="deferred.py",
        doc="0: one row per CELL in the sum matrices of every resolution (1: the finest deferred resolution holds one row per OCCUPIED cell)"),
    "T2H_SAMPLE_ADJOINT": dict(kind="flag", default=True, owner="ops.py", doc="0: no sample backward through the cached transposed matrix"),
    "T2H_SAMPLE_ADJOINT_MAX_ROWS": dict(kind="float", default=4.0, owner="ops.py",
        doc="rows per pixel above which t2h_sample_bwd's gather / per-cell partials stay"),
    "T2H_CELLS_MFMA": dict(kind="flag", default=True, owner="csrc/point_grid.hip", library=True, mirror="deferred.py",
        doc="0: the VALU form of the sample adjoint's per-cell partials; deferred.py's bit mask needs the matrix-core form"),
    "T2H_CELLS_MIN_WGS": dict(kind="int", default=4096, owner="csrc/point_grid.hip", library=True, doc="workgroups the per-cell partials' row splits aim at"),
    "T2H_CELLS_TABLE": dict(kind="int", default=1, owner="csrc/point_grid.hip", library=True,
        doc="0: no cell table in the matrix-core partials (the r04 walk)"),
    # ---- PointNet++ (pointops.py): read at the call
    "T2H_FPS_SLICE": dict(kind="int", default=None, owner="pointops.py", covered_by="tests/test_pnpp_gpu.py",
        doc="set (a multiple of 64): EVERY cloud takes the sliced farthest-point sampling with that slice"),
}


def get(name, environ=None):
    """The parsed value of switch ``name`` in ``os.environ`` (or the mapping given) at the moment of the call."""
    row = SWITCHES[name]
    raw, kind = (os.environ if environ is None else environ).get(name), row["kind"]
    if raw is None:
        return row["default"]
    if kind in ("int", "float", "str"):
        return {"int": int, "float": float, "str": str}[kind](raw)
    accepted = ("0", "1") if kind == "flag" else kind
    if raw not in accepted:
        raise ValueError(f"{name}={raw!r}: expected one of {accepted}")
    return raw == "1" if kind == "flag" else raw
