"""CPU (no GPU needed): the C-ABI library builds, loads, exports every symbol include/t2h.h declares, and the
product refuses to run without a device instead of falling back."""
import os
import re

import pytest
import torch

from abi_ref import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from tomosar2height_amd import _lib
    from tomosar2height_amd.csrc import build
    build.build()
    lib = _lib.load()
    declared = declared_symbols("t2h.h")
    assert len(declared) >= 36
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/t2h.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature in _lib.py"
    assert sorted(_lib.SIGNATURES) == declared
    assert lib.t2h_abi_version() == _lib.ABI_VERSION


def test_no_launch_takes_its_rows_from_a_call_before_it():
    """The compact rows of the per-cell matrices (include/t2h.h) are arguments of the launch that uses them: the entry point that
    left a request for "the next launch of this thread" is gone from the library and the binding, and no source names it, its
    thread-local or the function that took it."""
    import glob
    from tomosar2height_amd import _lib
    lib = _lib.load()
    assert not hasattr(lib, "t2h_compact_next") and not hasattr(_lib, "compact_next")
    files = (glob.glob(os.path.join(ROOT, "tomosar2height_amd", "**", "*.py"), recursive=True)
             + [f for f in glob.glob(os.path.join(ROOT, "tomosar2height_amd", "csrc", "*")) if os.path.isfile(f) and not f.endswith(".o")]
             + glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert len(files) > 40
    for f in files:
        text = open(f, errors="replace").read()
        for word in ("compact_next", "take_compact", "g_compact"):
            assert word not in text, f"{os.path.relpath(f, ROOT)} names {word}"


def test_host_side_helpers_need_no_gpu():
    from tomosar2height_amd import _lib
    lib = _lib.load()
    assert lib.t2h_pool_winner_stride(32) == 8 and lib.t2h_pool_winner_stride(6) == 6
    assert lib.t2h_tile_workspace_bytes(1, 131072, 8) >= 4 * 131072 * 4
    assert lib.t2h_tile_workspace_bytes(1, 10, 11) == 0            # nbits out of range
    # argument validation happens before any launch: null pointers are an error code, not a crash
    assert lib.t2h_segmean_fwd(None, None, 1, 100, 8, 0, 32, None, None, 0, None) == -1
    assert b"null pointer" in lib.t2h_last_error_string()


def test_on_chip_cell_sums_refuse_the_one_pixel_level():
    """t2h_sample_relu_cellsums*: level == nbits (a 1 x 1 plane) is an argument error, refused before any launch -- the on-chip
    pass has no form for it (the deferred level takes t2h_sample_fwd_relu + t2h_segsum_fwd there)."""
    import numpy as np
    from tomosar2height_amd import _lib
    lib = _lib.load()
    buf = np.zeros(4096, np.float32)                      # host memory: valid-looking, 16-byte aligned, never launched on
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    nbits = 8
    args = (p, p, 3, p, 1, 10, nbits, nbits, 0, 256, p, 256)
    for name, tail in (("t2h_sample_relu_cellsums", (None, None)), ("t2h_sample_relu_cellsums2", (None, 0, None, None)),
                       ("t2h_sample_relu_cellsums_ordered", (None, 0, None, None, None, None))):
        assert getattr(lib, name)(*args, *tail) == -1, name
        assert b"level < nbits" in lib.t2h_last_error_string(), name


def test_grid_conv_dispatch_host_logic():
    """grid.py's routing (host logic, no launches): which convolutions the implicit-GEMM kernels accept, workspace
    plans of the C side, and that geometry outside them is left to the stock module."""
    from tomosar2height_amd import _lib, grid
    lib = _lib.load()
    x = torch.rand(1, 32, 16, 16)
    assert not grid.conv3x3_supported(x, torch.nn.Conv2d(32, 32, 3, padding=1))                 # host tensor
    assert not grid.upconv2x2_supported(x, torch.nn.ConvTranspose2d(32, 16, 2, stride=2))
    meta = torch.empty(1, 32, 16, 16, device="meta")
    for conv, ok in ((torch.nn.Conv2d(32, 64, 3, padding=1), None), (torch.nn.Conv2d(32, 64, 3, padding=0), False),
                     (torch.nn.Conv2d(32, 64, 3, stride=2, padding=1), False), (torch.nn.Conv2d(24, 64, 3, padding=1), False),
                     (torch.nn.Conv2d(32, 64, 5, padding=2), False), (torch.nn.Conv2d(32, 64, 3, padding=1, groups=2), False)):
        if ok is False:
            assert not grid.conv3x3_supported(meta, conv)
    # split-reduction plans: small planes with many channels need slabs, large planes do not; weight gradients always do
    assert lib.t2h_conv3x3_fwd_workspace_bytes(1, 32, 32, 512, 512) % (1024 * 512 * 4) == 0
    assert lib.t2h_conv3x3_fwd_workspace_bytes(1, 32, 32, 512, 512) > 0
    assert lib.t2h_conv3x3_dgrad_workspace_bytes(1, 512, 512, 64, 128) == 0
    assert lib.t2h_conv3x3_wgrad_workspace_bytes(1, 512, 512, 64, 128) >= (128 * 9 * 64 + 128) * 4
    assert lib.t2h_upconv2x2_wgrad_workspace_bytes(1, 32, 32, 512, 256) >= 512 * 4 * 256 * 4
    assert lib.t2h_conv3x3_fwd_workspace_bytes(0, 32, 32, 512, 512) == 0
    # geometry errors come back as codes with a message, never as a launch
    assert lib.t2h_conv3x3_fwd(1, 1, None, 1, 1, 12, 16, 32, 32, 0, None, 0, None) < 0
    assert b"powers of two" in lib.t2h_last_error_string()
    assert lib.t2h_upconv2x2_fwd(1, 1, None, 1, 1, 16, 16, 24, 32, 0, None) < 0
    assert b"multiples of 16" in lib.t2h_last_error_string()


def test_no_cpu_fallback():
    from tomosar2height_amd.tile import TileIndex
    from tomosar2height_amd import ops
    cloud = torch.rand(1, 16, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        TileIndex(cloud, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.coordinate2index(cloud, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.upsample_bilinear(torch.rand(1, 2, 4, 4), 8)
    with pytest.raises(ValueError, match="power of two"):
        TileIndex(cloud, 12)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "tomosar2height_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"
                assert "libt2h_oracle" not in src


def test_every_entry_point_rejects_bad_arguments_without_a_gpu():
    """The C side validates before launching: null pointers / impossible sizes come back as T2H_ERR_ARG (-1) or
    T2H_ERR_WORKSPACE (-3) with a message, never a crash -- checked here without any device."""
    from tomosar2height_amd import _lib
    lib = _lib.load()
    n = None
    cases = {
        "t2h_coordinate2index": (n, 3, 10, 16, n, n),
        "t2h_tile_build": (n, 3, 1, 10, 8, n, n, n, n, n, n, 0, n),
        "t2h_tile_build_ragged": (n, 3, 2, n, 8, n, 4, n, n, n, n, n, 0, n),
        "t2h_pool_max_fwd": (n, 32, n, 1, 8, 32, n, 32, n, n),
        "t2h_pool_max_bwd": (n, 32, n, n, 1, 8, 32, 0, n, 32, n),
        "t2h_pool_mean": (n, 32, n, 1, 8, 32, 0, n, 32, n),
        "t2h_pool_rows_fwd": (n, 32, n, n, 100, 32, n, 32, n, n),
        "t2h_pool_rows_bwd": (n, 32, n, n, n, 100, 32, 0, n, 32, n),
        "t2h_segmean_fwd": (n, n, 1, 10, 8, 0, 32, n, n, 0, n),
        "t2h_segmean_bwd": (n, n, n, 1, 10, 8, 0, 32, n, n),
        "t2h_segmean_bwd_add": (n, n, n, 1, 10, 8, 0, 32, n, n, n),
        "t2h_segsum_fwd": (n, n, 1, 10, 8, 0, 32, n, 32, n, 0, n, n),
        "t2h_plane_sumpool2x2": (n, 32, 1, 32, 32, n, 32, n, n),
        "t2h_segsum_bwd_multi": (n, n, n, 1, n, 1, 10, 8, 32, n, n, n, n, n, -1),
        "t2h_cell_counts": (n, 1, 8, 0, n, n, n),
        "t2h_mean_bias_fwd": (n, n, n, 64, 32, n, n, n),
        "t2h_mean_bias_bwd": (n, n, 64, 32, n, n, n, 0, n, n),
        "t2h_sample_relu_cellsums": (n, n, 3, n, 1, 10, 8, 2, 0, 256, n, 256, n, n),
        "t2h_sample_relu_cellsums2": (n, n, 3, n, 1, 10, 8, 2, 0, 256, n, 256, n, 256, n, n),
        "t2h_sample_bwd_from_sums": (n, n, n, 1, n, n, 0, n, 3, n, 1, 10, 8, 0, 32, n, n, 0, n),
        "t2h_sample_bwd_from_sums_ordered": (n, n, n, 1, n, n, 0, n, 3, n, 1, 10, 8, 0, 32, n, n, 0, n, n, n, -1),
        "t2h_sample_relu_cellsums_ordered": (n, n, 3, n, 1, 10, 8, 2, 0, 256, n, 256, n, 256, n, n, n, n),
        "t2h_cell_order_build": (n, 1, 8, 2, n, n),
        "t2h_cell_order_build_range": (n, 1, 8, 1, 3, n, n),
        "t2h_sample_fwd": (n, n, 3, 1, 10, 32, 32, n, n),
        "t2h_sample_fwd_relu": (n, n, 3, 1, 10, 32, 32, n, n, n),
        "t2h_sample_bwd": (n, n, 3, n, 1, 10, 8, 0, 32, n, n, 0, n),
        "t2h_sample_bwd_add": (n, n, 3, n, 1, 10, 8, 0, 32, n, n, n, 0, n),
        "t2h_sample_bwd_atomic": (n, n, 3, 1, 10, 32, 32, n, n),
        "t2h_sample_adjoint_build": (n, 3, n, 1, 10, 8, 0, n, n, n),
        "t2h_sample_bwd_adjoint": (n, n, n, 1, 8, 0, 32, n, n, n),
        "t2h_linear_fwd": (n, 32, n, n, n, 32, 10, 32, 32, 0, n),
        "t2h_linear_fwd_add": (n, 32, n, n, n, 32, n, 32, 10, 32, 32, 0, n),
        "t2h_linear_dgrad": (n, 32, n, n, 32, 10, 32, 32, n, 0, 0, n),
        "t2h_linear_wgrad": (n, 32, n, 32, 10, 32, 32, 0, n, n, n, 0, n, n),
        "t2h_upsample_bilinear_fwd": (n, n, 1, 32, 16, 16, 32, 32, n, n),
        "t2h_upsample_bilinear_bwd": (n, 1, 32, 16, 16, 32, 32, n, n),
        "t2h_upsample_bilinear_nhwc_fwd": (n, n, 1, 32, 16, 16, 32, 32, n, n),
        "t2h_upsample_bilinear_nhwc_bwd": (n, 1, 32, 16, 16, 32, 32, n, n),
        "t2h_upsample2x_nhwc_fwd": (n, 1, 32, 16, 16, n, n),
        "t2h_upsample2x_nhwc_bwd": (n, 1, 32, 16, 16, n, n),
        "t2h_bias_relu_fwd": (n, n, 100, 32, 1, n),
        "t2h_bias_relu_bwd": (n, n, n, 100, 32, 1, 0, n, n, 0, n),
        "t2h_upsample_bicubic_fwd": (n, n, 1, 32, 16, 16, 32, 32, 0, n, n),
        "t2h_upsample_bicubic_bwd": (n, 1, 32, 16, 16, 32, 32, 0, n, n),
        "t2h_sample_bicubic_fwd": (n, n, 3, 1, 10, 16, 32, 0, n, n),
        "t2h_sample_bicubic_bwd": (n, n, 3, 1, 10, 16, 32, 0, n, n),
        "t2h_sample_nearest_fwd": (n, n, 3, 1, 10, 16, 32, 0, n, n),
        "t2h_sample_nearest_bwd": (n, n, 3, 1, 10, 16, 32, 0, n, n),
        "t2h_trunk_fused_fwd": (n, 3, n, n, n, 5, n, n, n, n, 100, n, n, n, n, n, 0, n, n),
        "t2h_trunk_units_build": (n, n, 100, n, n),
        "t2h_head1x1_fwd": (n, n, 4, n, n, 100, n, n),
        "t2h_head1x1_bwd": (n, n, n, 4, n, n, 100, 0, n, n, n, 0, n),
        "t2h_relu_mask": (n, n, n, 128, n),
        "t2h_conv3x3_fwd": (n, n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_conv3x3_dgrad": (n, n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_conv3x3_wgrad": (n, n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_conv3x3_bx3_prepare": (n, 32, 32, 0, n, n),
        "t2h_conv3x3_bx3_fwd": (n, n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_conv3x3_bx3_dgrad": (n, n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_conv3x3_bx3_wgrad": (n, n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_gemm_bx3_prepare": (n, 64, 64, 32, 0, n, n),
        "t2h_upconv2x2_bx3_fwd": (n, n, n, n, n, 1, 16, 16, 64, 64, 0, n),
        "t2h_upconv2x2_bx3_dgrad": (n, 64, n, n, 1, 16, 16, 64, 64, 0, n, 0, n),
        "t2h_upconv2x2_bx3_wgrad": (n, 64, n, n, n, 1, 16, 32, 64, 64, 0, n, 0, n),
        "t2h_conv3x3_f16x2_prepare": (n, 32, 32, 0, n, n),
        "t2h_gemm_f16x2_prepare": (n, 64, 64, 32, 0, n, n),
        "t2h_split_weights_batch": (n, 1, n),
        "t2h_conv3x3_bx3_dgrad_rank1": (n, n, n, n, n, n, 1, 512, 512, 64, 128, 64, n),
        "t2h_gemm_bx3_wgrad": (n, 2752, n, 64, 128, 64, 2752, n, n, 64, n, 0, n),
        "t2h_gemm_bx3": (n, 64, n, n, n, 0, n, 32, 128, 64, 32, 0, n, 0, n, n),
        "t2h_upconv2x2_fwd": (n, n, n, n, 1, 32, 32, 32, 32, 0, n),
        "t2h_upconv2x2_fwd_add": (n, n, n, n, n, 1, 32, 32, 32, 32, 0, n),
        "t2h_upconv2x2_dgrad": (n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_upconv2x2_wgrad": (n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_upconv2x2_wgrad_bias": (n, n, n, n, 1, 32, 32, 32, 32, 0, n, 0, n),
        "t2h_maxpool2x2_nhwc_fwd": (n, 1, 64, 64, 32, n, n, n),
        "t2h_maxpool2x2_nhwc_bwd": (n, n, 1, 64, 64, 32, n, n),
        "t2h_maxpool2x2_nhwc_bwd_add": (n, n, 1, 64, 64, 32, n, 32, n, n),
        "t2h_mosaic_accumulate": (n, 64, 64, n, n, n, 100, 100, 0, 0, 1, n),
        "t2h_mosaic_finalize": (n, n, 100, n),
        "t2h_tile_crop_normalise": (n, 100, 0.0, 0.0, 1.0, 1.0, 512.0, 512.0, 190.2, n, n, n, n, n, 0, n),
        "t2h_tile_crop_finish": (n, n),
        "t2h_tile_crop_normalise_aug": (n, 100, 0.0, 0.0, 1.0, 1.0, 512.0, 512.0, 190.2, 0, -1, n, n, n, n, n, 0, n),
        "t2h_raster_patch": (n, 0, 1, 64, 64, 0, 0, 16, 16, 0, -1, n, n),
        "t2h_adamw_flat_step": (n, n, 4, 1e-4, 0.9, 0.999, 1e-8, 0.01, 1, 0, n),
        "t2h_conv3x3_smallcin_fwd": (n, n, n, n, 1, 32, 32, 3, 32, 0, n),
        "t2h_conv3x3_smallcin_dgrad": (n, n, n, 1, 32, 32, 3, 32, 0, n),
        "t2h_conv3x3_smallcin_wgrad": (n, n, n, n, 1, 32, 32, 3, 32, 0, n, 0, n),
        "t2h_trunk_block_fwd": (n, 3, n, n, n, 32, n, n, n, n, n, n, n, n, n, 100, n, n, n, n, 32, n, n, n),
        "t2h_trunk_block_bwd": (n, 32, n, 32, n, n, n, n, n, n, n, n, 32, n, 32, n, 3, n, n, n, n, n, 100, n, n, 0, n),
        "t2h_trunk_block_reduce": (n, 100, 0, 0, n, n, n, n, n, n, n, 0, n),
        "t2h_scatter_max_fwd": (n, 32, n, n, 1, 100, 4, 32, n, n, n),
        "t2h_scatter_max_bwd": (n, n, 1, 32, 100, 256, n, n),
        "t2h_nchw_to_nhwc": (n, 1, 32, 64, n, n),
        "t2h_nhwc_to_nchw": (n, 1, 32, 64, n, n),
    }
    launching = [k for k, (res, _a) in _lib.SIGNATURES.items() if res is _lib._i and k not in ("t2h_abi_version", "t2h_pool_winner_stride", "t2h_adamw_chunk_elems", "t2h_conv3x3_bx3_supported", "t2h_gemm_bx3_supported", "t2h_gemm_bx3_wgrad_supported", "t2h_conv3x3_bx3_dgrad_rank1_supported", "t2h_upconv2x2_bx3_supported",
                                                                                    "t2h_reduce_capture_begin", "t2h_reduce_capture_pending", "t2h_reduce_capture_end",
                                                                                    "t2h_debug_poison_lds")]          # (test instrumentation: no arguments to reject)
    assert sorted(cases) == sorted(launching), set(launching) ^ set(cases)
    for name, args in cases.items():
        rc = getattr(lib, name)(*args)
        assert rc in (-1, -3), f"{name} returned {rc}"
        assert len(lib.t2h_last_error_string()) > 8


def test_in_place_gradient_joins_only_into_solely_owned_buffers():
    """mlp._join_plane_grad / deferred._DeferredLevel accumulate into the gradient tensor autograd hands them only
    when nobody else still reads it (mlp.sole_owner).  torch's add backward hands the SAME tensor to both producers: the node
    that runs first must not write into it."""
    import torch
    from tomosar2height_amd import mlp
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            seen.append(mlp.sole_owner(g))
            return g * 2

    class ChannelsLastGrad(torch.autograd.Function):        # returns a permuted view of a fresh NHWC buffer, as grid.py does
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, g):
            d = torch.empty(1, 3, 3, 4)
            d.copy_(g.permute(0, 2, 3, 1))
            return d.permute(0, 3, 1, 2)

    x = torch.randn(1, 4, 3, 3, requires_grad=True)
    (Probe.apply(x) * 3).sum().backward()
    assert seen == [True]
    seen.clear()
    z = Probe.apply(x) + Probe.apply(x * 1.5)              # one gradient buffer queued for two nodes
    (z * z).sum().backward()
    assert seen == [False, True]
    seen.clear()
    ChannelsLastGrad.apply(Probe.apply(x)).sum().backward()
    assert seen == [True]


# ---- the point-grid entry points (csrc/point_grid.hip): which code and message every refused call returns ------------------------
# Host memory only: every row below returns before a launch (a refusal, or T2H_OK for a call with no rows to work on).  A call is
# the entry point's `base` arguments with the positions in `change` replaced.  Codes and messages are those of the library as it
# stood before its host section was folded: a row with two faults pins WHICH check answers first.  A message ending in "..." is
# matched as a prefix, any other in full.
def _point_grid_rows():
    import ctypes
    import numpy as np
    buf = np.zeros(4096, np.float32)
    P = buf.ctypes.data + (-buf.ctypes.data % 16)      # 16-byte aligned
    Q, P2, n = P + 4, P + 4096, None                   # Q: float-aligned only
    keep = [buf]

    def ptrs(*v):
        keep.append((ctypes.c_void_p * len(v))(*v))
        return keep[-1]

    def ints(*v):
        keep.append((ctypes.c_int * len(v))(*v))
        return keep[-1]

    ARG, WS, OK = -1, -3, 0
    shape = lambda what, B, nbits, level, C: f"{what}: unsupported shape (B={B} nbits={nbits} level={level} C={C})"
    rows = []

    def entry(name, base, *cases):
        rows.extend((name, base, *c) for c in cases)

    for what in ("pool_max_fwd", "pool_max_bwd", "pool_mean"):
        # (in, ld_in, B, nbits, C, out, ld_out): the positions of the three signatures
        base, i, li, b, nb, c, o, lo = {
            "pool_max_fwd": ((P, 32, P, 1, 4, 32, P2, 32, P, n), 0, 1, 3, 4, 5, 6, 7),
            "pool_max_bwd": ((P, 32, P, P, 1, 4, 32, 0, P2, 32, n), 0, 1, 4, 5, 6, 8, 9),
            "pool_mean": ((P, 32, P, 1, 4, 32, 0, P2, 32, n), 0, 1, 3, 4, 5, 7, 8)}[what]
        entry("t2h_" + what, base,
              ({i: n}, ARG, what + ": null pointer"), ({o: n}, ARG, what + ": null pointer"), ({2: n}, ARG, what + ": null pointer"),
              ({i: n, nb: 0}, ARG, what + ": null pointer"),
              ({nb: 0}, ARG, shape(what, 1, 0, 0, 32)), ({nb: 11}, ARG, shape(what, 1, 11, 0, 32)),
              ({b: 0}, ARG, shape(what, 0, 4, 0, 32)), ({c: 0}, ARG, shape(what, 1, 4, 0, 0)),
              ({nb: 11, li: 16}, ARG, shape(what, 1, 11, 0, 32)),
              ({li: 16}, ARG, what + ": row stride smaller than C"), ({lo: 31}, ARG, what + ": row stride smaller than C"),
              ({li: 16, i: Q}, ARG, what + ": row stride smaller than C"),
              ({li: 34}, ARG, what + ": rows must be 16-byte aligned when C % 4 == 0"),
              ({lo: 34}, ARG, what + ": rows must be 16-byte aligned when C % 4 == 0"),
              ({i: Q}, ARG, what + ": rows must be 16-byte aligned when C % 4 == 0"),
              ({o: Q}, ARG, what + ": rows must be 16-byte aligned when C % 4 == 0"))
    entry("t2h_pool_mean", (P, 32, P, 1, 4, 32, 0, P2, 32, n),
          ({7: P}, ARG, "pool_mean: in-place call (a cell's rows are re-read while they are written)"),
          ({7: P, 4: 0}, ARG, "pool_mean: in-place call..."))
    for what, base, nr, c, i, li, o, lo in (("pool_rows_fwd", (P, 32, P, P, 100, 32, P2, 32, P, n), 4, 5, 0, 1, 6, 7),
                                           ("pool_rows_bwd", (P, 32, P, P, P, 100, 32, 0, P2, 32, n), 5, 6, 0, 1, 8, 9)):
        needs = what + ": needs C in {4, 8, .., 64} and 16-byte aligned rows"
        entry("t2h_" + what, base,
              ({i: n}, ARG, what + ": null pointer"), ({3: n}, ARG, what + ": null pointer"), ({i: n, nr: 0}, ARG, what + ": null pointer"),
              ({nr: -1}, ARG, needs), ({nr: (1 << 30) + 1}, ARG, needs), ({c: 68}, ARG, needs), ({c: 6}, ARG, needs), ({c: 0}, ARG, needs),
              ({li: 16}, ARG, needs), ({lo: 16}, ARG, needs), ({li: 34}, ARG, needs), ({lo: 34}, ARG, needs), ({i: Q}, ARG, needs),
              ({o: Q}, ARG, needs), ({nr: 0, c: 68}, ARG, needs), ({nr: 0}, OK, None))
    entry("t2h_segmean_fwd", (P, P, 1, 4096, 4, 2, 64, P2, n, 0, n),
          ({0: n}, ARG, "segmean_fwd: null pointer"), ({7: n}, ARG, "segmean_fwd: null pointer"),
          ({5: 5}, ARG, shape("segmean_fwd", 1, 4, 5, 64)), ({5: -1}, ARG, shape("segmean_fwd", 1, 4, -1, 64)),
          ({4: 11}, ARG, shape("segmean_fwd", 1, 11, 2, 64)), ({2: 0}, ARG, shape("segmean_fwd", 0, 4, 2, 64)),
          ({6: 0}, ARG, shape("segmean_fwd", 1, 4, 2, 0)),
          ({}, WS, "segmean_fwd: workspace 0 < 32768 bytes"), ({9: 1 << 20}, WS, "segmean_fwd: workspace 1048576 < 32768 bytes"),
          ({8: P, 9: 32767}, WS, "segmean_fwd: workspace 32767 < 32768 bytes"),
          ({6: 68, 8: P, 9: 34815}, WS, "segmean_fwd: workspace 34815 < 34816 bytes"))
    entry("t2h_segsum_fwd", (P, P, 1, 4096, 4, 2, 64, P2, 64, n, 0, n, n),
          ({1: n}, ARG, "segmean_fwd: null pointer"), ({1: n, 8: 32}, ARG, "segmean_fwd: null pointer"),
          ({8: 32}, ARG, "segmean_fwd: plane row stride 32 < C = 64"), ({8: 66}, ARG, "segmean_fwd: plane row stride 66 < C = 64"),
          ({8: 32, 5: 5}, ARG, "segmean_fwd: plane row stride 32 < C = 64"), ({5: 5}, ARG, shape("segmean_fwd", 1, 4, 5, 64)),
          ({5: 5, 9: P, 10: 100}, ARG, shape("segmean_fwd", 1, 4, 5, 64)),
          ({}, WS, "segmean_fwd: workspace 0 < 32768 bytes"), ({8: 128, 9: P, 10: 100}, WS, "segmean_fwd: workspace 100 < 32768 bytes"))
    needs = "plane_sumpool2x2: needs an even resolution, C % 4 == 0, row strides >= C and 16-byte aligned rows"
    entry("t2h_plane_sumpool2x2", (P, 32, 1, 8, 32, P2, 32, n, n),
          ({0: n}, ARG, "plane_sumpool2x2: null pointer"), ({5: n, 3: 7}, ARG, "plane_sumpool2x2: null pointer"),
          ({3: 7}, ARG, needs), ({3: 0}, ARG, needs), ({4: 6}, ARG, needs), ({4: 0}, ARG, needs), ({0: Q}, ARG, needs),
          ({5: Q}, ARG, needs), ({1: 16}, ARG, needs), ({6: 34}, ARG, needs), ({2: 0}, ARG, needs))
    GP, LV, LD = ptrs(P, P), ints(0, 2), ints(32, 32)
    entry("t2h_segsum_bwd_multi", (GP, LV, LD, 2, P, 1, 100, 4, 32, n, n, P2, n, n, -1),
          ({0: n}, ARG, "segsum_bwd_multi: null pointer"), ({11: n, 3: 0}, ARG, "segsum_bwd_multi: null pointer"),
          ({3: 0}, ARG, "segsum_bwd_multi: 1..8 planes, got 0"), ({3: 9, 7: 11}, ARG, "segsum_bwd_multi: 1..8 planes, got 9"),
          ({7: 11}, ARG, "segsum_bwd_multi: unsupported shape"), ({5: 0}, ARG, "segsum_bwd_multi: unsupported shape"),
          ({8: 0, 0: ptrs(P, n)}, ARG, "segsum_bwd_multi: unsupported shape"),
          ({0: ptrs(P, n)}, ARG, "segsum_bwd_multi: bad plane 1"), ({1: ints(0, 5)}, ARG, "segsum_bwd_multi: bad plane 1"),
          ({1: ints(-1, 5)}, ARG, "segsum_bwd_multi: bad plane 0"),
          ({0: ptrs(Q, P)}, ARG, "segsum_bwd_multi: planes must be 16-byte aligned"),
          ({2: ints(32, 34)}, ARG, "segsum_bwd_multi: planes must be 16-byte aligned"),
          ({2: ints(18, 32)}, ARG, "segsum_bwd_multi: planes must be 16-byte aligned"),
          ({2: ints(16, 32)}, ARG, "segsum_bwd_multi: plane 0 row stride 16 < C"),
          ({2: ints(32, 16)}, ARG, "segsum_bwd_multi: plane 1 row stride 16 < C"),
          ({2: ints(16, 32), 0: ptrs(P, n)}, ARG, "segsum_bwd_multi: plane 0 row stride 16 < C"),
          ({8: 6, 0: ptrs(Q, Q), 2: ints(6, 4)}, ARG, "segsum_bwd_multi: plane 1 row stride 4 < C"),
          ({9: Q}, ARG, "segsum_bwd_multi: rows must be 16-byte aligned"), ({10: Q}, ARG, "segsum_bwd_multi: rows must be 16-byte aligned"),
          ({11: Q}, ARG, "segsum_bwd_multi: rows must be 16-byte aligned"), ({9: Q, 0: ptrs(P, n)}, ARG, "segsum_bwd_multi: bad plane 1"),
          ({13: P, 14: 1}, ARG, "segsum_bwd_multi: compact rows of level 1, which no plane has"),
          ({13: P, 14: 1, 11: Q}, ARG, "segsum_bwd_multi: rows must be 16-byte aligned"),
          ({13: P, 14: -1, 6: 0}, ARG, "segsum_bwd_multi: compact rows of level -1, which no plane has"),
          ({6: 0}, OK, None), ({6: 0, 13: P, 14: 2}, OK, None), ({6: 0, 8: 6, 0: ptrs(Q, Q), 11: Q}, OK, None))
    entry("t2h_segmean_bwd", (P, P, P, 1, 100, 4, 2, 32, P2, n),
          ({0: n}, ARG, "segmean_bwd: null pointer"), ({8: n, 6: 5}, ARG, "segmean_bwd: null pointer"),
          ({6: 5}, ARG, shape("segmean_bwd", 1, 4, 5, 32)), ({4: 0}, OK, None), ({4: 0, 5: 0}, ARG, shape("segmean_bwd", 1, 0, 2, 32)))
    entry("t2h_segmean_bwd_add", (P, P, P, 1, 100, 4, 2, 32, n, P2, n),
          ({1: n}, ARG, "segmean_bwd: null pointer"), ({8: Q}, ARG, "segmean_bwd: addend must be 16-byte aligned"),
          ({8: Q, 6: 5}, ARG, "segmean_bwd: addend must be 16-byte aligned"), ({8: Q, 2: n}, ARG, "segmean_bwd: null pointer"),
          ({6: 5}, ARG, shape("segmean_bwd", 1, 4, 5, 32)), ({5: 0}, ARG, shape("segmean_bwd", 1, 0, 2, 32)),
          ({7: 0}, ARG, shape("segmean_bwd", 1, 4, 2, 0)), ({4: 0}, OK, None), ({4: 0, 8: P}, OK, None), ({4: 0, 7: 6, 8: Q}, OK, None))
    entry("t2h_sample_fwd", (P, P, 3, 1, 100, 16, 32, P2, n),
          ({0: n}, ARG, "sample_fwd: null pointer"), ({7: n, 2: 1}, ARG, "sample_fwd: null pointer"),
          ({2: 1}, ARG, "sample_fwd: unsupported shape"), ({3: 0}, ARG, "sample_fwd: unsupported shape"),
          ({5: 0}, ARG, "sample_fwd: unsupported shape"), ({6: 0}, ARG, "sample_fwd: unsupported shape"),
          ({4: -5, 2: 2}, ARG, "sample_fwd: unsupported shape"), ({4: 0, 5: 0}, ARG, "sample_fwd: unsupported shape"), ({4: 0}, OK, None))
    needs = "cell_order_build: needs 0 <= level_lo <= level_hi < nbits"
    entry("t2h_cell_order_build", (P, 1, 4, 2, P2, n),
          ({0: n}, ARG, "cell_order_build: null pointer"), ({4: n, 3: 4}, ARG, "cell_order_build: null pointer"),
          ({3: 4}, ARG, needs), ({3: -1}, ARG, needs), ({2: 11}, ARG, needs), ({1: 0}, ARG, needs))
    entry("t2h_cell_order_build_range", (P, 1, 4, 1, 3, P2, n),
          ({5: n}, ARG, "cell_order_build: null pointer"), ({0: n, 3: 3, 4: 1}, ARG, "cell_order_build: null pointer"),
          ({3: 3, 4: 1}, ARG, needs), ({4: 4}, ARG, needs), ({3: -1}, ARG, needs), ({2: 0}, ARG, needs))
    what = "sample_relu_cellsums"
    needs = what + ": needs C % 256 == 0, sum_level <= level, 16-byte aligned rows"
    pooled = what + ": the pooled sums need sum_level < level and 16-byte aligned rows of >= C floats"
    for name, base in (("t2h_sample_relu_cellsums", (P, P, 3, P, 1, 4096, 4, 2, 0, 256, P2, 256, P, n)),
                       ("t2h_sample_relu_cellsums2", (P, P, 3, P, 1, 4096, 4, 2, 0, 256, P2, 256, n, 0, P, n)),
                       ("t2h_sample_relu_cellsums_ordered", (P, P, 3, P, 1, 4096, 4, 2, 0, 256, P2, 256, n, 0, P, n, n, n))):
        sign = 12 if len(base) == 14 else 14
        entry(name, base,
              ({0: n}, ARG, what + ": null pointer"), ({10: n, 7: 5}, ARG, what + ": null pointer"),
              ({7: 5}, ARG, shape(what, 1, 4, 5, 256)), ({7: 5, 9: 64}, ARG, shape(what, 1, 4, 5, 64)), ({6: 11}, ARG, shape(what, 1, 11, 2, 256)),
              ({2: 1}, ARG, needs), ({8: 3}, ARG, needs), ({8: -1}, ARG, needs), ({9: 64}, ARG, needs), ({11: 128}, ARG, needs),
              ({11: 258}, ARG, needs), ({0: Q}, ARG, needs), ({10: Q}, ARG, needs), ({sign: Q}, ARG, needs),
              ({7: 4, 9: 64}, ARG, needs), ({5: 0, 9: 64}, ARG, needs),
              ({5: 0}, ARG, what + ": empty tile"), ({5: 0, 7: 4}, ARG, what + ": empty tile"),
              ({7: 4}, ARG, what + ": needs level < nbits (a 1 x 1 plane: use t2h_sample_fwd_relu + t2h_segsum_fwd)"),
              ({7: 4, 8: 4}, ARG, what + ": needs level < nbits..."))
        if sign == 14:
            entry(name, base,
                  ({12: P, 13: 256, 8: 2}, ARG, pooled), ({12: P, 13: 128}, ARG, pooled), ({12: P, 13: 258}, ARG, pooled),
                  ({12: Q, 13: 256}, ARG, pooled), ({12: P, 13: 128, 7: 5}, ARG, pooled), ({12: P, 13: 128, 0: n}, ARG, what + ": null pointer"),
                  ({12: P, 13: 256, 7: 4}, ARG, what + ": needs level < nbits..."))
    what = "sample_bwd_from_sums"
    few = what + ": level 0 holds too few points per cell for the per-cell partials (t2h_sample_bwd_workspace_bytes == 0): use t2h_segsum_bwd_multi + t2h_sample_bwd"
    LD = ints(256, 256)
    big = 1 << 40
    for name, base in (("t2h_sample_bwd_from_sums", (GP, LV, LD, 2, P, P, 0, P, 3, P, 1, 4096, 4, 2, 256, P2, n, 0, n)),
                       ("t2h_sample_bwd_from_sums_ordered", (GP, LV, LD, 2, P, P, 0, P, 3, P, 1, 4096, 4, 2, 256, P2, n, 0, n, n, n, -1))):
        entry(name, base,
              ({5: n}, ARG, what + ": null pointer"), ({0: n, 3: 9}, ARG, what + ": null pointer"),
              ({3: 0}, ARG, what + ": 1..8 planes, got 0"), ({3: 9, 13: 5}, ARG, what + ": 1..8 planes, got 9"),
              ({13: 5}, ARG, shape(what, 1, 4, 5, 256)), ({13: 5, 8: 1}, ARG, shape(what, 1, 4, 5, 256)),
              ({13: 5, 6: 1, 14: 64}, ARG, shape(what, 1, 4, 5, 64)),
              ({8: 1}, ARG, what + ": unsupported shape"), ({14: 6}, ARG, what + ": unsupported shape"), ({5: Q}, ARG, what + ": unsupported shape"),
              ({5: Q, 6: 1, 14: 64}, ARG, what + ": unsupported shape"),
              ({6: 1, 14: 64}, ARG, what + ": packed sign bits need C % 256 == 0 (and the matrix-core partials)"),
              ({6: 1, 14: 64, 11: 100, 13: 0}, ARG, what + ": packed sign bits need C % 256 == 0..."),
              ({11: 100, 13: 0}, ARG, few), ({11: 0}, ARG, what + ": level 2 holds too few points per cell..."),
              ({11: 100, 13: 0, 0: ptrs(P, n)}, ARG, few),
              ({}, WS, what + ": workspace 0 < 1179648 bytes"), ({17: big}, WS, what + f": workspace {big} < 1179648 bytes"),
              ({16: P, 17: 1179647}, WS, what + ": workspace 1179647 < 1179648 bytes"),
              ({16: P, 17: 100, 0: ptrs(P, n)}, WS, what + ": workspace 100 < 1179648 bytes"),
              ({14: 68, 2: ints(68, 68), 16: P, 17: 100}, WS, what + ": workspace 100 < 313344 bytes"),
              ({16: P, 17: big, 0: ptrs(P, n)}, ARG, what + ": bad plane 1"), ({16: P, 17: big, 0: ptrs(Q, n)}, ARG, what + ": bad plane 0"),
              ({16: P, 17: big, 1: ints(0, 5)}, ARG, what + ": bad plane 1"), ({16: P, 17: big, 1: ints(-1, 2)}, ARG, what + ": bad plane 0"),
              ({16: P, 17: big, 2: ints(256, 128)}, ARG, what + ": bad plane 1"), ({16: P, 17: big, 2: ints(258, 256)}, ARG, what + ": bad plane 0"))
    entry("t2h_sample_bwd_from_sums_ordered", base,
          ({16: P, 17: big, 20: P, 21: 1}, ARG, what + ": compact rows of level 1, which no plane has"),
          ({16: P, 17: big, 20: P, 21: -1}, ARG, what + ": compact rows of level -1, which no plane has"),
          ({16: P, 17: big, 20: P, 21: 1, 1: ints(0, 5)}, ARG, what + ": bad plane 1"),
          ({17: 100, 20: P, 21: 1}, WS, what + ": workspace 100 < 1179648 bytes"))
    bits = "sample_fwd_relu: the packed sign bits need C % 256 == 0 and a 16-byte aligned buffer"
    entry("t2h_sample_fwd_relu", (P, P, 3, 1, 100, 16, 256, P2, P, n),
          ({1: n}, ARG, "sample_fwd_relu: null pointer"), ({7: n, 2: 1}, ARG, "sample_fwd_relu: null pointer"),
          ({2: 1}, ARG, "sample_fwd_relu: unsupported shape"), ({4: -5, 2: 2}, ARG, "sample_fwd_relu: unsupported shape"),
          ({5: 0, 6: 64}, ARG, "sample_fwd_relu: unsupported shape"), ({6: 64}, ARG, bits), ({6: 6}, ARG, bits), ({8: Q}, ARG, bits),
          ({4: 0, 8: Q}, ARG, bits), ({4: 0}, OK, None), ({4: 0, 6: 6, 8: n}, OK, None))
    for name, base, shift in (("t2h_sample_bwd", (P, P, 3, P, 1, 4096, 4, 2, 64, P2, n, 0, n), 0),
                              ("t2h_sample_bwd_add", (P, P, 3, P, 1, 4096, 4, 2, 64, n, P2, n, 0, n), 1)):
        ws, wsb = 10 + shift, 11 + shift
        entry(name, base,
              ({0: n}, ARG, "sample_bwd: null pointer"), ({3: n, 7: 5}, ARG, "sample_bwd: null pointer"),
              ({7: 5}, ARG, shape("sample_bwd", 1, 4, 5, 64)), ({7: 5, 2: 1}, ARG, shape("sample_bwd", 1, 4, 5, 64)),
              ({4: 0}, ARG, shape("sample_bwd", 0, 4, 2, 64)), ({2: 1}, ARG, "sample_bwd: unsupported shape"),
              ({2: 1, ws: P, wsb: 100}, ARG, "sample_bwd: unsupported shape"),
              ({}, WS, "sample_bwd: workspace 0 < 294912 bytes"), ({wsb: big}, WS, f"sample_bwd: workspace {big} < 294912 bytes"),
              ({ws: P, wsb: 294911}, WS, "sample_bwd: workspace 294911 < 294912 bytes"),
              ({8: 68, ws: P, wsb: 0}, WS, "sample_bwd: workspace 0 < 313344 bytes"),
              ({5: -771, 6: 4, 7: 1, 8: 20, ws: P, wsb: 1}, WS, "sample_bwd: workspace 1 < 368640 bytes"))
    entry("t2h_sample_bwd_add", base,
          ({9: Q}, ARG, "sample_bwd: addend must be 16-byte aligned"), ({9: Q, 7: 5}, ARG, "sample_bwd: addend must be 16-byte aligned"),
          ({9: Q, 8: 6}, ARG, "sample_bwd: addend must be 16-byte aligned"), ({9: Q, 10: n}, ARG, "sample_bwd: null pointer"),
          ({9: P}, WS, "sample_bwd: workspace 0 < 294912 bytes"))
    what = "sample_adjoint_build"
    entry("t2h_sample_adjoint_build", (P, 3, P, 1, 100, 4, 2, P2, P, n),
          ({0: n}, ARG, what + ": null pointer"), ({8: n, 6: 5}, ARG, what + ": null pointer"),
          ({6: 5}, ARG, shape(what, 1, 4, 5, 1)), ({6: 5, 1: 1}, ARG, shape(what, 1, 4, 5, 1)), ({5: 11}, ARG, shape(what, 1, 11, 2, 1)),
          ({1: 1}, ARG, what + ": unsupported shape"), ({4: (1 << 28) + 1}, ARG, what + ": unsupported shape"),
          ({4: -(1 << 28) - 1}, ARG, what + ": unsupported shape"), ({1: 1, 8: Q}, ARG, what + ": unsupported shape"),
          ({8: Q}, ARG, what + ": entries must be 8-byte aligned"))
    what = "sample_bwd_adjoint"
    entry("t2h_sample_bwd_adjoint", (P, P, P, 1, 4, 2, 32, n, P2, n),
          ({0: n}, ARG, what + ": null pointer"), ({2: n, 7: Q}, ARG, what + ": null pointer"),
          ({7: Q}, ARG, what + ": addend must be 16-byte aligned"), ({7: Q, 5: 5}, ARG, what + ": addend must be 16-byte aligned"),
          ({7: Q, 6: 6}, ARG, what + ": addend must be 16-byte aligned"),
          ({5: 5}, ARG, shape(what, 1, 4, 5, 32)), ({5: -1}, ARG, shape(what, 1, 4, -1, 32)), ({6: 0}, ARG, shape(what, 1, 4, 2, 0)))
    what = "sample_bwd_atomic: unsupported shape (equal-N batches only)"
    entry("t2h_sample_bwd_atomic", (P, P, 3, 1, 100, 16, 32, P2, n),
          ({0: n}, ARG, "sample_bwd_atomic: null pointer"), ({7: n, 4: -5}, ARG, "sample_bwd_atomic: null pointer"),
          ({4: -5}, ARG, what), ({2: 1}, ARG, what), ({5: 0}, ARG, what), ({6: 0}, ARG, what), ({3: 0}, ARG, what),
          ({4: 0, 5: 0}, ARG, what), ({4: 0}, OK, None))
    return rows, keep


_SIZE_FUNCTIONS = ("t2h_segmean_workspace_bytes", "t2h_sample_bwd_workspace_bytes", "t2h_pool_winner_stride", "t2h_cell_order_len",
                   "t2h_sample_adjoint_offsets_len")


def test_point_grid_refusals_keep_their_code_message_and_order():
    from tomosar2height_amd import _lib
    lib = _lib.load()
    rows, _keep = _point_grid_rows()
    src = open(os.path.join(ROOT, "tomosar2height_amd", "csrc", "point_grid.hip")).read()
    defined = set(re.findall(r"^T2H_API \w+ (t2h_\w+)\(", src, flags=re.M))
    assert len(defined) == 30 and defined <= set(_lib.SIGNATURES)
    assert {r[0] for r in rows} == defined - set(_SIZE_FUNCTIONS)
    seen = set()
    for name, base, change, rc, message in rows:
        args = tuple(change.get(k, v) for k, v in enumerate(base))
        key = (name, tuple(map(id, args)))
        assert max(change, default=0) < len(base) and key not in seen, (name, change)
        seen.add(key)
        lib.t2h_sample_fwd(None, None, 3, 1, 1, 1, 1, None, None)          # a known message: a row must replace it, or return T2H_OK
        got = getattr(lib, name)(*args)
        text = lib.t2h_last_error_string().decode()
        assert got == rc, f"{name} {change}: returned {got} ({text}), expected {rc}"
        if rc == 0:
            assert text == "sample_fwd: null pointer", f"{name} {change}: T2H_OK, but wrote {text!r}"
        elif message.endswith("..."):
            assert text.startswith(message[:-3]), f"{name} {change}: {text!r}"
        else:
            assert text == message, f"{name} {change}: {text!r}"


# (B, N, nbits, level) -> (t2h_segmean_workspace_bytes, t2h_sample_bwd_workspace_bytes) at C = 3, 20, 64, 68, 256, 512: recorded
# from the library before its host section was folded; every point of the grid that is not listed gives 0 for all twelve.
# N = 257 / 4096 / -771 (ragged: 771 rows in all) cross coarse_plan's thresholds (16 and 6 points per cell) at nbits - level = 2
# and 3, and (3, 4096, 4, 0) at C = 512 its clamp of S to the workgroup target.
_SIZE_CS = (3, 20, 64, 68, 256, 512)
_ONE_CELL = ((0, 640, 2048, 2176, 8192, 16384), (0, 5760, 18432, 19584, 73728, 147456))
_ONE_CELL_3 = ((0, 1920, 6144, 6528, 24576, 49152), (0, 17280, 55296, 58752, 221184, 442368))
_R2 = ((0, 2560, 8192, 8704, 32768, 65536), (0, 23040, 73728, 78336, 294912, 589824))
_R2_3 = ((0, 7680, 24576, 26112, 98304, 196608), (0, 69120, 221184, 235008, 884736, 1769472))
_R4 = ((0, 10240, 32768, 34816, 131072, 262144), (0, 92160, 294912, 313344, 1179648, 2359296))
_R4_3 = ((0, 30720, 98304, 104448, 393216, 786432), (0, 276480, 884736, 940032, 3538944, 7077888))
_WORKSPACE_BYTES = {
    **{(1, N, 2, 0): _R4 for N in (257, 4096, -771)}, **{(1, N, 2, 1): _R2 for N in (257, 4096, -771)},
    **{(1, N, nbits, nbits): _ONE_CELL for N in (257, 4096, -771) for nbits in (2, 4, 8)},
    **{(3, N, 2, 0): _R4_3 for N in (257, 4096, -771)}, **{(3, N, 2, 1): _R2_3 for N in (257, 4096, -771)},
    **{(3, N, nbits, nbits): _ONE_CELL_3 for N in (257, 4096, -771) for nbits in (2, 4, 8)},
    (1, 4096, 4, 0): ((0, 163840, 524288, 557056, 2097152, 4194304), (0, 1474560, 4718592, 5013504, 18874368, 37748736)),
    (1, 4096, 4, 1): ((0, 40960, 131072, 139264, 524288, 1048576), (0, 368640, 1179648, 1253376, 4718592, 9437184)),
    (1, -771, 4, 1): ((0, 0, 0, 0, 0, 0), (0, 368640, 1179648, 1253376, 4718592, 9437184)),
    (3, 4096, 4, 0): ((0, 368640, 1179648, 1253376, 4718592, 4718592), (0, 3317760, 10616832, 11280384, 42467328, 42467328)),
    (3, 4096, 4, 1): ((0, 122880, 393216, 417792, 1572864, 3145728), (0, 1105920, 3538944, 3760128, 14155776, 28311552)),
}
# (B, nbits, level) -> (t2h_cell_order_len, t2h_sample_adjoint_offsets_len)
_LIST_LENGTHS = {
    (1, 2, 0): (20, 19), (1, 2, 1): (5, 7), (1, 2, 2): (0, 4), (1, 4, 0): (320, 274), (1, 4, 1): (80, 70), (1, 4, 4): (0, 4),
    (1, 8, 0): (81920, 69634), (1, 8, 1): (20480, 17410), (1, 8, 8): (0, 4),
    (3, 2, 0): (60, 53), (3, 2, 1): (15, 15), (3, 2, 2): (0, 6), (3, 4, 0): (960, 818), (3, 4, 1): (240, 206), (3, 4, 4): (0, 6),
    (3, 8, 0): (245760, 208898), (3, 8, 1): (61440, 52226), (3, 8, 8): (0, 6),
}


def test_point_grid_size_functions_keep_their_values():
    from tomosar2height_amd import _lib
    lib = _lib.load()
    assert len(_WORKSPACE_BYTES) == 35
    nothing = ((0,) * 6, (0,) * 6)
    for B in (1, 3):
        for nbits in (2, 4, 8):
            for level in (0, 1, nbits):
                for N in (0, 257, 4096, -771):
                    want = _WORKSPACE_BYTES.get((B, N, nbits, level), nothing)
                    got = tuple(tuple(getattr(lib, f)(B, N, nbits, level, C) for C in _SIZE_CS) for f in _SIZE_FUNCTIONS[:2])
                    assert got == want, (B, N, nbits, level, got)
                got = (lib.t2h_cell_order_len(B, nbits, level), lib.t2h_sample_adjoint_offsets_len(B, nbits, level))
                assert got == _LIST_LENGTHS[B, nbits, level], (B, nbits, level, got)
    assert [lib.t2h_pool_winner_stride(C) for C in _SIZE_CS] == [3, 5, 16, 17, 64, 128]
    # out of range: no size.  (10 is T2H_MAX_NBITS; the adjoint's lists do not depend on C)
    for B, N, nbits, level, C in ((0, 4096, 4, 0, 64), (-1, 4096, 4, 0, 64), (1, 4096, 0, 0, 64), (1, 4096, 11, 0, 64), (1, 4096, 4, -1, 64),
                                  (1, 4096, 4, 5, 64), (1, 4096, 4, 4, 0), (1, 4096, 4, 4, -4)):
        assert lib.t2h_segmean_workspace_bytes(B, N, nbits, level, C) == 0 and lib.t2h_sample_bwd_workspace_bytes(B, N, nbits, level, C) == 0
        if C > 0:
            assert lib.t2h_cell_order_len(B, nbits, level) == 0 and lib.t2h_sample_adjoint_offsets_len(B, nbits, level) == 0
    # the finest plane (r = 1024): 16 points per cell exactly, and one point fewer; sizes beyond 2^31
    assert [lib.t2h_segmean_workspace_bytes(1, N, 10, 0, 64) for N in (1 << 20, (1 << 24) - 1, 1 << 24)] == [0, 0, 268435456]
    assert [lib.t2h_sample_bwd_workspace_bytes(1, N, 10, 0, 64) for N in (1 << 20, (1 << 24) - 1, 1 << 24)] == [0, 2415919104, 2415919104]
    assert lib.t2h_cell_order_len(1, 10, 9) == 5 and lib.t2h_cell_order_len(1, 10, 10) == 0 and lib.t2h_sample_adjoint_offsets_len(1, 10, 10) == 4
