"""GPU: the entry-point calls of the hourglass modules per mode -- the forward under ``torch.no_grad()``, the graph forward and the
backward -- against tables recorded from the modules as they were before ``encoder/hourglass.py`` got one forward body per module
(``EXPECTED``: literals, recorded with ``tables`` below on that commit; a change of the body must leave them as they are; the
graph forward's table was equal to the ``no_grad`` one in every case there, so ``forward`` stands for both).

Shapes: the smallest that take every branch of a body -- a ConvBlock with and without the 1 x 1 residual (two affine pairs on one
statistics pass; the pass-through alias), an HourGlass of depth 2 down to one pixel (``b2_plus_1``, the upsample's addend), an
HGFilter of two stacks (the ``bl`` / ``al`` addend pair) for both kinds of ``hg_down`` with the stem in the graph and with the stem
frozen, and the folded BatchNorm block, which has no graph.  Names are the timeline's (``r[0]``); the ``t2h_linear_*`` tags lose
their bracketed shape.  Counts only: no tolerance.
"""
import collections

import pytest
import torch

import hg_ref
from test_hourglass_grad_gpu import precision

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("block64_128", "block128_128", "hourglass128", "block64_128_batch", "filter_ave_pool_stem", "filter_ave_pool_frozen",
         "filter_conv128_stem", "filter_conv128_frozen")
FROZEN_STEM = {"ave_pool": ("conv1",), "conv128": ("conv1", "bn1", "conv2", "down_conv2")}      # the layers the refusal names


def counted(fn):
    """({entry point: calls}, fn()) over one call of ``fn``."""
    from tomosar2height_amd import _lib
    with _lib.KernelTimeline() as tl:
        out = fn()
    torch.cuda.synchronize()
    names = [r[0].split("[")[0] if r[0].startswith("t2h_linear_") else r[0] for r in tl.records]
    return dict(sorted(collections.Counter(names).items())), out


def tables(module, shape, graph=True, input_grad=True):
    """{"no_grad": ..., "graph": ..., "backward": ...} of ``module`` on a ``shape`` input; the weights are warmed by one call first."""
    module = hg_ref.init_hg_(module).to(DEV)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    with precision("fp32"):
        with torch.no_grad():
            module(x)
            out = {"no_grad": counted(lambda: module(x))[0]}
        if graph:
            x.requires_grad_(input_grad)
            out["graph"], y = counted(lambda: module(x))
            out["backward"], _ = counted(lambda: y.backward(torch.ones_like(y)))
    return out


def filter_case(hg_down, stem_gradients):
    from tomosar2height_amd.encoder.hourglass import HGFilter
    net = HGFilter(3, 32, num_hourglass=1, num_stack=2, hg_down=hg_down, trainable=True, stem_gradients=stem_gradients)
    if not stem_gradients:
        for name in FROZEN_STEM[hg_down]:
            getattr(net, name).requires_grad_(False)
    return tables(net, (2, 3, 16, 16), input_grad=stem_gradients)


def cases():
    from tomosar2height_amd.encoder.hourglass import ConvBlock, HourGlass
    out = {
        "block64_128": lambda: tables(ConvBlock(64, 128, "group", trainable=True), (1, 64, 4, 4)),
        "block128_128": lambda: tables(ConvBlock(128, 128, "group", trainable=True), (1, 128, 2, 2)),
        "hourglass128": lambda: tables(HourGlass(1, 2, 128, "group", trainable=True), (1, 128, 4, 4)),
        "block64_128_batch": lambda: tables(ConvBlock(64, 128, "batch").eval(), (1, 64, 4, 4), graph=False),
    }
    for hg_down in FROZEN_STEM:
        for stem_gradients in (True, False):
            out[f"filter_{hg_down}_{'stem' if stem_gradients else 'frozen'}"] = lambda d=hg_down, s=stem_gradients: filter_case(d, s)
    return out


# recorded on the commit before the single bodies (the parent of the refactor), with ``tables`` as it stands here
_FILTER_AVE_POOL = {"t2h_conv3x3_fwd[128->128,4x4]": 1, "t2h_conv3x3_fwd[128->64,2x2]": 6, "t2h_conv3x3_fwd[128->64,4x4]": 6,
                    "t2h_conv3x3_fwd[256->128,2x2]": 6, "t2h_conv3x3_fwd[256->128,4x4]": 4, "t2h_conv3x3_fwd[32->32,4x4]": 1,
                    "t2h_conv3x3_fwd[32->32,8x8]": 1, "t2h_conv3x3_fwd[64->32,4x4]": 1, "t2h_conv3x3_fwd[64->32,8x8]": 1,
                    "t2h_conv3x3_fwd[64->64,2x2]": 6, "t2h_conv3x3_fwd[64->64,4x4]": 5, "t2h_conv3x3_fwd[64->64,8x8]": 1,
                    "t2h_hg_avgpool2x2": 3, "t2h_hg_block_tail": 13, "t2h_hg_conv_s2_fwd": 1, "t2h_hg_groupnorm_stats": 42,
                    "t2h_hg_norm_apply": 44, "t2h_linear_fwd": 8, "t2h_upsample_bicubic_fwd": 2}
_FILTER_CONV128 = {"t2h_conv3x3_fwd[128->128,4x4]": 1, "t2h_conv3x3_fwd[128->64,2x2]": 6, "t2h_conv3x3_fwd[128->64,4x4]": 6,
                   "t2h_conv3x3_fwd[256->128,2x2]": 6, "t2h_conv3x3_fwd[256->128,4x4]": 4, "t2h_conv3x3_fwd[32->32,4x4]": 1,
                   "t2h_conv3x3_fwd[32->32,8x8]": 1, "t2h_conv3x3_fwd[64->32,4x4]": 1, "t2h_conv3x3_fwd[64->32,8x8]": 1,
                   "t2h_conv3x3_fwd[64->64,2x2]": 6, "t2h_conv3x3_fwd[64->64,4x4]": 5, "t2h_conv3x3_fwd[64->64,8x8]": 1,
                   "t2h_hg_avgpool2x2": 2, "t2h_hg_block_tail": 13, "t2h_hg_conv_s2_fwd": 2, "t2h_hg_groupnorm_stats": 42,
                   "t2h_hg_norm_apply": 44, "t2h_linear_fwd": 8, "t2h_upsample_bicubic_fwd": 2}
EXPECTED = {
    "block64_128": {
        "forward": {"t2h_conv3x3_fwd[32->32,4x4]": 1, "t2h_conv3x3_fwd[64->32,4x4]": 1, "t2h_conv3x3_fwd[64->64,4x4]": 1,
                    "t2h_hg_block_tail": 1, "t2h_hg_groupnorm_stats": 3, "t2h_hg_norm_apply": 4, "t2h_linear_fwd": 1},
        "backward": {"t2h_conv3x3_dgrad[32->32,4x4]": 1, "t2h_conv3x3_dgrad[32->64,4x4]": 1, "t2h_conv3x3_dgrad[64->64,4x4]": 1,
                     "t2h_conv3x3_wgrad[32->32,4x4]": 1, "t2h_conv3x3_wgrad[64->32,4x4]": 1, "t2h_conv3x3_wgrad[64->64,4x4]": 1,
                     "t2h_hg_block_tail_bwd": 1, "t2h_hg_groupnorm_bwd_apply": 4, "t2h_hg_groupnorm_bwd_reduce": 4,
                     "t2h_linear_dgrad": 1, "t2h_linear_wgrad": 1},
    },
    "block128_128": {
        "forward": {"t2h_conv3x3_fwd[128->64,2x2]": 1, "t2h_conv3x3_fwd[32->32,2x2]": 1, "t2h_conv3x3_fwd[64->32,2x2]": 1,
                    "t2h_hg_block_tail": 1, "t2h_hg_groupnorm_stats": 3, "t2h_hg_norm_apply": 3},
        "backward": {"t2h_conv3x3_dgrad[32->32,2x2]": 1, "t2h_conv3x3_dgrad[32->64,2x2]": 1,
                     "t2h_conv3x3_dgrad[64->128,2x2]": 1, "t2h_conv3x3_wgrad[128->64,2x2]": 1,
                     "t2h_conv3x3_wgrad[32->32,2x2]": 1, "t2h_conv3x3_wgrad[64->32,2x2]": 1, "t2h_hg_block_tail_bwd": 1,
                     "t2h_hg_groupnorm_bwd_apply": 3, "t2h_hg_groupnorm_bwd_reduce": 3},
    },
    "hourglass128": {
        "forward": {"t2h_conv3x3_fwd[128->64,1x1]": 3, "t2h_conv3x3_fwd[128->64,2x2]": 3, "t2h_conv3x3_fwd[128->64,4x4]": 1,
                    "t2h_conv3x3_fwd[32->32,1x1]": 3, "t2h_conv3x3_fwd[32->32,2x2]": 3, "t2h_conv3x3_fwd[32->32,4x4]": 1,
                    "t2h_conv3x3_fwd[64->32,1x1]": 3, "t2h_conv3x3_fwd[64->32,2x2]": 3, "t2h_conv3x3_fwd[64->32,4x4]": 1,
                    "t2h_hg_avgpool2x2": 2, "t2h_hg_block_tail": 7, "t2h_hg_groupnorm_stats": 21, "t2h_hg_norm_apply": 21,
                    "t2h_upsample_bicubic_fwd": 2},
        "backward": {"t2h_conv3x3_dgrad[32->32,1x1]": 3, "t2h_conv3x3_dgrad[32->32,2x2]": 3, "t2h_conv3x3_dgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_dgrad[32->64,1x1]": 3, "t2h_conv3x3_dgrad[32->64,2x2]": 3, "t2h_conv3x3_dgrad[32->64,4x4]": 1,
                     "t2h_conv3x3_dgrad[64->128,1x1]": 3, "t2h_conv3x3_dgrad[64->128,2x2]": 3,
                     "t2h_conv3x3_dgrad[64->128,4x4]": 1, "t2h_conv3x3_wgrad[128->64,1x1]": 3,
                     "t2h_conv3x3_wgrad[128->64,2x2]": 3, "t2h_conv3x3_wgrad[128->64,4x4]": 1,
                     "t2h_conv3x3_wgrad[32->32,1x1]": 3, "t2h_conv3x3_wgrad[32->32,2x2]": 3, "t2h_conv3x3_wgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_wgrad[64->32,1x1]": 3, "t2h_conv3x3_wgrad[64->32,2x2]": 3, "t2h_conv3x3_wgrad[64->32,4x4]": 1,
                     "t2h_hg_avgpool2x2_bwd": 2, "t2h_hg_block_tail_bwd": 7, "t2h_hg_groupnorm_bwd_apply": 21,
                     "t2h_hg_groupnorm_bwd_reduce": 21, "t2h_upsample_bicubic_bwd": 2},
    },
    "block64_128_batch": {
        "forward": {"t2h_conv3x3_fwd[32->32,4x4]": 1, "t2h_conv3x3_fwd[64->32,4x4]": 1, "t2h_conv3x3_fwd[64->64,4x4]": 1,
                    "t2h_hg_block_tail": 1, "t2h_hg_norm_apply": 4, "t2h_linear_fwd": 1},
    },
    "filter_ave_pool_stem": {
        "forward": _FILTER_AVE_POOL,
        "backward": {"t2h_conv3x3_dgrad[128->128,4x4]": 1, "t2h_conv3x3_dgrad[128->256,2x2]": 6,
                     "t2h_conv3x3_dgrad[128->256,4x4]": 4, "t2h_conv3x3_dgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_dgrad[32->32,8x8]": 1, "t2h_conv3x3_dgrad[32->64,4x4]": 1, "t2h_conv3x3_dgrad[32->64,8x8]": 1,
                     "t2h_conv3x3_dgrad[64->128,2x2]": 6, "t2h_conv3x3_dgrad[64->128,4x4]": 6,
                     "t2h_conv3x3_dgrad[64->64,2x2]": 6, "t2h_conv3x3_dgrad[64->64,4x4]": 5, "t2h_conv3x3_dgrad[64->64,8x8]": 1,
                     "t2h_conv3x3_wgrad[128->128,4x4]": 1, "t2h_conv3x3_wgrad[128->64,2x2]": 6,
                     "t2h_conv3x3_wgrad[128->64,4x4]": 6, "t2h_conv3x3_wgrad[256->128,2x2]": 6,
                     "t2h_conv3x3_wgrad[256->128,4x4]": 4, "t2h_conv3x3_wgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_wgrad[32->32,8x8]": 1, "t2h_conv3x3_wgrad[64->32,4x4]": 1, "t2h_conv3x3_wgrad[64->32,8x8]": 1,
                     "t2h_conv3x3_wgrad[64->64,2x2]": 6, "t2h_conv3x3_wgrad[64->64,4x4]": 5, "t2h_conv3x3_wgrad[64->64,8x8]": 1,
                     "t2h_hg_avgpool2x2_bwd": 3, "t2h_hg_block_tail_bwd": 13, "t2h_hg_conv_s2_dgrad": 1,
                     "t2h_hg_conv_s2_wgrad": 1, "t2h_hg_groupnorm_bwd_apply": 44, "t2h_hg_groupnorm_bwd_reduce": 44,
                     "t2h_linear_dgrad": 8, "t2h_linear_wgrad": 8, "t2h_upsample_bicubic_bwd": 2},
    },
    "filter_ave_pool_frozen": {
        "forward": _FILTER_AVE_POOL,
        "backward": {"t2h_conv3x3_dgrad[128->128,4x4]": 1, "t2h_conv3x3_dgrad[128->256,2x2]": 6,
                     "t2h_conv3x3_dgrad[128->256,4x4]": 4, "t2h_conv3x3_dgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_dgrad[32->32,8x8]": 1, "t2h_conv3x3_dgrad[32->64,4x4]": 1, "t2h_conv3x3_dgrad[32->64,8x8]": 1,
                     "t2h_conv3x3_dgrad[64->128,2x2]": 6, "t2h_conv3x3_dgrad[64->128,4x4]": 6,
                     "t2h_conv3x3_dgrad[64->64,2x2]": 6, "t2h_conv3x3_dgrad[64->64,4x4]": 5, "t2h_conv3x3_dgrad[64->64,8x8]": 1,
                     "t2h_conv3x3_wgrad[128->128,4x4]": 1, "t2h_conv3x3_wgrad[128->64,2x2]": 6,
                     "t2h_conv3x3_wgrad[128->64,4x4]": 6, "t2h_conv3x3_wgrad[256->128,2x2]": 6,
                     "t2h_conv3x3_wgrad[256->128,4x4]": 4, "t2h_conv3x3_wgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_wgrad[32->32,8x8]": 1, "t2h_conv3x3_wgrad[64->32,4x4]": 1, "t2h_conv3x3_wgrad[64->32,8x8]": 1,
                     "t2h_conv3x3_wgrad[64->64,2x2]": 6, "t2h_conv3x3_wgrad[64->64,4x4]": 5, "t2h_conv3x3_wgrad[64->64,8x8]": 1,
                     "t2h_hg_avgpool2x2_bwd": 3, "t2h_hg_block_tail_bwd": 13, "t2h_hg_groupnorm_bwd_apply": 43,
                     "t2h_hg_groupnorm_bwd_reduce": 44, "t2h_linear_dgrad": 8, "t2h_linear_wgrad": 8,
                     "t2h_upsample_bicubic_bwd": 2},
    },
    "filter_conv128_stem": {
        "forward": _FILTER_CONV128,
        "backward": {"t2h_conv3x3_dgrad[128->128,4x4]": 1, "t2h_conv3x3_dgrad[128->256,2x2]": 6,
                     "t2h_conv3x3_dgrad[128->256,4x4]": 4, "t2h_conv3x3_dgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_dgrad[32->32,8x8]": 1, "t2h_conv3x3_dgrad[32->64,4x4]": 1, "t2h_conv3x3_dgrad[32->64,8x8]": 1,
                     "t2h_conv3x3_dgrad[64->128,2x2]": 6, "t2h_conv3x3_dgrad[64->128,4x4]": 6,
                     "t2h_conv3x3_dgrad[64->64,2x2]": 6, "t2h_conv3x3_dgrad[64->64,4x4]": 5, "t2h_conv3x3_dgrad[64->64,8x8]": 1,
                     "t2h_conv3x3_wgrad[128->128,4x4]": 1, "t2h_conv3x3_wgrad[128->64,2x2]": 6,
                     "t2h_conv3x3_wgrad[128->64,4x4]": 6, "t2h_conv3x3_wgrad[256->128,2x2]": 6,
                     "t2h_conv3x3_wgrad[256->128,4x4]": 4, "t2h_conv3x3_wgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_wgrad[32->32,8x8]": 1, "t2h_conv3x3_wgrad[64->32,4x4]": 1, "t2h_conv3x3_wgrad[64->32,8x8]": 1,
                     "t2h_conv3x3_wgrad[64->64,2x2]": 6, "t2h_conv3x3_wgrad[64->64,4x4]": 5, "t2h_conv3x3_wgrad[64->64,8x8]": 1,
                     "t2h_hg_avgpool2x2_bwd": 2, "t2h_hg_block_tail_bwd": 13, "t2h_hg_conv_s2_dgrad": 2,
                     "t2h_hg_conv_s2_wgrad": 2, "t2h_hg_groupnorm_bwd_apply": 44, "t2h_hg_groupnorm_bwd_reduce": 44,
                     "t2h_linear_dgrad": 8, "t2h_linear_wgrad": 8, "t2h_upsample_bicubic_bwd": 2},
    },
    "filter_conv128_frozen": {
        "forward": _FILTER_CONV128,
        "backward": {"t2h_conv3x3_dgrad[128->128,4x4]": 1, "t2h_conv3x3_dgrad[128->256,2x2]": 6,
                     "t2h_conv3x3_dgrad[128->256,4x4]": 4, "t2h_conv3x3_dgrad[32->32,4x4]": 1,
                     "t2h_conv3x3_dgrad[32->64,4x4]": 1, "t2h_conv3x3_dgrad[64->128,2x2]": 6,
                     "t2h_conv3x3_dgrad[64->128,4x4]": 6, "t2h_conv3x3_dgrad[64->64,2x2]": 6,
                     "t2h_conv3x3_dgrad[64->64,4x4]": 5, "t2h_conv3x3_wgrad[128->128,4x4]": 1,
                     "t2h_conv3x3_wgrad[128->64,2x2]": 6, "t2h_conv3x3_wgrad[128->64,4x4]": 6,
                     "t2h_conv3x3_wgrad[256->128,2x2]": 6, "t2h_conv3x3_wgrad[256->128,4x4]": 4,
                     "t2h_conv3x3_wgrad[32->32,4x4]": 1, "t2h_conv3x3_wgrad[64->32,4x4]": 1, "t2h_conv3x3_wgrad[64->64,2x2]": 6,
                     "t2h_conv3x3_wgrad[64->64,4x4]": 5, "t2h_hg_avgpool2x2_bwd": 2, "t2h_hg_block_tail_bwd": 12,
                     "t2h_hg_groupnorm_bwd_apply": 38, "t2h_hg_groupnorm_bwd_reduce": 39, "t2h_linear_dgrad": 7,
                     "t2h_linear_wgrad": 7, "t2h_upsample_bicubic_bwd": 2},
    },
}


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_calls_per_mode(name):
    got, want = cases()[name](), EXPECTED[name]
    for mode, table in got.items():
        print(f"{name} {mode}: {sum(table.values())} calls {table}")
    assert got["no_grad"] == want["forward"]
    assert sorted(got) == (["backward", "graph", "no_grad"] if "backward" in want else ["no_grad"])
    if "graph" in got:                                            # the graph forward launches what the forward without one does
        assert got["graph"] == got["no_grad"] and got["backward"] == want["backward"]


def test_every_case_has_a_table_and_the_downsample_block_is_the_one_read_off_the_code():
    assert sorted(EXPECTED) == sorted(cases()) == sorted(NAMES)
    assert [k for k in NAMES if "backward" not in EXPECTED[k]] == ["block64_128_batch"]
    block = EXPECTED["block64_128"]["forward"]                     # stats of x, out1, out2; bn1, bn4, bn2, bn3; three 3 x 3; 1 x 1; tail
    conv = sum(n for k, n in block.items() if k.startswith("t2h_conv3x3_fwd"))
    assert sum(block.values()) == 12 and conv == 3
    assert {k: n for k, n in block.items() if not k.startswith("t2h_conv3x3_fwd")} == {
        "t2h_hg_groupnorm_stats": 3, "t2h_hg_norm_apply": 4, "t2h_linear_fwd": 1, "t2h_hg_block_tail": 1}
