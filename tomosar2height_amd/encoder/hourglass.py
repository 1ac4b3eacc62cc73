"""HGFilter, the stacked-hourglass image encoder (reference: tomosar2height/encoder/hourglass.py:25-218), on the MI355X path.

Constructor signatures, defaults, attribute names and ``state_dict`` keys and shapes are the reference's -- ``bn4`` is also
``downsample.0`` (both keys, one storage) and exists unused when ``in_planes == out_planes``; the ``add_module`` names are
``b1_{k}``, ``b2_{k}``, ``b2_plus_1``, ``b3_{k}``, ``m{i}``, ``top_m_{i}``, ``conv_last{i}``, ``bn_end{i}``, ``l{i}``, ``bl{i}``,
``al{i}``; an unknown ``hg_down`` raises ``NameError`` and ``norm='group'`` with ``hg_down='conv64'`` fails at construction as
``GroupNorm(32, 16)`` does -- so a reference checkpoint loads with ``strict=True``.

Every layer runs on a t2h kernel over channels_last planes: the unbiased 3 x 3 convolutions on the kernels of ``grid.conv3x3_fwd_``,
every 1 x 1 convolution on ``grid.conv1x1`` (``previous + ll + tmp_out_`` rides its addend epilogue), ``up1 + up2`` on the bicubic
kernel's addend, and GroupNorm / folded BatchNorm, the stride-2 convolutions, the average pool and ``cat(out1, out2, out3) +
residual`` on csrc/hourglass.hip (include/t2h_hg.h, bound here: ``_lib.declare``).  ``bn1`` and ``bn4`` of a ConvBlock normalise
the same tensor with the same groups: one statistics pass serves both.  Layout: the kernels have no NCHW form, so an NCHW input is
converted at the module boundary, whatever ``TomoSAR2Height.set_channels_last`` says, and the output is channels_last memory.  H
and W of every plane must be powers of two (the 3 x 3 kernels), for ``HGFilter`` at least ``4 * 2 ** num_hourglass``: a
``ValueError`` before any launch otherwise.

Each module states its layer sequence once (``_fwd``), in terms of a small set of operations -- norm + ReLU for one or two affine
pairs with an optional pass-through of the input, 3 x 3 convolution, stride-2 convolution, pool, tail, upsample-add -- and runs it
on one of two implementations of that set: ``_Plain``, the kernel wrappers of this file under ``torch.no_grad()``, or ``_Graph``,
the autograd ``Function`` s over the same wrappers (``_GroupNorm``, ``grid._Conv3x3``, ``_ConvS2``, ``_AvgPool2x2``, ``_BlockTail``,
``_Upsample2xAdd``; ``grid.conv1x1`` serves both).  Both launch the same kernels on the same operands: the outputs are equal bit
for bit.

By default the modules run for inference (DESIGN.md sections 4.10 and 8): ``_Plain`` throughout, no autograd graph.  The forward
raises ``NotImplementedError`` when gradients are enabled and a parameter of the module requires one, and for ``norm='batch'``
under ``train()`` (batch statistics); ``norm='batch'`` in ``eval()`` runs on scale and shift folded from the running statistics,
``norm='group'`` computes the same thing in either mode.

Two keyword-only switches, both plain attributes (no parameter, no buffer, nothing in the ``state_dict``), add training:

* ``trainable=False`` on ``ConvBlock``, ``HourGlass`` and ``HGFilter``; setting it on a module sets it on the hourglass modules
  below it.  With ``trainable=True``, ``norm='group'`` and gradients enabled the forward runs on ``_Graph``: gradients reach every
  parameter behind the stem and, for ``ConvBlock`` and ``HourGlass``, the input, in ``train()`` and ``eval()`` alike.  Under
  ``torch.no_grad()`` the forward is the inference one.  ``HGFilter`` keeps its stem out of the graph: ``conv1`` -- and, for
  ``hg_down='conv64' / 'conv128'``, everything up to ``down_conv2``, since what lies in front of a stride-2 convolution would need
  its data gradient -- runs on ``_Plain`` and the image gets no gradient.
* ``stem_gradients=False`` on ``HGFilter``, read by the trainable forward only (so it can ride ``model.encoder2_kwargs``).  With
  ``trainable=True, stem_gradients=True`` the whole stem runs on ``_Graph``: ``conv1`` and ``down_conv2`` through ``_ConvS2``
  (``t2h_hg_conv_s2_dgrad`` / ``_wgrad``: the data gradient only for an input that needs one, the weight gradient only for a
  weight or bias that does), and an image with ``requires_grad`` gets ``.grad``.

Refused before any launch, in this order on the trainable path: ``norm='batch'`` with ``trainable=True``, in either mode and with
gradients enabled or not; without ``stem_gradients``, a stem layer named above that requires a gradient; then what every forward
checks -- device, dtype and rank of the input, the channel count, the plane size.  ``Trainer`` refuses a model whose image
encoder is trainable.

A tensor with two consumers inside a block (the block's input: bn1, bn4 and the identity residual; out1 and out2: the next norm
and the tail) is handed to the second one by the norm operation's pass-through -- the tensor itself on ``_Plain``, an alias out
of the ``_GroupNorm`` node on ``_Graph``, whose backward takes that consumer's gradient, and each affine pair's dx, as the addend
of the next apply: the tensor gets the sum of its gradients without a pass that only adds.

``group_norm``, ``avg_pool2x2``, ``conv2d_stride2`` and ``conv_block_tail`` are the differentiable operations on their own.
"""
import contextlib
import ctypes

import torch
import torch.nn as nn

from .. import _lib, grid

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

# name -> (restype, argtypes); mirrors include/t2h_hg.h one to one
SIGNATURES = {
    "t2h_hg_groupnorm_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "t2h_hg_groupnorm_stats": (_i, [_vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "t2h_hg_norm_apply": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "t2h_hg_conv_s2_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "t2h_hg_avgpool2x2": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "t2h_hg_block_tail": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _vp, _vp]),
    "t2h_hg_groupnorm_bwd_reduce": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "t2h_hg_groupnorm_bwd_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "t2h_hg_avgpool2x2_bwd": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "t2h_hg_block_tail_bwd": (_i, [_vp, _i64, _i, _vp, _vp, _vp, _vp]),
    "t2h_hg_conv_s2_dgrad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "t2h_hg_conv_s2_wgrad": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
}
GNB_PIXELS = 64              # T2H_HG_GNB_PIXELS: pixels of one sample per workgroup of the GroupNorm backward reduction
CS2_SLAB_ROWS, CS2_SLAB_COLS = 8, 32     # T2H_CS2_SLAB_ROWS / _COLS: output pixels of one slab of the stride-2 weight gradient

_lib.declare("t2h_hg.h", SIGNATURES)
load = _lib.load


# ------------------------------------------------------------------------------------------------ kernels
def _plane(x: torch.Tensor, what: str, detach: bool = True) -> torch.Tensor:
    """``x`` [B, C, H, W] float32 on the device, as a dense NHWC tensor (an NCHW input is converted here); ``detach=False``: with
    its place in the autograd graph (the trainable path)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{what}: expected a [B, C, H, W] tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: expected a tensor on the MI355X (cuda device), got {x.device}: tomosar2height_amd has no CPU path")
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: float32 expected, got {x.dtype}")
    return grid._as_cl(x.detach() if detach else x)


def group_norm_stats(x: torch.Tensor, groups: int, eps: float) -> torch.Tensor:
    """[B, G, 2] = (mean, rstd) of GroupNorm(groups, C) over the channels_last plane ``x``."""
    b, c, h, w = x.shape
    stats = torch.empty(b, groups, 2, dtype=torch.float32, device=x.device)
    nws = _lib.ws_bytes("t2h_hg_groupnorm_workspace_bytes", b, h, w, c, groups)
    if nws == 0:
        raise ValueError(f"group_norm_stats: no kernel for a {tuple(x.shape)} plane with {groups} groups")
    ws = _lib.workspace(nws, x.device)
    _lib.call("t2h_hg_groupnorm_stats", _lib.ptr(x), b, h, w, c, groups, float(eps), _lib.ptr(stats), _lib.ptr(ws), nws, _lib.stream(),
              nbytes=4 * x.numel())
    return stats


def norm_apply(x: torch.Tensor, stats, scale: torch.Tensor, shift: torch.Tensor, groups: int, relu: bool) -> torch.Tensor:
    """relu?(((x - mean) * rstd) * scale + shift) with ``stats`` of ``group_norm_stats``, or relu?(x * scale + shift) without."""
    b, c, h, w = x.shape
    y = grid._empty_cl(b, c, h, w, x.device)
    _lib.call("t2h_hg_norm_apply", _lib.ptr(x), _lib.ptr(stats) if stats is not None else None, _lib.ptr(scale), _lib.ptr(shift),
              b, h, w, c, groups, 1 if relu else 0, _lib.ptr(y), _lib.stream(), nbytes=8 * x.numel())
    return y


def conv_s2(x: torch.Tensor, w_kkio: torch.Tensor, bias, k: int, pad: int) -> torch.Tensor:
    """K x K / stride 2 / zero padding ``pad`` of the channels_last plane ``x``; ``w_kkio``: the weight as [K, K, Cin, Cout]."""
    b, cin, h, w = x.shape
    cout = w_kkio.shape[3]
    oh, ow = (h + 2 * pad - k) // 2 + 1, (w + 2 * pad - k) // 2 + 1
    y = grid._empty_cl(b, cout, oh, ow, x.device)
    _lib.call("t2h_hg_conv_s2_fwd", _lib.ptr(x), _lib.ptr(w_kkio), _lib.ptr(bias) if bias is not None else None, _lib.ptr(y),
              b, h, w, cin, cout, k, pad, _lib.stream(), nbytes=4 * (x.numel() + y.numel() + w_kkio.numel()),
              flops=2 * k * k * cin * cout * b * oh * ow)
    return y


def avgpool2x2(x: torch.Tensor) -> torch.Tensor:
    b, c, h, w = x.shape
    y = grid._empty_cl(b, c, h // 2, w // 2, x.device)
    _lib.call("t2h_hg_avgpool2x2", _lib.ptr(x), b, h, w, c, _lib.ptr(y), _lib.stream(), nbytes=4 * (x.numel() + y.numel()))
    return y


def block_tail(o1, o2, o3, res) -> torch.Tensor:
    """cat(o1, o2, o3, dim=1) + res in one pass."""
    b, c, h, w = res.shape
    if (o1.shape[1], o2.shape[1], o3.shape[1]) != (c // 2, c // 4, c // 4):
        raise ValueError("block_tail: inputs of C / 2, C / 4 and C / 4 channels expected")
    y = grid._empty_cl(b, c, h, w, res.device)
    _lib.call("t2h_hg_block_tail", _lib.ptr(o1), _lib.ptr(o2), _lib.ptr(o3), _lib.ptr(res), b * h * w, c, _lib.ptr(y), _lib.stream(),
              nbytes=12 * res.numel())
    return y


def upsample2x_bicubic_add(x: torch.Tensor, addend: torch.Tensor) -> torch.Tensor:
    """addend + F.interpolate(x, scale_factor=2, mode='bicubic', align_corners=True) on channels_last planes."""
    b, c, h, w = x.shape
    y = grid._empty_cl(b, c, 2 * h, 2 * w, x.device)
    _lib.call("t2h_upsample_bicubic_fwd", _lib.ptr(x), _lib.ptr(addend), b, c, h, w, 2 * h, 2 * w, 1, _lib.ptr(y), _lib.stream(),
              nbytes=4 * (x.numel() + 2 * y.numel()))
    return y


# ------------------------------------------------------------------------------------------------ adjoints
def gn_bwd_partial_floats(b: int, h: int, w: int, c: int) -> int:
    """Floats of the ``partial`` scratch of ``t2h_hg_groupnorm_bwd_reduce`` (the formula of include/t2h_hg.h)."""
    return b * (-(-(h * w) // GNB_PIXELS)) * 2 * c


def group_norm_bwd_reduce(gy, y, x, stats, gamma):
    """(gsum [B, G, 2], dbeta [C], dgamma [C]) of GroupNorm's backward; ``y``: the forward's output when a ReLU followed, else
    None.  ``gy``, ``y``, ``x``: channels_last planes; ``stats``: what ``group_norm_stats`` returned for ``x``."""
    b, c, h, w = x.shape
    groups = stats.shape[1]
    partial = torch.empty(gn_bwd_partial_floats(b, h, w, c), dtype=torch.float32, device=x.device)
    gsum = torch.empty(b, groups, 2, dtype=torch.float32, device=x.device)
    dbeta, dgamma = torch.empty(c, dtype=torch.float32, device=x.device), torch.empty(c, dtype=torch.float32, device=x.device)
    _lib.call("t2h_hg_groupnorm_bwd_reduce", _lib.ptr(gy), _lib.ptr(y) if y is not None else None, _lib.ptr(x), _lib.ptr(stats),
              _lib.ptr(gamma), b, h, w, c, groups, _lib.ptr(partial), _lib.ptr(gsum), _lib.ptr(dbeta), _lib.ptr(dgamma), _lib.stream(),
              nbytes=4 * x.numel() * (3 if y is not None else 2))
    return gsum, dbeta, dgamma


def group_norm_bwd_apply(gy, y, x, stats, gamma, gsum, addend=None) -> torch.Tensor:
    """dx of GroupNorm's backward [+ addend] from the group sums of ``group_norm_bwd_reduce``."""
    b, c, h, w = x.shape
    dx = grid._empty_cl(b, c, h, w, x.device)
    _lib.call("t2h_hg_groupnorm_bwd_apply", _lib.ptr(gy), _lib.ptr(y) if y is not None else None, _lib.ptr(x), _lib.ptr(stats),
              _lib.ptr(gamma), _lib.ptr(gsum), _lib.ptr(addend) if addend is not None else None, b, h, w, c, stats.shape[1], _lib.ptr(dx),
              _lib.stream(), nbytes=4 * x.numel() * (3 + (y is not None) + (addend is not None)))
    return dx


def avgpool2x2_bwd(gy: torch.Tensor, h: int, w: int) -> torch.Tensor:
    b, c = gy.shape[:2]
    dx = grid._empty_cl(b, c, h, w, gy.device)
    _lib.call("t2h_hg_avgpool2x2_bwd", _lib.ptr(gy), b, h, w, c, _lib.ptr(dx), _lib.stream(), nbytes=4 * (gy.numel() + dx.numel()))
    return dx


def block_tail_bwd(g: torch.Tensor):
    """The gradients of ``o1``, ``o2`` and ``o3`` of ``block_tail`` as three dense planes (that of ``res`` is ``g`` itself)."""
    b, c, h, w = g.shape
    d1, d2, d3 = (grid._empty_cl(b, n, h, w, g.device) for n in (c // 2, c // 4, c // 4))
    _lib.call("t2h_hg_block_tail_bwd", _lib.ptr(g), b * h * w, c, _lib.ptr(d1), _lib.ptr(d2), _lib.ptr(d3), _lib.stream(),
              nbytes=8 * g.numel())
    return d1, d2, d3


def conv_s2_wgrad_partial_floats(b: int, h: int, w: int, cin: int, cout: int, k: int, pad: int) -> int:
    """Floats of the ``partial`` scratch of ``t2h_hg_conv_s2_wgrad`` (the formula of include/t2h_hg.h)."""
    oh, ow = (h + 2 * pad - k) // 2 + 1, (w + 2 * pad - k) // 2 + 1
    return b * (-(-oh // CS2_SLAB_ROWS)) * (-(-ow // CS2_SLAB_COLS)) * (k * k * cin + 1) * cout


def conv_s2_dgrad(gy: torch.Tensor, w_kkio: torch.Tensor, h: int, w: int, k: int, pad: int, addend=None) -> torch.Tensor:
    """dx [B, Cin, H, W] (channels_last) of ``conv_s2`` [+ addend] from ``gy``, the channels_last gradient of its output."""
    b, cout = gy.shape[:2]
    cin = w_kkio.shape[2]
    if tuple(w_kkio.shape) != (k, k, cin, cout):
        raise ValueError(f"conv_s2_dgrad: a [{k}, {k}, Cin, {cout}] weight expected for this gy, got {tuple(w_kkio.shape)}")
    if k % 2 and 0 <= 2 * pad <= k and tuple(gy.shape[2:]) != ((h + 2 * pad - k) // 2 + 1, (w + 2 * pad - k) // 2 + 1):
        raise ValueError(f"conv_s2_dgrad: gy {tuple(gy.shape)} is not the output of a {h} x {w} plane")
    dx = grid._empty_cl(b, cin, h, w, gy.device)
    _lib.call("t2h_hg_conv_s2_dgrad", _lib.ptr(gy), _lib.ptr(w_kkio), _lib.ptr(addend) if addend is not None else None, _lib.ptr(dx),
              b, h, w, cin, cout, k, pad, _lib.stream(), nbytes=4 * (gy.numel() + w_kkio.numel() + dx.numel() * (1 + (addend is not None))),
              flops=2 * k * k * cin * cout * gy.shape[0] * gy.shape[2] * gy.shape[3])
    return dx


def conv_s2_wgrad(x: torch.Tensor, gy: torch.Tensor, k: int, pad: int, with_bias: bool = True):
    """(dw [K, K, Cin, Cout], dbias [Cout] or None) of ``conv_s2`` from its channels_last input and output gradient."""
    b, cin, h, w = x.shape
    cout = gy.shape[1]
    if gy.shape[0] != b or (k % 2 and 0 <= 2 * pad <= k and tuple(gy.shape[2:]) != ((h + 2 * pad - k) // 2 + 1, (w + 2 * pad - k) // 2 + 1)):
        raise ValueError(f"conv_s2_wgrad: gy {tuple(gy.shape)} is not the output of x {tuple(x.shape)}")
    dw = torch.empty(k, k, cin, cout, dtype=torch.float32, device=x.device)
    dbias = torch.empty(cout, dtype=torch.float32, device=x.device) if with_bias else None
    floats = conv_s2_wgrad_partial_floats(b, h, w, cin, cout, k, pad)
    partial = _lib.workspace(4 * floats, x.device)
    _lib.call("t2h_hg_conv_s2_wgrad", _lib.ptr(x), _lib.ptr(gy), _lib.ptr(partial), _lib.ptr(dw), _lib.ptr(dbias) if with_bias else None,
              b, h, w, cin, cout, k, pad, _lib.stream(), nbytes=4 * (x.numel() + gy.numel() + 2 * floats + dw.numel()),
              flops=2 * k * k * cin * cout * b * gy.shape[2] * gy.shape[3])
    return dw, dbias


class _ConvS2(torch.autograd.Function):
    """``conv_s2`` of a K x K / stride 2 ``nn.Conv2d`` weight [Cout, Cin, K, K] with its adjoints: the data gradient only when the
    input needs one (not for the stem's image), the weight gradient only for a weight or a bias that does."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_kkio, pad: int):
        x = grid._as_cl(x)
        ctx.save_for_backward(x, w_kkio)
        ctx.conf = (weight.shape[2], pad, bias is not None)
        return conv_s2(x, w_kkio, bias, weight.shape[2], pad)

    @staticmethod
    def backward(ctx, gy):
        x, w_kkio = ctx.saved_tensors
        k, pad, has_bias = ctx.conf
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        gy = grid._as_cl(gy)
        dx = conv_s2_dgrad(gy, w_kkio, x.shape[2], x.shape[3], k, pad) if need_x else None
        dw = db = None
        if need_w or need_b:
            dw, db = conv_s2_wgrad(x, gy, k, pad, with_bias=need_b)
            dw = dw.permute(3, 2, 0, 1).contiguous() if need_w else None          # the parameter's own [Cout, Cin, K, K]
        return dx, dw, db, None, None


class _GroupNorm(torch.autograd.Function):
    """``relu?(GroupNorm(x))`` for one or two (weight, bias) pairs over the same statistics -- ``bn1`` and ``bn4`` of a ConvBlock --:
    one output per pair and, ``thru``, ``x`` again (an alias) for another consumer of it.  The backward hands the gradient of
    that consumer, then each pair's dx, on as the next pair's addend: ``x`` gets the sum without a pass that only adds."""

    @staticmethod
    def forward(ctx, x, groups: int, eps: float, relu: bool, thru: bool, *affine):
        x = grid._as_cl(x)
        stats = group_norm_stats(x, groups, eps)
        ys = tuple(norm_apply(x, stats, affine[k], affine[k + 1], groups, relu) for k in range(0, len(affine), 2))
        ctx.save_for_backward(x, stats, *affine[0::2], *(ys if relu else ()))
        ctx.conf = (relu, thru, len(ys))
        ctx.set_materialize_grads(False)
        return ys + ((grid._alias(x),) if thru else ())

    @staticmethod
    def backward(ctx, *grads):
        relu, thru, n = ctx.conf
        x, stats = ctx.saved_tensors[:2]
        gammas = ctx.saved_tensors[2:2 + n]
        ys = ctx.saved_tensors[2 + n:] if relu else (None,) * n
        need_dx = ctx.needs_input_grad[0]
        dx = grid._as_cl(grads[n]) if thru and grads[n] is not None else None
        out = [None] * (2 * n)
        for k in reversed(range(n)):
            if grads[k] is None:
                continue
            gy = grid._as_cl(grads[k])
            gsum, out[2 * k + 1], out[2 * k] = group_norm_bwd_reduce(gy, ys[k], x, stats, gammas[k])
            if need_dx:
                dx = group_norm_bwd_apply(gy, ys[k], x, stats, gammas[k], gsum, dx)
        return (dx if need_dx else None, None, None, None, None) + tuple(out)


class _AvgPool2x2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = grid._as_cl(x)
        ctx.hw = (x.shape[2], x.shape[3])
        return avgpool2x2(x)

    @staticmethod
    def backward(ctx, g):
        return avgpool2x2_bwd(grid._as_cl(g), *ctx.hw)


class _BlockTail(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o1, o2, o3, res):
        return block_tail(grid._as_cl(o1), grid._as_cl(o2), grid._as_cl(o3), grid._as_cl(res))

    @staticmethod
    def backward(ctx, g):
        g = grid._as_cl(g)
        return block_tail_bwd(g) + (g,)


class _Upsample2xAdd(torch.autograd.Function):
    """``addend + bicubic x 2 (align_corners=True) of x`` on channels_last planes of any H x W (``ops.upsample_bicubic`` is the same
    pair of kernels for square outputs); the backward is the deterministic gather, the addend's gradient is ``g`` itself."""

    @staticmethod
    def forward(ctx, x, addend):
        x, addend = grid._as_cl(x), grid._as_cl(addend)
        ctx.shape = tuple(x.shape)
        return upsample2x_bicubic_add(x, addend)

    @staticmethod
    def backward(ctx, g):
        b, c, h, w = ctx.shape
        g = grid._as_cl(g)
        gin = grid._empty_cl(b, c, h, w, g.device)
        _lib.call("t2h_upsample_bicubic_bwd", _lib.ptr(g), b, c, h, w, 2 * h, 2 * w, 1, _lib.ptr(gin), _lib.stream(),
                  nbytes=4 * (g.numel() + gin.numel()))
        return gin, g


def group_norm(x: torch.Tensor, layer: nn.GroupNorm, relu: bool = False) -> torch.Tensor:
    """``relu?(layer(x))``, differentiable with respect to ``x`` and the layer's weight and bias."""
    x = _plane(x, "group_norm", detach=False)
    return _GroupNorm.apply(x, layer.num_groups, layer.eps, bool(relu), False, layer.weight, layer.bias)[0]


def avg_pool2x2(x: torch.Tensor) -> torch.Tensor:
    """``F.avg_pool2d(x, 2, stride=2)`` for even H and W, differentiable."""
    x = _plane(x, "avg_pool2x2", detach=False)
    if x.shape[2] % 2 or x.shape[3] % 2:
        raise ValueError(f"avg_pool2x2: H={x.shape[2]}, W={x.shape[3]} must be even (the adjoint writes whole windows)")
    return _AvgPool2x2.apply(x)


def conv2d_stride2(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor = None, padding: int = 0) -> torch.Tensor:
    """``F.conv2d(x, weight, bias, stride=2, padding=padding)`` for an odd K <= 7, ``padding <= K // 2`` and ``Cout % 64 == 0``,
    differentiable with respect to ``x``, ``weight`` and ``bias`` (``weight``: [Cout, Cin, K, K] as ``nn.Conv2d`` keeps it; it is
    re-laid to [K, K, Cin, Cout] on every call -- the modules cache that per weight version)."""
    x = _plane(x, "conv2d_stride2", detach=False)
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[1] != x.shape[1]:
        raise ValueError(f"conv2d_stride2: a [Cout, {x.shape[1]}, K, K] weight expected, got {tuple(weight.shape)}")
    return _ConvS2.apply(x, weight, bias, weight.detach().permute(2, 3, 1, 0).contiguous(), int(padding))


def conv_block_tail(o1, o2, o3, res) -> torch.Tensor:
    """``cat(o1, o2, o3, dim=1) + res``, differentiable."""
    o1, o2, o3, res = (_plane(t, "conv_block_tail", detach=False) for t in (o1, o2, o3, res))
    if (o1.shape[1], o2.shape[1], o3.shape[1]) != (res.shape[1] // 2, res.shape[1] // 4, res.shape[1] // 4):
        raise ValueError("conv_block_tail: inputs of C / 2, C / 4 and C / 4 channels expected")
    return _BlockTail.apply(o1, o2, o3, res)


# ------------------------------------------------------------------------------------------------ module plumbing
def _require_inference(module: nn.Module, what: str):
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        raise NotImplementedError(f"{what} runs for inference only (call it under torch.no_grad()): the backward of GroupNorm, of the "
                                  "stride-2 convolution, of the average pool and of the block tail is not built")
    if module.training and any(isinstance(m, nn.BatchNorm2d) for m in module.modules()):
        raise NotImplementedError(f"{what} with norm='batch' runs in eval() only: BatchNorm batch statistics are not built")


def _check_planes(x, what, min_h, min_w):
    h, w = x.shape[2], x.shape[3]
    if not (grid._pow2(h) and grid._pow2(w) and h >= min_h and w >= min_w):
        raise ValueError(f"{what}: H={h}, W={w} must be powers of two, at least {min_h} x {min_w} (the 3 x 3 convolution kernels "
                         "take power-of-two planes)")


def _weight_cl(conv):
    if not conv.weight.permute(0, 2, 3, 1).is_contiguous():          # the kernels read [Cout][3][3][Cin]: re-laid once, in place
        conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    return conv.weight


class _Plain:
    """The operations of the forward bodies on the kernel wrappers, without a graph (a namespace, never instantiated: plain
    functions); ``scope``: what a region of a forward that runs on this set is wrapped in."""
    scope = torch.no_grad
    pool, tail, up_add = avgpool2x2, block_tail, upsample2x_bicubic_add

    def norm(module, x, names, thru=False):
        """(relu(layer(x)) for the GroupNorm / eval-mode BatchNorm2d attributes ``names`` -- one, or two over the same statistics
        --, then, ``thru``, ``x`` again for another consumer of it)."""
        layers = [getattr(module, n) for n in names]
        if isinstance(layers[0], nn.GroupNorm):
            stats = group_norm_stats(x, layers[0].num_groups, layers[0].eps)
            ys = tuple(norm_apply(x, stats, layer.weight, layer.bias, layer.num_groups, True) for layer in layers)
        else:
            ys = tuple(norm_apply(x, None, *module._folded(n), 1, True) for n in names)
        return ys + ((x,) if thru else ())

    def conv3x3(x, conv):
        w = _weight_cl(conv)
        b, _, h, wd = x.shape
        return grid.conv3x3_fwd_(x, w, conv.bias, grid._empty_cl(b, w.shape[0], h, wd, x.device))

    def stride2(x, conv, w_kkio):
        return conv_s2(x, w_kkio, conv.bias, conv.kernel_size[0], conv.padding[0])


class _Graph:
    """The same operations as nodes of an autograd graph (``norm='group'``); ``thru`` is the alias the ``_GroupNorm`` returns."""
    scope = contextlib.nullcontext
    pool, tail, up_add = _AvgPool2x2.apply, _BlockTail.apply, _Upsample2xAdd.apply

    def norm(module, x, names, thru=False):
        layers = [getattr(module, n) for n in names]
        affine = [p for layer in layers for p in (layer.weight, layer.bias)]
        return _GroupNorm.apply(x, layers[0].num_groups, layers[0].eps, True, thru, *affine)

    def conv3x3(x, conv):
        _weight_cl(conv)
        if not grid.conv3x3_supported(x, conv):
            raise NotImplementedError(f"no 3 x 3 kernel for {conv.in_channels} -> {conv.out_channels} channels on a {tuple(x.shape[2:])} plane")
        return grid._Conv3x3.apply(x, conv.weight, conv.bias, False, False, False)

    def stride2(x, conv, w_kkio):
        return _ConvS2.apply(x, conv.weight, conv.bias, w_kkio, conv.padding[0])


class _HGModule(nn.Module):
    @property
    def trainable(self) -> bool:
        """The opt-in switch of the autograd path (a plain attribute: no parameter, no buffer, nothing in the ``state_dict``);
        setting it sets it on every hourglass module below this one."""
        return self.__dict__.get("_hg_trainable", False)

    @trainable.setter
    def trainable(self, flag: bool):
        self.__dict__["_hg_trainable"] = bool(flag)
        for child in self.children():
            if isinstance(child, _HGModule):
                child.trainable = flag

    def _builds_graph(self, what: str) -> bool:
        """True when this forward is the trainable one: the switch is on and gradients are enabled."""
        if not self.trainable:
            return False
        if any(isinstance(m, nn.BatchNorm2d) for m in self.modules()):
            raise NotImplementedError(f"{what}(trainable=True) with norm='batch' is not built, in train() or eval(): neither the "
                                      "frozen-BatchNorm backward nor batch statistics (norm='group' trains)")
        return torch.is_grad_enabled()

    def _begin(self, x, what: str, low: int):
        """What a forward starts with: (the operation set of this call, ``x`` as a checked plane of at least ``low`` x ``low``)."""
        graph = self._builds_graph(what)
        if not graph:
            _require_inference(self, what)
        x = _plane(x, what, detach=not graph)
        _check_planes(x, what, low, low)
        return (_Graph if graph else _Plain), x

    def _derived(self) -> _lib.Derived:
        d = self.__dict__.get("_hg_derived")
        if d is None:
            d = self.__dict__["_hg_derived"] = _lib.Derived()
        return d

    def _folded(self, name):
        """(scale, shift) of the eval-mode BatchNorm2d attribute ``name``, cached per version of its tensors."""
        layer = getattr(self, name)
        if layer.training:
            raise NotImplementedError("BatchNorm2d batch statistics are not built: norm='batch' runs in eval() only")

        def fold():          # float64, rounded once (as pointnetpp._FoldedLayers)
            s = layer.weight.double() / torch.sqrt(layer.running_var.double() + layer.eps)
            return (s.float().contiguous(), (layer.bias.double() - layer.running_mean.double() * s).float().contiguous())

        return self._derived().get(name, (layer.weight, layer.bias, layer.running_mean, layer.running_var), fold)

    def _conv_s2(self, ops, x, name):
        """The stride-2 convolution attribute ``name`` on its weight re-laid to [K, K, Cin, Cout], cached per weight version."""
        conv = getattr(self, name)
        w = self._derived().get(name, (conv.weight,), lambda: conv.weight.detach().permute(2, 3, 1, 0).contiguous())
        return ops.stride2(x, conv, w)


class ConvBlock(_HGModule):
    def __init__(self, in_planes, out_planes, norm="batch", *, trainable: bool = False):
        super().__init__()
        self.trainable = trainable
        self.conv1 = nn.Conv2d(in_planes, int(out_planes / 2), 3, 1, 1, bias=False)
        self.conv2 = nn.Conv2d(int(out_planes / 2), int(out_planes / 4), 3, 1, 1, bias=False)
        self.conv3 = nn.Conv2d(int(out_planes / 4), int(out_planes / 4), 3, 1, 1, bias=False)
        if norm == "batch":
            self.bn1 = nn.BatchNorm2d(in_planes)
            self.bn2 = nn.BatchNorm2d(int(out_planes / 2))
            self.bn3 = nn.BatchNorm2d(int(out_planes / 4))
            self.bn4 = nn.BatchNorm2d(in_planes)
        elif norm == "group":
            self.bn1 = nn.GroupNorm(32, in_planes)
            self.bn2 = nn.GroupNorm(32, int(out_planes / 2))
            self.bn3 = nn.GroupNorm(32, int(out_planes / 4))
            self.bn4 = nn.GroupNorm(32, in_planes)
        if in_planes != out_planes:
            self.downsample = nn.Sequential(self.bn4, nn.ReLU(inplace=True), nn.Conv2d(in_planes, out_planes, 1, 1, bias=False))
        else:
            self.downsample = None

    def _fwd(self, ops, x):
        """``x``, ``out1`` and ``out2`` each have two consumers: the second one takes the norm's pass-through."""
        if self.downsample is not None:
            y1, y4 = ops.norm(self, x, ("bn1", "bn4"))
            residual = grid.conv1x1(y4, self.downsample[2])
        else:
            y1, residual = ops.norm(self, x, ("bn1",), thru=True)
        out1 = ops.conv3x3(y1, self.conv1)
        y2, out1 = ops.norm(self, out1, ("bn2",), thru=True)
        out2 = ops.conv3x3(y2, self.conv2)
        y3, out2 = ops.norm(self, out2, ("bn3",), thru=True)
        out3 = ops.conv3x3(y3, self.conv3)
        return ops.tail(out1, out2, out3, residual)

    def forward(self, x):
        ops, x = self._begin(x, "ConvBlock", 1)
        with ops.scope():
            return self._fwd(ops, x)


class HourGlass(_HGModule):
    def __init__(self, num_modules, depth, num_features, norm="batch", *, trainable: bool = False):
        super().__init__()
        self.num_modules, self.depth, self.features, self.norm = num_modules, depth, num_features, norm
        self._generate_network(self.depth)
        self.trainable = trainable

    def _generate_network(self, level):
        self.add_module("b1_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        self.add_module("b2_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        if level > 1:
            self._generate_network(level - 1)
        else:
            self.add_module("b2_plus_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        self.add_module("b3_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))

    def _fwd(self, ops, level, inp):
        up1 = self._modules["b1_" + str(level)]._fwd(ops, inp)
        low1 = self._modules["b2_" + str(level)]._fwd(ops, ops.pool(inp))
        low2 = self._fwd(ops, level - 1, low1) if level > 1 else self._modules["b2_plus_" + str(level)]._fwd(ops, low1)
        low3 = self._modules["b3_" + str(level)]._fwd(ops, low2)
        return ops.up_add(low3, up1)

    def forward(self, x):
        ops, x = self._begin(x, "HourGlass", 2 ** self.depth)
        with ops.scope():
            return self._fwd(ops, self.depth, x)


class HGFilter(_HGModule):
    def __init__(self, in_channel, feature_dim=256, num_hourglass=2, num_stack=4, norm="group", hg_down="ave_pool", *,
                 trainable: bool = False, stem_gradients: bool = False):
        super().__init__()
        self.stem_gradients = bool(stem_gradients)     # (a plain attribute; consulted by the trainable forward only)
        self.in_channel = in_channel
        self.out_feature_dim = feature_dim
        self.num_hourglass = num_hourglass
        self.num_modules = num_stack
        self.norm = norm
        self.hg_down = hg_down
        self.conv1 = nn.Conv2d(self.in_channel, 64, kernel_size=7, stride=2, padding=3)
        if self.norm == "batch":
            self.bn1 = nn.BatchNorm2d(64)
        elif self.norm == "group":
            self.bn1 = nn.GroupNorm(32, 64)
        if self.hg_down == "conv64":
            self.conv2 = ConvBlock(64, 64, self.norm)
            self.down_conv2 = nn.Conv2d(64, 128, kernel_size=3, stride=2, padding=1)
        elif self.hg_down == "conv128":
            self.conv2 = ConvBlock(64, 128, self.norm)
            self.down_conv2 = nn.Conv2d(128, 128, kernel_size=3, stride=2, padding=1)
        elif self.hg_down == "ave_pool":
            self.conv2 = ConvBlock(64, 128, self.norm)
        else:
            raise NameError("Unknown HGFilter downsampling method!")
        self.conv3 = ConvBlock(128, 128, self.norm)
        self.conv4 = ConvBlock(128, 256, self.norm)
        for i in range(self.num_modules):
            self.add_module("m" + str(i), HourGlass(1, self.num_hourglass, 256, self.norm))
            self.add_module("top_m_" + str(i), ConvBlock(256, 256, self.norm))
            self.add_module("conv_last" + str(i), nn.Conv2d(256, 256, kernel_size=1, stride=1, padding=0))
            if self.norm == "batch":
                self.add_module("bn_end" + str(i), nn.BatchNorm2d(256))
            elif self.norm == "group":
                self.add_module("bn_end" + str(i), nn.GroupNorm(32, 256))
            self.add_module("l" + str(i), nn.Conv2d(256, self.out_feature_dim, kernel_size=1, stride=1, padding=0))
            if i < self.num_modules - 1:
                self.add_module("bl" + str(i), nn.Conv2d(256, 256, kernel_size=1, stride=1, padding=0))
                self.add_module("al" + str(i), nn.Conv2d(self.out_feature_dim, 256, kernel_size=1, stride=1, padding=0))
        self.trainable = trainable

    def _frozen_stem(self):
        """The layers the trainable forward runs without a graph: ``conv1`` -- and, where ``down_conv2`` follows, everything up to it,
        since what lies in front of a stride-2 convolution would need its data gradient."""
        names = ("conv1",) if self.hg_down == "ave_pool" else ("conv1", "bn1", "conv2", "down_conv2")
        wants = [f"{n}.{k}" for n in names for k, p in getattr(self, n).named_parameters() if p.requires_grad]
        if wants:
            raise NotImplementedError(f"HGFilter(trainable=True) runs with a frozen stem: {', '.join(wants)} require a gradient, but the "
                                      "stride-2 convolution's weight / data gradient is not built (conv1"
                                      + ("" if self.hg_down == "ave_pool" else ", down_conv2 and what lies in front of it")
                                      + "); call requires_grad_(False) on them")

    def forward(self, x, trace: dict = None):
        """``x`` [B, in_channel, H, W] -> [B, feature_dim, H / 4, W / 4] (channels_last memory).  ``trace``: a dict that receives
        ``stem``, ``conv2``, ``conv3``, ``conv4`` and per stack ``hg{i}``, ``ll{i}``, ``tmp_out{i}``."""
        graph = self._builds_graph("HGFilter")
        if not graph:
            _require_inference(self, "HGFilter")
        elif not self.stem_gradients:
            self._frozen_stem()
        x = _plane(x, "HGFilter", detach=not (graph and self.stem_gradients))      # (with the stem in the graph the image gets .grad)
        if x.shape[1] != self.in_channel:
            raise ValueError(f"HGFilter: {self.in_channel} input channels expected, got {x.shape[1]}")
        low = 4 * 2 ** self.num_hourglass
        _check_planes(x, "HGFilter", low, low)
        if self.hg_down not in ("ave_pool", "conv64", "conv128"):
            raise NameError("Unknown HGFilter downsampling method!")
        # the operation set per region: ``conv1``; ``bn1`` .. the pool / ``down_conv2``; everything behind.  A frozen stem stays
        # without a graph up to its last stride-2 convolution
        rest = _Graph if graph else _Plain
        head = rest if self.stem_gradients else _Plain
        front = rest if self.stem_gradients or self.hg_down == "ave_pool" else _Plain
        rec = trace.__setitem__ if trace is not None else (lambda k, v: None)
        m = self._modules
        with rest.scope():
            with head.scope():
                x = self._conv_s2(head, x, "conv1")
            with front.scope():
                x = front.norm(self, x, ("bn1",))[0]
                rec("stem", x)
                x = self.conv2._fwd(front, x)
                rec("conv2", x)
                x = front.pool(x) if self.hg_down == "ave_pool" else self._conv_s2(front, x, "down_conv2")
            x = self.conv3._fwd(rest, x)
            rec("conv3", x)
            x = self.conv4._fwd(rest, x)
            rec("conv4", x)
            previous, tmp_out = x, None
            for i in range(self.num_modules):
                hg = m["m" + str(i)]._fwd(rest, self.num_hourglass, previous)
                ll = m["top_m_" + str(i)]._fwd(rest, hg)
                ll = rest.norm(self, grid.conv1x1(ll, m["conv_last" + str(i)]), ("bn_end" + str(i),))[0]
                tmp_out = grid.conv1x1(ll, m["l" + str(i)])
                rec(f"hg{i}", hg), rec(f"ll{i}", ll), rec(f"tmp_out{i}", tmp_out)
                if i < self.num_modules - 1:
                    previous = grid.conv1x1(tmp_out, m["al" + str(i)], grid.conv1x1(ll, m["bl" + str(i)], previous))
        return tmp_out
