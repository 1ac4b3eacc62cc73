"""HGFilter, the stacked-hourglass image encoder (reference: tomosar2height/encoder/hourglass.py:25-218), on the MI355X path, for
inference.

Constructor signatures, defaults, attribute names and ``state_dict`` keys and shapes are the reference's -- ``bn4`` is also
``downsample.0`` (both keys, one storage) and exists unused when ``in_planes == out_planes``; the ``add_module`` names are
``b1_{k}``, ``b2_{k}``, ``b2_plus_1``, ``b3_{k}``, ``m{i}``, ``top_m_{i}``, ``conv_last{i}``, ``bn_end{i}``, ``l{i}``, ``bl{i}``,
``al{i}``; an unknown ``hg_down`` raises ``NameError`` and ``norm='group'`` with ``hg_down='conv64'`` fails at construction as
``GroupNorm(32, 16)`` does -- so a reference checkpoint loads with ``strict=True``.

Every layer runs on a t2h kernel over channels_last planes: the unbiased 3 x 3 convolutions on ``grid.conv3x3_fwd_``, every 1 x 1
convolution on ``grid.conv1x1`` (``previous + ll + tmp_out_`` rides its addend epilogue), ``up1 + up2`` on the bicubic kernel's
addend, and GroupNorm / folded BatchNorm, the stride-2 convolutions, the average pool and ``cat(out1, out2, out3) + residual``
on csrc/hourglass.hip (include/t2h_hg.h, bound here: ``_lib.declare``).  ``bn1`` and ``bn4`` of a ConvBlock normalise the same
tensor with the same groups: one statistics pass serves both.  The kernels have no NCHW form: an NCHW input is converted at the
module boundary, whatever ``TomoSAR2Height.set_channels_last`` says, and the output is channels_last memory.

Inference only (DESIGN.md sections 4.10 and 8).  The forward builds no autograd graph.  It raises ``NotImplementedError`` when
gradients are enabled and a parameter of the module requires one, and for ``norm='batch'`` under ``train()`` (batch statistics);
``norm='group'`` computes the same thing in either mode.  H and W of every plane must be powers of two (the 3 x 3 kernels), for
``HGFilter`` at least ``4 * 2 ** num_hourglass``: a ``ValueError`` before any launch otherwise.
"""
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
}

_lib.declare("t2h_hg.h", SIGNATURES)
load = _lib.load


# ------------------------------------------------------------------------------------------------ kernels
def _plane(x: torch.Tensor, what: str) -> torch.Tensor:
    """``x`` [B, C, H, W] float32 on the device, as a dense NHWC tensor (an NCHW input is converted here)."""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{what}: expected a [B, C, H, W] tensor")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: expected a tensor on the MI355X (cuda device), got {x.device}: tomosar2height_amd has no CPU path")
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: float32 expected, got {x.dtype}")
    return grid._as_cl(x.detach())


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


class _HGModule(nn.Module):
    def _derived(self) -> _lib.Derived:
        d = self.__dict__.get("_hg_derived")
        if d is None:
            d = self.__dict__["_hg_derived"] = _lib.Derived()
        return d

    def _norm(self, x, name, relu, stats=None):
        """relu?(layer(x)) for the GroupNorm / eval-mode BatchNorm2d attribute ``name``; ``stats``: GroupNorm statistics of ``x``
        already at hand."""
        layer = getattr(self, name)
        if isinstance(layer, nn.GroupNorm):
            if stats is None:
                stats = group_norm_stats(x, layer.num_groups, layer.eps)
            return norm_apply(x, stats, layer.weight, layer.bias, layer.num_groups, relu)
        if layer.training:
            raise NotImplementedError("BatchNorm2d batch statistics are not built: norm='batch' runs in eval() only")

        def fold():          # float64, rounded once (as pointnetpp._FoldedLayers)
            s = layer.weight.double() / torch.sqrt(layer.running_var.double() + layer.eps)
            return (s.float().contiguous(), (layer.bias.double() - layer.running_mean.double() * s).float().contiguous())

        scale, shift = self._derived().get(name, (layer.weight, layer.bias, layer.running_mean, layer.running_var), fold)
        return norm_apply(x, None, scale, shift, 1, relu)

    def _conv3x3(self, x, conv):
        w = conv.weight
        if not w.permute(0, 2, 3, 1).is_contiguous():          # the kernels read [Cout][3][3][Cin]: re-laid once, in place
            conv.weight.data = w.data.contiguous(memory_format=torch.channels_last)
            w = conv.weight
        b, _, h, wd = x.shape
        y = grid._empty_cl(b, w.shape[0], h, wd, x.device)
        return grid.conv3x3_fwd_(x, w, conv.bias, y)

    def _conv_s2(self, x, name):
        conv = getattr(self, name)
        w = self._derived().get(name, (conv.weight,), lambda: conv.weight.detach().permute(2, 3, 1, 0).contiguous())
        return conv_s2(x, w, conv.bias, conv.kernel_size[0], conv.padding[0])


class ConvBlock(_HGModule):
    def __init__(self, in_planes, out_planes, norm="batch"):
        super().__init__()
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

    def _fwd(self, x):
        stats = group_norm_stats(x, self.bn1.num_groups, self.bn1.eps) if isinstance(self.bn1, nn.GroupNorm) else None
        out1 = self._conv3x3(self._norm(x, "bn1", True, stats), self.conv1)
        out2 = self._conv3x3(self._norm(out1, "bn2", True), self.conv2)
        out3 = self._conv3x3(self._norm(out2, "bn3", True), self.conv3)
        residual = x
        if self.downsample is not None:
            residual = grid.conv1x1(self._norm(x, "bn4", True, stats), self.downsample[2])
        return block_tail(out1, out2, out3, residual)

    def forward(self, x):
        _require_inference(self, "ConvBlock")
        x = _plane(x, "ConvBlock")
        _check_planes(x, "ConvBlock", 1, 1)
        with torch.no_grad():
            return self._fwd(x)


class HourGlass(_HGModule):
    def __init__(self, num_modules, depth, num_features, norm="batch"):
        super().__init__()
        self.num_modules, self.depth, self.features, self.norm = num_modules, depth, num_features, norm
        self._generate_network(self.depth)

    def _generate_network(self, level):
        self.add_module("b1_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        self.add_module("b2_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        if level > 1:
            self._generate_network(level - 1)
        else:
            self.add_module("b2_plus_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))
        self.add_module("b3_" + str(level), ConvBlock(self.features, self.features, norm=self.norm))

    def _fwd(self, level, inp):
        up1 = self._modules["b1_" + str(level)]._fwd(inp)
        low1 = self._modules["b2_" + str(level)]._fwd(avgpool2x2(inp))
        low2 = self._fwd(level - 1, low1) if level > 1 else self._modules["b2_plus_" + str(level)]._fwd(low1)
        low3 = self._modules["b3_" + str(level)]._fwd(low2)
        return upsample2x_bicubic_add(low3, up1)

    def forward(self, x):
        _require_inference(self, "HourGlass")
        x = _plane(x, "HourGlass")
        _check_planes(x, "HourGlass", 2 ** self.depth, 2 ** self.depth)
        with torch.no_grad():
            return self._fwd(self.depth, x)


class HGFilter(_HGModule):
    def __init__(self, in_channel, feature_dim=256, num_hourglass=2, num_stack=4, norm="group", hg_down="ave_pool"):
        super().__init__()
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

    def forward(self, x, trace: dict = None):
        """``x`` [B, in_channel, H, W] -> [B, feature_dim, H / 4, W / 4] (channels_last memory).  ``trace``: a dict that receives
        ``stem``, ``conv2``, ``conv3``, ``conv4`` and per stack ``hg{i}``, ``ll{i}``, ``tmp_out{i}``."""
        _require_inference(self, "HGFilter")
        x = _plane(x, "HGFilter")
        if x.shape[1] != self.in_channel:
            raise ValueError(f"HGFilter: {self.in_channel} input channels expected, got {x.shape[1]}")
        low = 4 * 2 ** self.num_hourglass
        _check_planes(x, "HGFilter", low, low)
        if self.hg_down not in ("ave_pool", "conv64", "conv128"):
            raise NameError("Unknown HGFilter downsampling method!")
        rec = (lambda k, v: trace.__setitem__(k, v)) if trace is not None else (lambda k, v: None)
        with torch.no_grad():
            x = self._norm(self._conv_s2(x, "conv1"), "bn1", True)
            rec("stem", x)
            x = self.conv2._fwd(x)
            rec("conv2", x)
            x = avgpool2x2(x) if self.hg_down == "ave_pool" else self._conv_s2(x, "down_conv2")
            x = self.conv3._fwd(x)
            rec("conv3", x)
            x = self.conv4._fwd(x)
            rec("conv4", x)
            previous, tmp_out = x, None
            for i in range(self.num_modules):
                m = self._modules
                hg = m["m" + str(i)]._fwd(self.num_hourglass, previous)
                ll = m["top_m_" + str(i)]._fwd(hg)
                ll = self._norm(grid.conv1x1(ll, m["conv_last" + str(i)]), "bn_end" + str(i), True)
                tmp_out = grid.conv1x1(ll, m["l" + str(i)])
                rec(f"hg{i}", hg), rec(f"ll{i}", ll), rec(f"tmp_out{i}", tmp_out)
                if i < self.num_modules - 1:
                    previous = grid.conv1x1(tmp_out, m["al" + str(i)], grid.conv1x1(ll, m["bl" + str(i)], previous))
        return tmp_out
