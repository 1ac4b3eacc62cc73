"""Plain-torch restatement of the hourglass image encoder (reference: tomosar2height/encoder/hourglass.py; here:
tomosar2height_amd/encoder/hourglass.py, include/t2h_hg.h), written against the ``state_dict`` keys alone, so it runs on the
parameters of either implementation, in float64 (the tests' oracle) or float32 (the probe's baseline), on any device:

    group_norm   (x - mean) / sqrt(var + eps) * gamma + beta, mean and biased variance over (C / G, H, W) per sample and group
    batch_norm   eval(): (x - running_mean) / sqrt(running_var + eps) * gamma + beta
    conv         F.conv2d (the strided ones with their stride and zero padding)
    avg_pool     the mean of the four pixels of every 2 x 2 window
    block        cat(out1, out2, out3) + residual with out_k = conv_k(relu(bn_k(.))); the residual goes through
                 conv1x1(relu(bn4(x))) when the channel count changes
    hourglass    up1 = b1(x); low = b3(inner(b2(avg_pool(x)))); up1 + bicubic x 2 (align_corners=True) of low
    hg_filter    stem, conv2, down, conv3, conv4 and the stacks with the inter-stack previous + bl(ll) + al(tmp_out)

plus the deterministic parameter fill the fixture generator and the tests share (``init_hg_``) and the fixture's cases.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from detinit import det_init_

# name -> (B, H, W, constructor arguments); every case has in_channel = 3, feature_dim = 32
CASES = {
    "g64": (1, 64, 64, dict(norm="group", hg_down="ave_pool", num_stack=2, num_hourglass=2)),
    "g32b2": (2, 32, 32, dict()),
    "c128": (1, 64, 32, dict(hg_down="conv128", num_stack=1, num_hourglass=3)),
    "bn32": (1, 32, 32, dict(norm="batch", hg_down="conv64", num_stack=1, num_hourglass=2)),
}
SEED = 43
MODEL_CASE = "model64"


def case_kwargs(name):
    return dict(in_channel=3, feature_dim=32, **CASES[name][3])


def case_image(name):
    """The input image of a case: uniform in [-1, 1), seeded by the case's name."""
    b, h, w = (1, 64, 64) if name == MODEL_CASE else CASES[name][:3]
    g = torch.Generator().manual_seed(zlib.crc32(("image:" + name).encode()) % (2 ** 31))
    return torch.rand(b, 3, h, w, generator=g, dtype=torch.float32) * 2 - 1


def tensor_names(num_stack):
    return ["stem", "conv2", "conv3", "conv4"] + [f"{k}{i}" for i in range(num_stack) for k in ("hg", "ll", "tmp_out")] + ["out"]


# ------------------------------------------------------------------------------------------------ parameters
def init_hg_(model: torch.nn.Module, seed: int = SEED) -> torch.nn.Module:
    """``det_init_`` for the parameters, then name-keyed non-trivial affine parameters of every GroupNorm / BatchNorm2d (gamma in
    [0.75, 1.25), beta in [-0.1, 0.1)) and, for BatchNorm2d, running_mean in [-0.1, 0.1) and running_var in [0.5, 1.5).  A layer
    registered under two names (``bn4`` / ``downsample.0``) is keyed by the first."""
    det_init_(model, seed=seed)
    with torch.no_grad():
        for name, m in sorted(model.named_modules()):
            if not isinstance(m, (torch.nn.GroupNorm, torch.nn.BatchNorm2d)):
                continue
            g = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(("norm:" + name).encode())) % (2 ** 31))
            u = torch.rand(4, m.weight.numel(), generator=g, dtype=torch.float32)
            m.weight.copy_(0.75 + 0.5 * u[0])
            m.bias.copy_(0.2 * u[1] - 0.1)
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * u[2] - 0.1)
                m.running_var.copy_(0.5 + u[3])
                m.num_batches_tracked.fill_(7)
    return model


def params_of(module, dtype=torch.float64, device=None):
    """The module's ``state_dict`` as detached tensors of ``dtype`` (integer buffers left alone)."""
    return {k: (v.detach().to(device=device, dtype=dtype) if v.is_floating_point() else v.detach().to(device=device))
            for k, v in module.state_dict().items()}


# ------------------------------------------------------------------------------------------------ layers
def group_norm(x, groups, gamma, beta, eps=1e-5, relu=False, stats=False):
    b, c, h, w = x.shape
    xg = x.reshape(b, groups, -1)
    mean = xg.mean(dim=2, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=2, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = ((xg - mean) * rstd).reshape(b, c, h, w) * gamma.view(1, c, 1, 1) + beta.view(1, c, 1, 1)
    y = torch.clamp_min(y, 0) if relu else y
    return (y, mean.reshape(b, groups), rstd.reshape(b, groups)) if stats else y


def batch_norm_eval(x, p, prefix, eps=1e-5, relu=False):
    c = x.shape[1]
    s = p[prefix + ".weight"] / torch.sqrt(p[prefix + ".running_var"] + eps)
    y = (x - p[prefix + ".running_mean"].view(1, c, 1, 1)) * s.view(1, c, 1, 1) + p[prefix + ".bias"].view(1, c, 1, 1)
    return torch.clamp_min(y, 0) if relu else y


def norm(x, p, prefix, relu=True):
    if prefix + ".running_var" in p:
        return batch_norm_eval(x, p, prefix, relu=relu)
    return group_norm(x, 32, p[prefix + ".weight"], p[prefix + ".bias"], relu=relu)


def conv(x, p, prefix, stride=1, padding=0):
    return F.conv2d(x, p[prefix + ".weight"], p.get(prefix + ".bias"), stride=stride, padding=padding)


def avg_pool(x):
    return (((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + x[:, :, 1::2, 0::2]) + x[:, :, 1::2, 1::2]) * 0.25


def block_tail(o1, o2, o3, res):
    return torch.cat((o1, o2, o3), 1) + res


def block(x, p, prefix):
    out1 = conv(norm(x, p, prefix + ".bn1"), p, prefix + ".conv1", padding=1)
    out2 = conv(norm(out1, p, prefix + ".bn2"), p, prefix + ".conv2", padding=1)
    out3 = conv(norm(out2, p, prefix + ".bn3"), p, prefix + ".conv3", padding=1)
    residual = x
    if prefix + ".downsample.2.weight" in p:
        residual = conv(norm(x, p, prefix + ".bn4"), p, prefix + ".downsample.2")
    return block_tail(out1, out2, out3, residual)


def hourglass(x, p, prefix, level):
    up1 = block(x, p, f"{prefix}.b1_{level}")
    low = block(avg_pool(x), p, f"{prefix}.b2_{level}")
    low = hourglass(low, p, prefix, level - 1) if level > 1 else block(low, p, f"{prefix}.b2_plus_{level}")
    low = block(low, p, f"{prefix}.b3_{level}")
    return up1 + F.interpolate(low, scale_factor=2, mode="bicubic", align_corners=True)


def hg_filter(x, p, num_hourglass=2, num_stack=4, hg_down="ave_pool", trace=None, **_):
    """HGFilter.forward on the parameters ``p`` (keys without a prefix); ``trace`` receives every tensor of ``tensor_names``."""
    rec = (lambda k, v: trace.__setitem__(k, v)) if trace is not None else (lambda k, v: None)
    x = norm(conv(x, p, "conv1", stride=2, padding=3), p, "bn1")
    rec("stem", x)
    x = block(x, p, "conv2")
    rec("conv2", x)
    x = avg_pool(x) if hg_down == "ave_pool" else conv(x, p, "down_conv2", stride=2, padding=1)
    x = block(x, p, "conv3")
    rec("conv3", x)
    x = block(x, p, "conv4")
    rec("conv4", x)
    previous, out = x, None
    for i in range(num_stack):
        hg = hourglass(previous, p, f"m{i}", num_hourglass)
        ll = block(hg, p, f"top_m_{i}")
        ll = norm(conv(ll, p, f"conv_last{i}"), p, f"bn_end{i}")
        out = conv(ll, p, f"l{i}")
        rec(f"hg{i}", hg), rec(f"ll{i}", ll), rec(f"tmp_out{i}", out)
        if i < num_stack - 1:
            previous = previous + conv(ll, p, f"bl{i}") + conv(out, p, f"al{i}")
    rec("out", out)
    return out


class TorchHGFilter(torch.nn.Module):
    """The restatement as a module over a copy of another implementation's parameters (the probe's plain-torch baseline)."""

    def __init__(self, source, dtype=torch.float32, device=None):
        super().__init__()
        self.kwargs = dict(num_hourglass=source.num_hourglass, num_stack=source.num_modules, hg_down=source.hg_down)
        self.p = params_of(source, dtype, device)

    def forward(self, x, trace=None):
        with torch.no_grad():
            return hg_filter(x, self.p, trace=trace, **self.kwargs)


# ------------------------------------------------------------------------------------------------ fixture access
def ref64(g, name, key):
    """(ref64, tolerance): the float64 result rebuilt from the stored float32 one, and 4 x max|ref32 - ref64|."""
    dev = float(g[f"{name}_{key}_dev"])
    return g[f"{name}_{key}"].astype(np.float64) + g[f"{name}_{key}_q"].astype(np.float64) * dev, 4.0 * dev


def model_cfg(g):
    """The configuration tests/golden/make_golden_hourglass.py built its full reference model with."""
    from tomosar2height_amd.config import berlin_config
    cfg = berlin_config()
    cfg.use_image = True
    cfg.model.encoder_kwargs = dict(hidden_dim=int(g["feature_dim"]), feature_dim=int(g["feature_dim"]), plane_resolution=int(g["resolution"]),
                                    scatter_type="max", unet_type="alto", unet_kwargs=dict(depth=3, merge_mode="concat", start_filts=32))
    cfg.model.encoder2 = "hourglass"
    cfg.model.encoder2_kwargs = dict(in_channel=3, feature_dim=int(g["feature_dim"]), num_stack=int(g["model_num_stack"]),
                                     num_hourglass=int(g["model_num_hourglass"]))
    cfg.model.decoder_pixel_kwargs.output_size = int(g["output_size"])
    return cfg
