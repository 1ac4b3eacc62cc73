"""GPU: the hourglass encoder's kernels (csrc/hourglass.hip through tomosar2height_amd.encoder.hourglass) against float64 computed
on the host from the same inputs, and the encoder built on them against the fixture of the reference's own modules
(tests/golden/make_golden_hourglass.py).

Kernel bars: the same float64 comparison is made for torch's own float32 operator on the host on the same inputs; the kernel
gets 4 x that worst deviation per shape (another accumulation order, the same precision).  The average pool and the block tail
are compared bit for bit with a float32 host computation in the kernel's order.  Composed results: within 4 x max|ref32 - ref64|
of ref64.

Measured against the composed bar (4 x ref32_dev), worst ratio err / ref32_dev over every tensor of g64, g32b2, c128 and bn32:
see DESIGN.md section 4.10.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hg_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = tuple(hg_ref.CASES)
PRECISIONS = ("f16x2", "fp32")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("hourglass_encoder")
    return _cache["g"]


def cl(t):
    """A host NCHW tensor as a channels_last device tensor."""
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def host(t):
    return t.detach().float().cpu().contiguous()


def encoder(name):
    from tomosar2height_amd.encoder import encoder_dict
    if name not in _cache:
        _cache[name] = hg_ref.init_hg_(encoder_dict["hourglass"](**hg_ref.case_kwargs(name))).to(DEV).eval()
    return _cache[name]


class precision:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from tomosar2height_amd import grid
        grid.set_conv_precision(self.name)

    def __exit__(self, *exc):
        from tomosar2height_amd import grid
        grid.set_conv_precision(None)


def worst(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max())


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_SHAPES = [(c, 32, h, w) for c in (32, 64, 128, 256) for (h, w) in ((2, 1), (16, 16))] + [(64, 32, 128, 128)]


@pytest.mark.parametrize("c,groups,h,w", GN_SHAPES)
def test_group_norm_against_float64(c, groups, h, w):
    from tomosar2height_amd.encoder import hourglass as hg
    gen = torch.Generator().manual_seed(1000 * c + h)
    x = torch.randn(2, c, h, w, generator=gen)
    x[0] *= 0.05                                                   # two samples of different scale;
    x[1] += 100.0                                                  # one with mean 100 and unit spread
    gamma, beta = 0.75 + 0.5 * torch.rand(c, generator=gen), 0.2 * torch.rand(c, generator=gen) - 0.1
    eps = 1e-5
    y64, mean64, rstd64 = (t.numpy() for t in hg_ref.group_norm(x.double(), groups, gamma.double(), beta.double(), eps, stats=True))
    t_out, t_mean, t_rstd = torch.native_group_norm(x, gamma, beta, 2, c, h * w, groups, eps)          # torch's own float32, on the host
    xd = cl(x)
    assert hg.load().t2h_hg_groupnorm_workspace_bytes(2, h, w, c, groups) == (1 if h * w * c <= 65536 else 2 * (h * w * c // 65536) * groups * 12)
    stats = hg.group_norm_stats(xd, groups, eps)
    again = hg.group_norm_stats(xd, groups, eps)
    assert tuple(stats.shape) == (2, groups, 2) and torch.equal(stats, again)
    got = host(stats).numpy()
    for key, mine, theirs, ref in (("mean", got[..., 0], t_mean.numpy(), mean64), ("rstd", got[..., 1], t_rstd.numpy(), rstd64)):
        bar = 4 * worst(theirs, ref)
        err = worst(mine, ref)
        print(f"GroupNorm C={c} {h}x{w} {key}: err {err:.3g} (per sample {worst(mine[0], ref[0]):.3g}, {worst(mine[1], ref[1]):.3g}), "
              f"torch float32 {bar / 4:.3g}, bar {bar:.3g}")
        assert err <= bar, (key, err, bar)
    for relu in (False, True):
        y = hg.norm_apply(xd, stats, gamma.to(DEV), beta.to(DEV), groups, relu)
        y2 = hg.norm_apply(xd, stats, gamma.to(DEV), beta.to(DEV), groups, relu)
        assert torch.equal(y, y2) and y.shape == x.shape
        ref = np.maximum(y64, 0) if relu else y64
        theirs = (t_out.clamp_min(0) if relu else t_out).numpy()
        mine = host(y).numpy()
        bar = 4 * worst(theirs, ref)
        err = worst(mine, ref)
        print(f"GroupNorm C={c} {h}x{w} relu={relu}: err {err:.3g} (per sample {worst(mine[0], ref[0]):.3g}, {worst(mine[1], ref[1]):.3g}), "
              f"torch float32 {bar / 4:.3g} (per sample {worst(theirs[0], ref[0]):.3g}, {worst(theirs[1], ref[1]):.3g}), bar {bar:.3g}")
        assert err <= bar, (relu, err, bar)
        if relu:
            assert float(y.min()) == 0.0


def test_folded_batch_norm_apply_against_float64():
    """The statistics-free form: y = relu?(x * scale + shift), two roundings per element."""
    from tomosar2height_amd.encoder import hourglass as hg
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(2, 64, 8, 4, generator=gen)
    scale, shift = 0.5 + torch.rand(64, generator=gen), torch.randn(64, generator=gen)
    for relu in (False, True):
        y = host(hg.norm_apply(cl(x), None, scale.to(DEV), shift.to(DEV), 1, relu))
        want = x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        assert torch.equal(y, want.clamp_min(0) if relu else want)


# ------------------------------------------------------------------------------------------------ strided convolution
CONV_SHAPES = [(7, 3, cin, 64, b, h, w) for cin in (2, 3) for (b, h, w) in ((1, 32, 32), (1, 16, 64), (2, 32, 32))] + [
    (3, 1, 64, 128, 1, 16, 8), (3, 1, 128, 128, 1, 16, 8)]


@pytest.mark.parametrize("k,pad,cin,cout,b,h,w", CONV_SHAPES)
@pytest.mark.parametrize("with_bias", (True, False))
def test_strided_convolution_against_float64(k, pad, cin, cout, b, h, w, with_bias):
    from tomosar2height_amd.encoder import hourglass as hg
    gen = torch.Generator().manual_seed(100 * k + cin + h)
    x = torch.randn(b, cin, h, w, generator=gen)
    weight = (torch.rand(cout, cin, k, k, generator=gen) * 2 - 1) / (cin * k * k) ** 0.5
    bias = torch.randn(cout, generator=gen) if with_bias else None
    ref = F.conv2d(x.double(), weight.double(), None if bias is None else bias.double(), stride=2, padding=pad).numpy()
    bar = 4 * worst(F.conv2d(x, weight, bias, stride=2, padding=pad).numpy(), ref)
    wd = weight.permute(2, 3, 1, 0).contiguous().to(DEV)
    bd = None if bias is None else bias.to(DEV)
    y = hg.conv_s2(cl(x), wd, bd, k, pad)
    assert tuple(y.shape) == ref.shape and torch.equal(y, hg.conv_s2(cl(x), wd, bd, k, pad))
    err = worst(host(y).numpy(), ref)
    print(f"conv {k}x{k}/2 {cin}->{cout} B={b} {h}x{w} bias={with_bias}: err {err:.3g}, torch float32 {bar / 4:.3g}, bar {bar:.3g}")
    assert err <= bar, (err, bar)


# ------------------------------------------------------------------------------------------------ pool, tail
@pytest.mark.parametrize("b,c,h,w", ((1, 64, 2, 2), (2, 128, 16, 8), (1, 256, 2, 4)))
def test_average_pool_is_exact(b, c, h, w):
    """Four floats added in the window's row-major order, times 0.25 (exact): byte-equal to the same float32 steps on the host."""
    from tomosar2height_amd.encoder import hourglass as hg
    x = torch.randn(b, c, h, w, generator=torch.Generator().manual_seed(c + h))
    y = hg.avgpool2x2(cl(x))
    assert tuple(y.shape) == (b, c, h // 2, w // 2) and torch.equal(host(y), hg_ref.avg_pool(x))


@pytest.mark.parametrize("b,c,h,w", ((1, 64, 2, 1), (2, 256, 8, 4), (1, 128, 1, 1)))
def test_block_tail_is_exact(b, c, h, w):
    """One addition per element: byte-equal to torch.cat + the addition on the host."""
    from tomosar2height_amd.encoder import hourglass as hg
    gen = torch.Generator().manual_seed(c + w)
    o1, o2, o3 = (torch.randn(b, n, h, w, generator=gen) for n in (c // 2, c // 4, c // 4))
    res = torch.randn(b, c, h, w, generator=gen)
    y = hg.block_tail(cl(o1), cl(o2), cl(o3), cl(res))
    assert torch.equal(host(y), hg_ref.block_tail(o1, o2, o3, res))


# ------------------------------------------------------------------------------------------------ composed pieces
def host_bar(fn, x):
    """(ref64, 4 x max|float32 - float64|) of a restated piece on the host."""
    r64 = fn(x.double(), torch.float64).numpy()
    return r64, 4 * worst(fn(x, torch.float32).numpy(), r64)


@pytest.mark.parametrize("cin,cout,h,w", ((64, 128, 8, 4), (128, 128, 4, 4)))
@pytest.mark.parametrize("conv_precision", PRECISIONS)
def test_conv_block_with_and_without_downsample(cin, cout, h, w, conv_precision):
    from tomosar2height_amd import grid
    from tomosar2height_amd.encoder.hourglass import ConvBlock
    blk = hg_ref.init_hg_(ConvBlock(cin, cout, norm="group")).to(DEV).eval()
    assert (blk.downsample is None) == (cin == cout)
    x = torch.randn(2, cin, h, w, generator=torch.Generator().manual_seed(cin))
    r64, bar = host_bar(lambda t, dt: hg_ref.block(t, {"b." + k: v for k, v in hg_ref.params_of(blk, dt, "cpu").items()}, "b"), x)
    before = grid.fallback_count()
    with precision(conv_precision), torch.no_grad():
        y = blk(x.to(DEV))
    err = worst(host(y).numpy(), r64)
    print(f"ConvBlock({cin}, {cout}) {conv_precision}: err {err:.3g}, bar {bar:.3g}")
    assert err <= bar and grid.fallback_count() == before


@pytest.mark.parametrize("conv_precision", PRECISIONS)
def test_hourglass_of_depth_two_down_to_one_pixel(conv_precision):
    from tomosar2height_amd import grid
    from tomosar2height_amd.encoder.hourglass import HourGlass
    net = hg_ref.init_hg_(HourGlass(1, 2, 256, "group")).to(DEV).eval()
    x = torch.randn(1, 256, 4, 4, generator=torch.Generator().manual_seed(9))
    r64, bar = host_bar(lambda t, dt: hg_ref.hourglass(t, {"m." + k: v for k, v in hg_ref.params_of(net, dt, "cpu").items()}, "m", 2), x)
    before = grid.fallback_count()
    with precision(conv_precision), torch.no_grad():
        y = net(x.to(DEV))
        with pytest.raises(ValueError, match="powers of two"):
            net(x[:, :, :2, :].to(DEV))                       # 2 x 4: the lowest level would have no pixel
    err = worst(host(y).numpy(), r64)
    print(f"HourGlass(depth 2) on 4 x 4, {conv_precision}: err {err:.3g}, bar {bar:.3g}")
    assert tuple(y.shape) == (1, 256, 4, 4) and err <= bar and grid.fallback_count() == before


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("conv_precision", PRECISIONS)
def test_encoder_within_the_reference_tolerance(name, conv_precision):
    from tomosar2height_amd import grid
    g = golden()
    enc, trace = encoder(name), {}
    before = grid.fallback_count()
    with precision(conv_precision), torch.no_grad():
        trace["out"] = enc(hg_ref.case_image(name).to(DEV), trace=trace)
    assert grid.fallback_count() == before
    assert sorted(trace) == sorted(hg_ref.tensor_names(enc.num_modules))
    ratios = {}
    for key, t in trace.items():
        want, tol = hg_ref.ref64(g, name, key)
        err = worst(host(t).numpy(), want)
        ratios[key] = err / (tol / 4)
        print(f"{name} {conv_precision} {key}: max err {err:.3g}, tolerance {tol:.3g} (4 x ref32_dev), ratio to ref32_dev {ratios[key]:.2f}")
    bad = {k: round(r, 2) for k, r in ratios.items() if r > 4}
    assert not bad, (name, conv_precision, bad)


@pytest.mark.parametrize("conv_precision", PRECISIONS)
def test_full_model_heights_within_the_reference_tolerance(conv_precision):
    from tomosar2height_amd import TomoSAR2Height, grid
    g = golden()
    if "model" not in _cache:
        _cache["model"] = hg_ref.init_hg_(TomoSAR2Height(hg_ref.model_cfg(g))).to(DEV).eval()
    model = _cache["model"]
    pts, image = torch.as_tensor(g["model64_points"]).to(DEV), hg_ref.case_image("model64").to(DEV)
    before = grid.fallback_count()
    with precision(conv_precision), torch.no_grad():
        heights, _ = model(input_cloud=pts, input_image=image)
        out = model.image_encoder(image)
    assert grid.fallback_count() == before
    for key, t in (("out", out), ("heights", heights)):
        want, tol = hg_ref.ref64(g, "model64", key)
        err = worst(host(t).numpy().reshape(want.shape), want)
        print(f"model64 {conv_precision} {key}: max err {err:.3g}, tolerance {tol:.3g} (4 x ref32_dev)")
        assert err <= tol, (key, err, tol)
    fresh = TomoSAR2Height(hg_ref.model_cfg(g))
    fresh.load_state_dict(model.state_dict(), strict=True)


def test_determinism_layouts_modes_and_refusals():
    from tomosar2height_amd import grid
    enc = encoder("g32b2")
    image = hg_ref.case_image("g32b2").to(DEV)
    assert image.is_contiguous()
    before = grid.fallback_count()
    with torch.no_grad():
        a = enc(image)
        b = enc(image)
        c = enc(image.contiguous(memory_format=torch.channels_last))
        d = enc.train()(image)                                     # norm='group' computes the same thing in either mode
        enc.eval()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
        assert tuple(a.shape) == (2, 32, 8, 8) and not a.requires_grad and a.grad_fn is None
        launched = grid.fallback_count()
        with pytest.raises(ValueError, match="powers of two"):
            enc(torch.zeros(1, 3, 48, 64, device=DEV))
        with pytest.raises(ValueError, match="powers of two"):
            enc(torch.zeros(1, 3, 8, 64, device=DEV))              # below 4 * 2 ** num_hourglass
        with pytest.raises(NotImplementedError, match="batch statistics"):
            encoder("bn32").train()(hg_ref.case_image("bn32").to(DEV))
        encoder("bn32").eval()
    assert grid.fallback_count() == before == launched
    with pytest.raises(NotImplementedError, match="inference only"):
        enc(image)                                                 # gradients enabled, trainable parameters
    for p in enc.parameters():
        p.requires_grad_(False)
    try:
        assert torch.equal(enc(image), a)                          # nothing to train: runs with gradients enabled, no graph
    finally:
        for p in enc.parameters():
            p.requires_grad_(True)


def test_folded_batch_norm_follows_the_running_statistics():
    enc = encoder("bn32")
    image = hg_ref.case_image("bn32").to(DEV)
    with torch.no_grad():
        a = enc(image).clone()
        saved = enc.bn_end0.running_mean.clone()
        enc.bn_end0.running_mean.add_(0.05)
        b = enc(image).clone()
        enc.bn_end0.running_mean.copy_(saved)
        c = enc(image)
    assert not torch.equal(a, b) and torch.equal(a, c)
