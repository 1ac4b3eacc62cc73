"""GPU parity at the module seam: the HIP-backed modules (same constructor / forward / state_dict as the
reference) against fixtures captured from the reference itself and against the torch oracle on the CPU.
Tolerance (north_star): fp32 heights within 1e-4 relative."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from detinit import det_init_, synth_cloud

pytestmark = pytest.mark.gpu

REL = 1e-4


def _dev():
    return torch.device("cuda:0")


def _close(got, want, rel=REL, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want).max() / scale
    assert err <= rel, f"{what}: max rel err {err:.3e} > {rel:g}"


def _dsm(lo):
    return torch.from_numpy(lo).repeat_interleave(8, -2).repeat_interleave(8, -1)


def test_local_pool_pointnet_reduced_golden():
    from tomosar2height_amd.encoder.pointnet import LocalPoolPointnet
    g = load_golden("local_pool_pointnet_reduced")
    enc = LocalPoolPointnet(feature_dim=8, dim=3, hidden_dim=8, scatter_type="max", unet_type="alto",
                            unet_kwargs=dict(depth=3, merge_mode="concat", start_filts=8), plane_resolution=16)
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    assert list(sd) == list(enc.state_dict())
    enc.load_state_dict(sd, strict=True)
    enc.to(_dev())
    out = enc(torch.from_numpy(g["cloud"]).to(_dev()))["xy"]
    _close(out.detach().cpu().numpy(), g["out"], what="plane")
    out.backward(torch.from_numpy(g["gout"]).to(_dev()))
    none_grad = [k for k, v in enc.named_parameters() if v.grad is None]
    assert none_grad == g["none_grad"].tolist()
    for k, v in enc.named_parameters():
        if v.grad is not None:
            _close(v.grad.cpu().numpy(), g["g." + k], rel=2e-4, what=k)


def test_local_pool_pointnet_reduced_mean_golden():
    """scatter_type='mean' (pointnet.py:55-56; no shipped config selects it) through the whole reduced encoder."""
    from tomosar2height_amd.encoder.pointnet import LocalPoolPointnet
    g = load_golden("local_pool_pointnet_reduced_mean")
    enc = LocalPoolPointnet(feature_dim=8, dim=3, hidden_dim=8, scatter_type="mean", unet_type="alto",
                            unet_kwargs=dict(depth=3, merge_mode="concat", start_filts=8), plane_resolution=16)
    enc.load_state_dict({k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}, strict=True)
    enc.to(_dev())
    out = enc(torch.from_numpy(g["cloud"]).to(_dev()))["xy"]
    _close(out.detach().cpu().numpy(), g["out"], what="plane")
    out.backward(torch.from_numpy(g["gout"]).to(_dev()))
    assert [k for k, v in enc.named_parameters() if v.grad is None] == g["none_grad"].tolist()
    for k, v in enc.named_parameters():
        if v.grad is not None:
            _close(v.grad.cpu().numpy(), g["g." + k], rel=2e-4, what=k)
    with pytest.raises(ValueError):
        LocalPoolPointnet(scatter_type="median", unet_kwargs=dict(depth=3, start_filts=8), plane_resolution=16)


@pytest.mark.parametrize("channels_last", [True, False])
def test_up_mode_upsample_golden(channels_last):
    """up_mode='upsample' (alto.py:23-35, unet.py; no shipped config selects it) in both U-Nets against the reference's own
    outputs: bilinear x2 (``t2h_upsample2x_nhwc_*``, align_corners=False) + 1x1 convolution on the GEMM kernels."""
    import tomosar2height_amd as t2h
    from tomosar2height_amd.encoder.pointnet import LocalPoolPointnet
    from tomosar2height_amd.encoder.unet import UNet
    t2h.allow_library_fallback(True).set()        # 8-channel planes: the 3x3 convolutions of this reduced model are MIOpen's
    g = load_golden("local_pool_pointnet_reduced_upsample")
    enc = LocalPoolPointnet(feature_dim=8, dim=3, hidden_dim=8, scatter_type="max", unet_type="alto",
                            unet_kwargs=dict(depth=3, merge_mode="concat", start_filts=8, up_mode="upsample"),
                            plane_resolution=16)
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    assert list(sd) == list(enc.state_dict())                     # nn.Sequential names: up_convs.N.upconv.1.weight
    enc.load_state_dict(sd, strict=True)
    enc.to(_dev())
    enc.set_channels_last(channels_last)
    out = enc(torch.from_numpy(g["cloud"]).to(_dev()))["xy"]
    _close(out.detach().cpu().numpy(), g["out"], what="plane")
    out.backward(torch.from_numpy(g["gout"]).to(_dev()))
    assert [k for k, v in enc.named_parameters() if v.grad is None] == g["none_grad"].tolist()
    for k, v in enc.named_parameters():
        if v.grad is not None:
            _close(v.grad.cpu().numpy(), g["g." + k], rel=2e-4, what=k)
    g = load_golden("plain_unet_upsample")
    net = UNet(8, in_channels=4, depth=3, start_filts=8, up_mode="upsample")
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}
    assert list(sd) == list(net.state_dict())
    net.load_state_dict(sd, strict=True)
    net.to(_dev())
    if hasattr(net, "set_channels_last"):
        net.set_channels_last(channels_last)
    x = torch.from_numpy(g["x"]).to(_dev()).requires_grad_(True)
    y = net(x)
    _close(y.detach().cpu().numpy(), g["y"], what="unet out")
    y.backward(torch.from_numpy(g["gy"]).to(_dev()))
    _close(x.grad.cpu().numpy(), g["gx"], rel=2e-4, what="unet gx")
    for k, v in net.named_parameters():
        _close(v.grad.cpu().numpy(), g["g." + k], rel=2e-4, what=k)
    with pytest.raises(ValueError):
        UNet(8, up_mode="upsample", merge_mode="add")


def test_up_mode_upsample_runs_without_library_kernels():
    """16-aligned widths: the whole upsample-mode U-Net (bilinear x2, 1x1 and 3x3 convolutions, pooling) on t2h kernels --
    library fallbacks stay off and none is counted -- against the oracle's PlainUNet with the same weights."""
    import tomosar2height_amd as t2h
    from tomosar2height_amd.encoder.unet import UNet
    from oracle import torch_ref
    net = det_init_(UNet(16, in_channels=4, depth=3, start_filts=16, up_mode="upsample"), seed=11)
    ref = torch_ref.PlainUNet(16, in_channels=4, depth=3, start_filts=16, up_mode="upsample")
    ref.load_state_dict(net.state_dict(), strict=True)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 4, 32, 32, generator=g)
    gy = torch.randn(1, 16, 32, 32, generator=g)
    xr = x.clone().requires_grad_(True)
    want = ref(xr)
    want.backward(gy)
    net.to(_dev())
    net.set_channels_last(True)
    before = sum(t2h.fallback_counts().values())
    xd = x.to(_dev()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    got = net(xd)
    got.backward(gy.to(_dev()))
    assert sum(t2h.fallback_counts().values()) == before
    _close(got.detach().cpu().numpy(), want.detach().numpy(), what="out")
    _close(xd.grad.cpu().numpy(), xr.grad.numpy(), rel=2e-4, what="gx")
    for (k, v), (_, vr) in zip(net.named_parameters(), ref.named_parameters()):
        _close(v.grad.cpu().numpy(), vr.grad.numpy(), rel=2e-4, what=k)


def _hip_module_fixture(g, prefix, mod, inputs, channels_last, rel=2e-4, grad_rel=None):
    sd = {k[len(prefix) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix + ".w.")}
    assert list(sd) == list(mod.state_dict())
    mod.load_state_dict(sd, strict=True)
    mod.to(_dev())
    for m in mod.modules():
        if hasattr(m, "set_channels_last"):
            m.set_channels_last(channels_last)
    args = [torch.from_numpy(g[f"{prefix}.in.{k}"]).to(_dev()).requires_grad_(k.startswith("x")) for k in inputs]
    out = mod(*args)
    out = out["xy"] if isinstance(out, dict) else out
    _close(out.detach().cpu().numpy(), g[prefix + ".out"], what=prefix + " out")
    out.backward(torch.from_numpy(g[prefix + ".gout"]).to(_dev()))
    assert [k for k, v in mod.named_parameters() if v.grad is None] == g[prefix + ".none_grad"].tolist()
    for k, v in mod.named_parameters():
        if v.grad is not None:
            _close(v.grad.cpu().numpy(), g[f"{prefix}.g.{k}"], rel=grad_rel or rel, what=f"{prefix} {k}")
    for k, a in zip(inputs, args):
        if a.grad is not None:
            _close(a.grad.cpu().numpy(), g[f"{prefix}.gin.{k}"], rel=grad_rel or rel, what=f"{prefix} d{k}")


@pytest.mark.parametrize("channels_last", [False, True])
def test_reference_options_golden(channels_last):
    """r06 (VERDICT r05 missing 3 / 4): ``ConvDecoder(leaky=True)`` (pixel.py:8-32), ``unet_type='unet'`` (pointnet.py:45-49) and
    ``merge_mode='add'`` in both U-Nets (alto.py:176-179, 221-224; unet.py:92-105) against the reference's own outputs and
    gradients (tests/golden/reference_options.npz).  Reduced widths (8 channels) are below the convolution kernels' slabs, so the
    library fallback is allowed here; ``test_leaky_decoder_runs_on_the_t2h_kernels`` is the full-width check without it."""
    import tomosar2height_amd as t2h
    from tomosar2height_amd.decoder.pixel import PixelwiseDecoder
    from tomosar2height_amd.encoder.pointnet import LocalPoolPointnet
    from tomosar2height_amd.encoder.unet import UNet
    t2h.allow_library_fallback(True).set()
    g = load_golden("reference_options")

    class _Dec(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.d = PixelwiseDecoder(hidden_dim=32, out_dim=1, output_size=32, mode="conv", leaky=True)

        def forward(self, x):
            return self.d({"xy": x})[0]
    # (leaky slopes keep every gradient path alive: no mask-flip steps, the tight bound holds for the input gradient too)
    _hip_module_fixture(g, "leaky_decoder", _Dec(), ["x"], channels_last)
    _hip_module_fixture(g, "plane_unet", LocalPoolPointnet(feature_dim=8, dim=3, hidden_dim=8, scatter_type="max", unet_type="unet",
                                                            unet_kwargs=dict(depth=3, merge_mode="concat", start_filts=8),
                                                            plane_resolution=16), ["cloud"], channels_last)
    _hip_module_fixture(g, "alto_add", LocalPoolPointnet(feature_dim=8, dim=3, hidden_dim=8, scatter_type="max", unet_type="alto",
                                                          unet_kwargs=dict(depth=3, merge_mode="add", start_filts=8),
                                                          plane_resolution=16), ["cloud"], channels_last)
    _hip_module_fixture(g, "unet_add", UNet(8, in_channels=4, depth=3, start_filts=8, merge_mode="add"), ["x"], channels_last)


def test_leaky_decoder_runs_on_the_t2h_kernels():
    """``ConvDecoder(leaky=True)`` at the shipped widths in channels_last mode: the three 3x3 convolutions and the 288 -> 1 head on
    the t2h kernels (library fallbacks OFF and none counted), F.leaky_relu between them; against the oracle in float64."""
    import tomosar2height_amd as t2h
    from oracle import torch_ref
    from tomosar2height_amd.decoder.pixel import ConvDecoder
    dec = det_init_(ConvDecoder(32, 1, leaky=True), seed=31)
    ref = torch_ref.ConvDecoder(32, 1, leaky=True).double()
    ref.load_state_dict({k: v.double() for k, v in dec.state_dict().items()}, strict=True)
    g = torch.Generator().manual_seed(31)
    x = torch.randn(1, 32, 64, 64, generator=g)
    gy = torch.randn(1, 1, 64, 64, generator=g)
    xr = x.double().requires_grad_(True)
    want = ref(xr)
    want.backward(gy.double())
    dec.to(_dev())
    dec.channels_last = True
    before = sum(t2h.fallback_counts().values())
    xd = x.to(_dev()).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    got = dec(xd)
    got.backward(gy.to(_dev()))
    assert sum(t2h.fallback_counts().values()) == before, "a vendor-library fallback ran"
    _close(got.detach().cpu().numpy(), want.detach().numpy(), rel=2e-5, what="out")
    _close(xd.grad.cpu().numpy(), xr.grad.numpy(), rel=2e-5, what="gx")
    for (k, v), (_, vr) in zip(dec.named_parameters(), ref.named_parameters()):
        _close(v.grad.cpu().numpy(), vr.grad.numpy(), rel=2e-5, what=k)


@pytest.mark.parametrize("mode", ["conv", "fc"])
@pytest.mark.parametrize("foot", [False, True])
@pytest.mark.parametrize("img", [False, True])
def test_pixelwise_decoder_golden(mode, foot, img):
    from tomosar2height_amd.decoder.pixel import PixelwiseDecoder
    g = load_golden("pixelwise_decoder")
    tag = f"{mode}_f{int(foot)}_i{int(img)}"
    import tomosar2height_amd as t2h
    before = sum(t2h.fallback_counts().values())       # r05: the per-pixel FC head's 1-column Linear runs on the head kernels too
    dec = det_init_(PixelwiseDecoder(hidden_dim=32, out_dim=1, output_size=32, mode=mode, use_footprint=foot), seed=7)
    assert list(dec.state_dict()) == g[f"keys_{tag}"].tolist()
    dec.to(_dev())
    planes = {"xy": torch.from_numpy(g[f"xy_{tag}"]).to(_dev()).requires_grad_(True)}
    if img:
        planes["image"] = torch.from_numpy(g[f"image_{tag}"]).to(_dev())
    x, xf = dec(planes)
    _close(x.detach().cpu().numpy(), g[f"x_{tag}"], what="x")
    loss = x.sum()
    if foot:
        _close(xf.detach().cpu().numpy(), g[f"xf_{tag}"], what="xf")
        loss = loss + 0.5 * xf.sum()
    else:
        assert xf is None
    loss.backward()
    # input gradient through three ReLU conv layers (MIOpen): a ReLU mask that flips under 1e-7 differences moves
    # single entries by a finite step (see test_model_vs_torch_oracle_all_grads), hence max-norm 1e-2 + L2 3e-3
    got, want = planes["xy"].grad.cpu().double(), torch.from_numpy(g[f"gxy_{tag}"]).double()
    _close(got.numpy(), want.numpy(), rel=1e-2, what="gxy")
    assert ((got - want).norm() / want.norm()).item() <= 3e-3
    assert sum(t2h.fallback_counts().values()) == before, "a vendor-library fallback ran"
    if mode == "fc":      # Linear(32, 1) head: weight / bias gradients against float64 on the device (the fixture holds gxy only)
        head = dec.fc_decoder
        rows = torch.randn(4096, 32, generator=torch.Generator().manual_seed(3)).to(_dev()).requires_grad_(True)
        up = torch.randn(4096, 1, generator=torch.Generator().manual_seed(4)).to(_dev())
        for p in head.parameters():
            p.grad = None
        head(rows).backward(up)
        r64 = rows.detach().double().requires_grad_(True)
        w64, b64 = head.fc_out.weight.detach().double().requires_grad_(True), head.fc_out.bias.detach().double().requires_grad_(True)
        (torch.relu(r64) @ w64.t() + b64).backward(up.double())
        _close(rows.grad.cpu().numpy(), r64.grad.cpu().numpy(), rel=2e-6, what="fc head dx")
        _close(head.fc_out.weight.grad.cpu().numpy(), w64.grad.cpu().numpy(), rel=2e-6, what="fc head dw")
        _close(head.fc_out.bias.grad.cpu().numpy(), b64.grad.cpu().numpy(), rel=2e-6, what="fc head db")


def _full_model(tag):
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config, munich_config
    cfg = berlin_config() if tag == "berlin" else munich_config(use_image=True)
    return det_init_(TomoSAR2Height(cfg), seed=8).to(_dev()), cfg


@pytest.mark.parametrize("tag", ["berlin", "munich"])
@pytest.mark.parametrize("channels_last", [False, True])
def test_full_model_golden(tag, channels_last):
    """Full-size networks at N=4096 against the reference's own output (fixture 8 of SURVEY 8c)."""
    from tomosar2height_amd.trainer import Trainer
    g = load_golden(f"full_model_{tag}_n4096")
    import tomosar2height_amd as t2h
    t2h.allow_library_fallback(not channels_last).set()        # the NCHW grid side is MIOpen's by definition
    model, cfg = _full_model(tag)
    assert sum(p.numel() for p in model.parameters()) == int(g["n_params"])
    assert list(model.state_dict()) == g["state_keys"].tolist()
    model.set_channels_last(channels_last)
    cloud = torch.from_numpy(g["cloud"]).to(_dev())
    image = None
    if tag == "munich":
        image = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(8)).to(_dev())
    with torch.no_grad():
        pa, pb = model(input_cloud=cloud, input_image=image)
    assert pa.shape == (1, 512, 512, 1)
    _close(pa[0, :, :, 0].cpu().numpy(), g["height"], what="height")
    if tag == "munich":
        _close(pb[0, :, :, 0].cpu().numpy(), g["footprint_logits"], what="footprint logits")
    else:
        assert pb is None
    # loss + gradients through Trainer.train_step semantics
    dsm = _dsm(g["dsm_lo"])
    tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=2,
                 use_cloud=True, use_image=tag == "munich", use_footprint=tag == "munich")
    data = {"inputs": cloud, "dsm": dsm.to(_dev())}
    if image is not None:
        data["image"] = image
    assert tr.train_step(data) is False
    np.testing.assert_allclose(float(tr.accumulated_loss), float(g["loss"]), rtol=1e-4)
    grads = dict(model.named_parameters())
    assert [k for k, v in grads.items() if v.grad is None] == g["none_grad"].tolist()
    # L1's gradient is sign(pa - dsm): pixels with pa ~ dsm flip under 1e-6 height differences, so gradient
    # NORMS under the reference loss are only comparable to ~1e-2; tight gradient parity is checked with a
    # smooth loss in test_model_vs_torch_oracle_all_grads.
    for k, n in zip(g["grad_names"].tolist(), g["grad_norm"]):
        got = grads[k].grad.double().norm().item()
        assert abs(got - n) <= 2e-2 * n + 1e-9, f"{k}: grad norm {got} vs {n}"


def test_model_vs_torch_oracle_all_grads():
    """Same weights, same skewed tile (N=20000): every output pixel and every parameter gradient against the
    CPU torch oracle."""
    from oracle import torch_ref
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    cfg = berlin_config()
    ref = det_init_(torch_ref.TomoSAR2Height(cfg), seed=21)
    model = TomoSAR2Height(cfg)
    model.load_state_dict(ref.state_dict(), strict=True)
    model.to(_dev())
    cloud = synth_cloud(20000, seed=77)
    cloud[0, :3000, :2] = cloud[0, 0, :2]                    # 3000 points in ONE finest cell (facade-like skew)
    # smooth (linear) loss with fixed random weights: the gradient does not depend on sign(pa - dsm)
    w = torch.randn(512, 512, generator=torch.Generator().manual_seed(1))
    pa_ref, _ = ref(input_cloud=cloud)
    loss_ref = (pa_ref.squeeze() * w).mean()
    loss_ref.backward()
    pa_ref = pa_ref.detach()
    pa, _ = model(input_cloud=cloud.to(_dev()))
    loss = (pa.squeeze() * w.to(_dev())).mean()
    loss.backward()
    _close(pa.detach().cpu().numpy(), pa_ref.numpy(), what="height")
    np.testing.assert_allclose(loss.item(), loss_ref.item(), rtol=1e-4, atol=1e-5)
    # Gradients of a ReLU/max-pool network are piecewise constant in the activations: a mask that flips under
    # a 1e-7 activation difference moves a gradient entry by a finite step.  The torch oracle itself, run on
    # this GPU instead of the CPU, deviates from its CPU run by up to ~6e-3 (max-normalised) on the same inputs
    # (measured), so that is the resolution of this check: 1e-2 max-normalised, 3e-3 in L2.
    ref_gpu = det_init_(torch_ref.TomoSAR2Height(cfg), seed=21).to(_dev())
    pg, _ = ref_gpu(input_cloud=cloud.to(_dev()))
    (pg.squeeze() * w.to(_dev())).mean().backward()
    for (k, p), (_, q), (_, r) in zip(model.named_parameters(), ref.named_parameters(), ref_gpu.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is None:
            continue
        got, want, want_gpu = p.grad.cpu().double(), q.grad.double(), r.grad.cpu().double()
        _close(got.numpy(), want.numpy(), rel=1e-2, what=k)
        l2 = ((got - want).norm() / (want.norm() + 1e-30)).item()
        l2_gpu = ((got - want_gpu).norm() / (want_gpu.norm() + 1e-30)).item()
        assert l2 <= 3e-3, f"{k}: L2 rel err vs CPU oracle {l2:.2e}"
        assert l2_gpu <= 3e-3, f"{k}: L2 rel err vs the oracle run on the device {l2_gpu:.2e}"


def test_trainer_accumulation_golden():
    """trainer.py:47-89: 3 tiles summed, one AdamW step -- post-step weights of the reference's own Trainer."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    g = load_golden("trainer_accumulation")
    cfg = berlin_config()
    import tomosar2height_amd as t2h
    t2h.allow_library_fallback(True).set()             # reduced widths (start_filts = 8): below the kernels' 16-channel slabs
    cfg.model.encoder_kwargs.plane_resolution = 16
    cfg.model.encoder_kwargs.unet_kwargs.depth = 3
    cfg.model.encoder_kwargs.unet_kwargs.start_filts = 8
    model = det_init_(TomoSAR2Height(cfg), seed=9).to(_dev())
    tr = Trainer(model, torch.optim.AdamW(model.parameters(), lr=1e-4), device=_dev(), optimize_every=3, use_cloud=True)
    stepped = [tr.train_step({"inputs": torch.from_numpy(g[f"cloud_{t}"]), "dsm": _dsm(g[f"dsm_lo_{t}"])[None]})
               for t in range(3)]
    assert stepped == [False, False, True]
    np.testing.assert_allclose(float(tr.last_avg_loss), float(g["last_avg_loss"]), rtol=1e-5)
    params = dict(model.named_parameters())
    for k in g.files:
        if k.startswith("after."):
            name = k[len("after."):]
            np.testing.assert_allclose(params[name].detach().cpu().numpy(), g[k], rtol=1e-4, atol=2e-6)
    # grads were zeroed for the next accumulation window; never-used parameters still have no grad
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in model.parameters())
    assert sum(p.grad is None for p in model.parameters()) == 8


def test_full_size_properties():
    """BASELINE.json config 2 (N = 131072): size-independent properties -- run-to-run determinism (no atomics
    on the path) and invariance to the order of the input points (the network is a set function of the cloud)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.synthetic import berlin_tile
    model = det_init_(TomoSAR2Height(berlin_config()), seed=3).to(_dev())
    tile = berlin_tile(5)
    cloud = tile["inputs"].to(_dev())
    with torch.no_grad():
        h1, _ = model(input_cloud=cloud)
        h2, _ = model(input_cloud=cloud)
        perm = torch.randperm(cloud.shape[1], generator=torch.Generator().manual_seed(0)).to(_dev())
        h3, _ = model(input_cloud=cloud[:, perm].contiguous())
    assert torch.isfinite(h1).all()
    assert torch.equal(h1, h2), "two runs on the same tile differ: a nondeterministic reduction crept in"
    _close(h3.cpu().numpy(), h1.cpu().numpy(), what="point-order invariance")


def test_full_size_backward_is_exactly_linear_in_the_upstream_gradient():
    """BASELINE.json config 2 (N = 131072), whole backward: the gradient of sum(h * 2w) is bit for bit twice the gradient of
    sum(h * w) -- doubling commutes with every rounding on the path (products, sums, the fixed-order reductions, the
    transposed-matrix sample backward, the fused trunk), so any race, stale workspace or uninitialised read breaks it --
    and a repeated backward reproduces the first."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.synthetic import berlin_tile
    model = det_init_(TomoSAR2Height(berlin_config()), seed=3).to(_dev())
    model.set_channels_last(True)
    cloud = berlin_tile(6)["inputs"].to(_dev())
    w = torch.randn(1, 512, 512, 1, generator=torch.Generator().manual_seed(1)).to(_dev())

    def grads(scale):
        model.zero_grad(set_to_none=True)
        h, _ = model(input_cloud=cloud)
        (h * (w * scale)).sum().backward()
        return {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}

    g1, g2, g1b = grads(1.0), grads(2.0), grads(1.0)
    assert len(g1) > 100
    for k in g1:
        assert torch.isfinite(g1[k]).all(), k
        assert torch.equal(g1[k], g1b[k]), f"{k}: two identical backwards differ"
        assert torch.equal(g2[k], 2.0 * g1[k]), f"{k}: backward is not linear in the upstream gradient"


def test_direct_grad_accumulation_matches_autograd():
    """From the second optimizer window on, Trainer lets the wgrad kernels accumulate straight into the flat
    gradient bucket; the accumulated gradients must equal plain autograd accumulation."""
    from tomosar2height_amd import TomoSAR2Height, mlp
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.plane_resolution = 32
    cfg.model.encoder_kwargs.unet_kwargs.depth = 3
    tiles = [{"inputs": synth_cloud(3000, seed=300 + i), "dsm": torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30}
             for i in range(4)]
    model = det_init_(TomoSAR2Height(cfg), seed=11).to(_dev())
    tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=2, use_cloud=True)
    tr.coalesce_tiles = 1                # (tile by tile: the comparison below is with per-tile autograd at 1e-5)
    assert tr.train_step(tiles[0]) is False and tr.train_step(tiles[1]) is True       # tile 0 builds the bucket
    assert tr.bucket is not None
    tr.train_step(tiles[2])
    tr.accumulated_steps = 0                                                          # keep accumulating, no step
    tr.train_step(tiles[3])
    tr.flush_gradients()                 # (the composed maps' share of the gradients: back-propagated once per window)
    got = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    ref = det_init_(TomoSAR2Height(cfg), seed=11).to(_dev())
    for t in tiles[2:]:
        pa, _ = ref(input_cloud=t["inputs"].to(_dev()))
        torch.nn.functional.l1_loss(pa.squeeze(), t["dsm"].squeeze().to(_dev())).backward()
    for k, p in ref.named_parameters():
        if p.grad is None:
            assert k not in got
            continue
        _close(got[k].cpu().numpy(), p.grad.cpu().numpy(), rel=1e-5, what=k)


def test_config3_cloud_image_bf16_mlp():
    """BASELINE.json configs[2]: Berlin cloud+image with bf16 MLP GEMMs on MFMA (fp32 accumulate, fp32 tensors).
    Tolerance for this mode, stated here: heights within 2e-2 of the fp32 reference fixture scale (bf16 has 8
    significant bits; measured ~3e-3), gradients not compared bit-wise.  fp32 mode on the same weights stays 1e-4."""
    from tomosar2height_amd import TomoSAR2Height, mlp
    from tomosar2height_amd.config import berlin_config
    from oracle import torch_ref
    cfg = berlin_config(use_image=True)
    ref = det_init_(torch_ref.TomoSAR2Height(cfg), seed=13)
    model = TomoSAR2Height(cfg)
    model.load_state_dict(ref.state_dict(), strict=True)
    model.to(_dev())
    cloud = synth_cloud(6000, seed=5)
    image = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want, _ = ref(input_cloud=cloud, input_image=image)
        fp32, _ = model(input_cloud=cloud.to(_dev()), input_image=image.to(_dev()))
    _close(fp32.cpu().numpy(), want.numpy(), what="fp32 height")
    model.set_mlp_precision("bf16")                    # per-point GEMMs and 3x3 convolutions (grid.set_conv_precision)
    try:
        pa, _ = model(input_cloud=cloud.to(_dev()), input_image=image.to(_dev()))
        loss = pa.abs().mean()
        loss.backward()
        _close(pa.detach().cpu().numpy(), want.numpy(), rel=2e-2, what="bf16 height")
        err = (pa.detach().cpu() - want).abs().max() / want.abs().max()
        assert err > 1e-5, "bf16 mode produced fp32-identical output: the flag is not reaching the kernels"
        assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    finally:
        model.set_mlp_precision("fp32")


def test_hip_graph_replay_matches_eager():
    """Trainer.capture_graph: the replayed step must leave exactly the same accumulated gradients and losses as eager
    steps on the same tiles (different tile contents, same shapes)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.plane_resolution = 64
    cfg.model.encoder_kwargs.unet_kwargs.depth = 3
    tiles = [{"inputs": synth_cloud(5000, seed=500 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(4)]

    def run(use_graph):
        model = det_init_(TomoSAR2Height(cfg), seed=12).to(_dev())
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=100, use_cloud=True)
        tr.train_step(tiles[0])
        if use_graph:
            tr.capture_graph(tiles[1])
        for t in tiles[1:]:
            tr.train_step(t)
        tr.flush_gradients()
        return tr.bucket.flat.clone(), float(tr.accumulated_loss)

    g_eager, l_eager = run(False)
    g_graph, l_graph = run(True)
    assert l_eager == l_graph
    # the t2h kernels are deterministic, MIOpen's conv weight-gradient kernels are not (split-K atomics), so the
    # accumulated gradients agree to rounding rather than bit for bit
    scale = g_eager.abs().max().item()
    assert (g_eager - g_graph).abs().max().item() <= 1e-5 * scale


@pytest.mark.parametrize("coalesce", [1, 4])
def test_training_step_is_bit_reproducible(coalesce):
    """channels_last mode: every kernel of the tile step (point<->grid, GEMMs, grid convolutions, reductions) sums in a
    fixed order and nothing uses float atomics, so repeated runs -- eager or replayed from a hipGraph -- leave bit-identical
    accumulated gradients and losses.  coalesce = 4 (r06, the Trainer's default): the same for windows issued as ragged
    micro-batches (the hipGraph replay is per tile: compared in the tile-by-tile form only)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    tiles = [{"inputs": synth_cloud(20000 + 700 * i, seed=600 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())}
             for i in range(3 if coalesce == 1 else 7)]
    if coalesce == 1:
        for t in tiles[1:]:
            t["inputs"] = t["inputs"][:, :20000].contiguous()      # (one shape for the captured graph)

    def run(use_graph):
        model = det_init_(TomoSAR2Height(cfg), seed=21).to(_dev())
        model.set_channels_last(True)
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=100, use_cloud=True)
        tr.coalesce_tiles = coalesce
        tr.train_step(tiles[0])
        if use_graph:
            tr.capture_graph(tiles[1])
        for t in tiles[1:]:
            tr.train_step(t)
        tr.flush_gradients()
        torch.cuda.synchronize()
        return tr.bucket.flat.clone(), float(tr.accumulated_loss)

    g1, l1 = run(False)
    g2, l2 = run(False)
    assert l1 == l2 and torch.equal(g1, g2)
    if coalesce == 1:
        g3, l3 = run(True)
        assert l1 == l3 and torch.equal(g1, g3)


def test_batched_training_step_equals_mean_of_single_tile_steps():
    """B = 2 tiles in one forward/backward (cell ids offset per tile, image borders inside the convolution row tiles):
    the L1(mean) loss gradient equals the average of the two single-tile gradients (channels_last / HIP convolutions)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    model = det_init_(TomoSAR2Height(cfg), seed=31).to(_dev())
    model.set_channels_last(True)
    clouds = torch.cat([synth_cloud(6000, seed=810 + i) for i in range(2)], 0).to(_dev())
    dsm = (torch.rand(2, 512, 512, generator=torch.Generator().manual_seed(8)) * 30).to(_dev())

    def grads(cloud, target):
        model.zero_grad(set_to_none=True)
        pa, _ = model(input_cloud=cloud)
        torch.nn.functional.smooth_l1_loss(pa.squeeze(-1), target).backward()
        return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}

    both = grads(clouds, dsm)
    one = [grads(clouds[i:i + 1].contiguous(), dsm[i:i + 1]) for i in range(2)]
    assert both.keys() == one[0].keys()
    num = den = 0.0
    for k in both:
        want = 0.5 * (one[0][k] + one[1][k])
        num += (both[k] - want).double().pow(2).sum().item()
        den += want.double().pow(2).sum().item()
        assert (both[k] - want).abs().max().item() <= 2e-3 * (want.abs().max().item() + 1e-12), k
    assert num <= (1e-4 ** 2) * den


def test_hipgraph_captured_inference_forward_is_bit_identical():
    """BASELINE configs[4]: the Munich forward captured once into a hipGraph and replayed on other tiles (copied into the
    static inputs) returns exactly the eager heights and footprint logits."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import munich_config
    model = det_init_(TomoSAR2Height(munich_config(use_image=True)), seed=6).to(_dev()).eval()
    clouds = [synth_cloud(6000, seed=90 + i).to(_dev()) for i in range(3)]
    images = [torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(i)).to(_dev()) for i in range(3)]
    static_cloud, static_image = clouds[0].clone(), images[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        model(input_cloud=static_cloud, input_image=static_image)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        pa_s, pb_s = model(input_cloud=static_cloud, input_image=static_image)
    for cloud, image in zip(clouds, images):
        static_cloud.copy_(cloud)
        static_image.copy_(image)
        graph.replay()
        with torch.no_grad():
            pa, pb = model(input_cloud=cloud, input_image=image)
        assert torch.equal(pa, pa_s) and torch.equal(pb, pb_s)


def test_batched_tiles_equal_single_tiles():
    """BASELINE configs[4] (large-batch inference): B tiles of equal N in one forward (cell ids offset by b*R^2) give the
    same heights as B single-tile forwards, for Munich (depth 6, footprint head, image encoder)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import munich_config
    model = det_init_(TomoSAR2Height(munich_config(use_image=True)), seed=5).to(_dev()).eval()
    model.set_channels_last(True)
    clouds = torch.cat([synth_cloud(5000, seed=70 + i) for i in range(3)], 0).to(_dev())
    images = torch.randn(3, 3, 512, 512, generator=torch.Generator().manual_seed(3)).to(_dev())
    with torch.no_grad():
        pa, pb = model(input_cloud=clouds, input_image=images)
        assert pa.shape == (3, 512, 512, 1) and pb.shape == (3, 512, 512, 1)
        for i in range(3):
            qa, qb = model(input_cloud=clouds[i:i + 1].contiguous(), input_image=images[i:i + 1].contiguous())
            _close(pa[i].cpu().numpy(), qa[0].cpu().numpy(), rel=2e-5, what=f"height tile {i}")
            _close(pb[i].cpu().numpy(), qb[0].cpu().numpy(), rel=2e-5, what=f"footprint tile {i}")


def test_training_reduces_loss_over_optimizer_steps():
    """End-to-end guard for the flat gradient bucket + direct wgrad accumulation + AdamW path: overfitting two tiles for
    25 optimizer steps (2 tiles each) must cut the L1 loss substantially and keep everything finite."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.synthetic import berlin_tile
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    torch.manual_seed(0)
    model = TomoSAR2Height(cfg).to(_dev())
    model.set_channels_last(True)
    tr = Trainer(model, torch.optim.AdamW(model.parameters(), lr=5e-4), device=_dev(), optimize_every=2, use_cloud=True)
    tiles = []
    for i in range(2):
        t = berlin_tile(80 + i, n_points=8192)
        tiles.append({"inputs": t["inputs"].to(_dev()), "dsm": t["dsm"].to(_dev())})
    history = []
    for it in range(25):
        for t in tiles:
            stepped = tr.train_step(t)
        assert stepped
        history.append(float(tr.last_avg_loss))
    assert all(np.isfinite(history))
    assert history[-1] < 0.7 * history[0], history
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_side_stream_wgrad_overlap_gives_identical_gradients():
    """Trainer issues the accumulating weight-gradient GEMMs on a side stream, joined at the end of each train_step.
    MIOpen's conv backward uses split-K atomics, so upstream gradients differ in the last bits from run to run: the
    accumulated gradients must agree to rounding (a lost or raced accumulation would be off by a whole tile)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    tiles = [{"inputs": synth_cloud(20000, seed=900 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(5)]

    def run(overlap):
        model = det_init_(TomoSAR2Height(cfg), seed=14).to(_dev())
        model.set_channels_last(True)
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=5, use_cloud=True)
        tr.overlap_wgrad = overlap
        for t in tiles[:-1]:
            assert tr.train_step(t) is False
        tr.flush_gradients()
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        assert (tr._side is not None) == overlap
        return grads

    a, b = run(False), run(True)
    linear = [k for k in a if ".fc_" in k or "fc_comm" in k or k.endswith("shortcut.weight")]
    assert len(linear) > 40
    for k in a:
        scale = a[k].abs().max().item() + 1e-12
        assert (a[k] - b[k]).abs().max().item() <= 1e-4 * scale, k


def test_pipelined_tiles_give_identical_gradients():
    """``Trainer.pipeline_tiles``: tile i + 1's forward is issued before tile i's backward, each tile on its own stream of a
    ping-pong pair.  Same kernels and the same accumulation order per buffer as one tile after the other: the accumulated
    gradients, the loss accumulator and the weights after the optimizer step are identical bit for bit -- also across an
    optimizer boundary (the next window's forward waits for the new weights)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    tiles = [{"inputs": synth_cloud(20000, seed=300 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(7)]

    def run(pipelined):
        model = det_init_(TomoSAR2Height(cfg), seed=15).to(_dev())
        model.set_channels_last(True)
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=1e-3), device=_dev(), optimize_every=4, use_cloud=True)
        tr.pipeline_tiles = pipelined
        ended = [tr.train_step(t) for t in tiles]                 # 4 tiles + optimizer step, then 3 tiles of the next window
        assert ended == [False, False, False, True, False, False, False]
        tr.flush_pipeline()
        tr.flush_gradients()
        torch.cuda.synchronize()
        assert (tr._tile_streams is not None) == pipelined
        return ({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                {k: p.detach().clone() for k, p in model.named_parameters()}, float(tr.accumulated_loss), float(tr.last_avg_loss))

    (ga, wa, la, lavg_a), (gb, wb, lb, lavg_b) = run(False), run(True)
    assert la == lb and lavg_a == lavg_b
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k


@pytest.mark.parametrize("feed", ["fresh", "prepared", "producer"])
def test_pipelined_tiles_whose_inputs_the_caller_drops_at_once(feed):
    """The tile pipeline reads a tile's inputs on ITS streams until the end of its backward -- one ``train_step`` call after
    the caller may have dropped them.  Here every tile is a FRESH device allocation (copied from the host / built ahead by
    ``Trainer.prepare`` on a side stream / produced by ``producer.TileSource`` with prefetch on a side stream), dropped right
    after ``train_step`` returns, and the caller's (and the producer's) stream then re-allocates blocks of the same sizes and
    fills them with NaN.  The trainer holds the inputs until their backward has completed (``Trainer._hold_inputs``): gradients,
    losses and weights equal the sequential run's bit for bit -- a recycled block would show up as NaN."""
    import numpy as np_
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    dev = _dev()
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    n_tiles = 7
    host = [{"inputs": synth_cloud(20000, seed=600 + i),
             "dsm": torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30} for i in range(n_tiles)]
    if feed == "producer":
        from tomosar2height_amd.producer import RasterPatcher, TileProducer
        from tomosar2height_amd.synthetic import berlin_chunk
        ch = berlin_chunk(seed=5, tiles_per_side=2, n_points=20000)
        chunk = (TileProducer(ch["points"].to(dev), z_bound=ch["z_bound"]), RasterPatcher(ch["dsm"].to(dev), ch["left"], ch["top"]))
        anchors = np_.floor(np_.random.RandomState(3).uniform(0, 512.0, (n_tiles, 2))) + np_.array([ch["left"], ch["bottom"]])

    def churn(shapes, streams):
        for st in streams:
            with torch.cuda.stream(st):
                junk = [torch.full(shp, float("nan"), device=dev) for shp in shapes for _ in range(2)]
                del junk

    def run(pipelined):
        model = det_init_(TomoSAR2Height(cfg), seed=17).to(dev)
        model.set_channels_last(True)
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=1e-3), device=dev, optimize_every=4, use_cloud=True)
        tr.pipeline_tiles = pipelined
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        source = None
        if feed == "producer":
            from tomosar2height_amd.producer import TileSource
            source = TileSource(*chunk, flip_augm=True, rotate_augm=True, rng=np_.random.RandomState(9), stream=side)
            ahead = source.get(anchors[0], defer_wait=True)
        elif feed == "prepared":
            ahead = tr.prepare({k: v.to(dev) for k, v in host[0].items()}, side)
        ended = []
        for i in range(n_tiles):
            if feed == "fresh":
                data = {k: v.to(dev) for k, v in host[i].items()}
            else:
                data = ahead                                      # produced / indexed while the previous step ran
                if i + 1 < n_tiles:
                    ahead = (source.get(anchors[i + 1], defer_wait=True) if source is not None
                             else tr.prepare({k: v.to(dev) for k, v in host[i + 1].items()}, side))
                if source is not None:
                    source.wait(data)
            n_i = data["inputs"].n_points if hasattr(data["inputs"], "n_points") else data["inputs"].shape[1]
            ended.append(tr.train_step(data))
            del data                                              # the caller's last reference
            churn([(1, n_i, 3), (n_i, 3), (n_i,), (1, 512, 512), (65537,)], [main, side])
        assert ended == [False, False, False, True, False, False, False]
        tr.flush_gradients()
        torch.cuda.synchronize()
        assert all(ev.query() for ev, _ in tr._held)
        return ({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                {k: p.detach().clone() for k, p in model.named_parameters()}, float(tr.accumulated_loss), float(tr.last_avg_loss))

    (ga, wa, la, lavg_a), (gb, wb, lb, lavg_b) = run(False), run(True)
    assert np.isfinite(la) and np.isfinite(lavg_a)
    assert la == lb and lavg_a == lavg_b
    for k in ga:
        assert torch.isfinite(gb[k]).all(), k
        assert torch.equal(ga[k], gb[k]), k
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k


def test_pipelined_tiles_as_hipgraphs_give_identical_gradients():
    """``Trainer.capture_pipeline_graphs``: the tile pipeline with one forward and one backward hipGraph per tile stream.  Replays
    run the kernels the eager pipeline launches, in the same order per buffer: accumulated gradients, loss accumulator and the
    weights after an optimizer step are identical bit for bit to the eager pipeline; a tile of another shape falls back to eager."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    tiles = [{"inputs": synth_cloud(20000, seed=400 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(7)]
    odd = {"inputs": synth_cloud(15000, seed=499).to(_dev()), "dsm": tiles[0]["dsm"]}

    def run(graphs):
        model = det_init_(TomoSAR2Height(cfg), seed=16).to(_dev())
        model.set_channels_last(True)
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=1e-3), device=_dev(), optimize_every=5, use_cloud=True)
        tr.pipeline_tiles = True
        tr.coalesce_tiles = 1                                       # (the graphs are per tile)
        tr.overlap_wgrad = tr.overlap_conv_wgrad = False            # (the graphs keep the weight gradients on the tile's stream)
        assert tr.train_step(tiles[0]) is False                     # eager: lays out the bucket
        if graphs:
            tr.capture_pipeline_graphs(tiles[1])
        ended = [tr.train_step(t) for t in tiles[1:]] + [tr.train_step(odd)]
        assert ended == [False, False, False, True, False, False, False]
        tr.flush_gradients()
        torch.cuda.synchronize()
        return ({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                {k: p.detach().clone() for k, p in model.named_parameters()}, float(tr.accumulated_loss), float(tr.last_avg_loss))

    (ga, wa, la, lavg_a), (gb, wb, lb, lavg_b) = run(False), run(True)
    assert la == lb and lavg_a == lavg_b
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k


@pytest.mark.parametrize("form", ["capture_graph", "capture_pipeline_graphs"])
def test_capture_leaves_the_accumulators_as_they_were(form):
    """Both capture forms run two warm-up steps and the captured one on the live gradient bucket, loss accumulators and compose
    cache, and promise to leave them as they found them: bit for bit, so no tolerance."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.plane_resolution = 64
    cfg.model.encoder_kwargs.unet_kwargs.depth = 3
    tiles = [{"inputs": synth_cloud(5000, seed=500 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(3)]
    model = det_init_(TomoSAR2Height(cfg), seed=12).to(_dev())
    tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=100, use_cloud=True)
    tr.coalesce_tiles = 1
    if form == "capture_pipeline_graphs":
        tr.pipeline_tiles = True
        tr.overlap_wgrad = tr.overlap_conv_wgrad = False            # (the graphs keep the weight gradients on the tile's stream)
    tr.train_step(tiles[0])
    tr.train_step(tiles[1])
    tr.flush_gradients()

    def cache_tensors():
        return [t for level in tr.compose_cache.snapshot()[0] for t in level] if tr.compose_cache is not None else []

    grads, loss, steps, cache = tr.bucket.flat.clone(), float(tr.accumulated_loss), tr.accumulated_steps, cache_tensors()
    assert steps == 2 and loss > 0 and grads.abs().max().item() > 0     # (something is there to be polluted)
    getattr(tr, form)(tiles[2])
    torch.cuda.synchronize()
    assert torch.equal(tr.bucket.flat, grads)
    assert float(tr.accumulated_loss) == loss and tr.accumulated_steps == steps
    after = cache_tensors()
    assert len(after) == len(cache) and all(torch.equal(a, b) for a, b in zip(after, cache))


def test_tile_index_built_ahead_on_a_side_stream_gives_the_same_step():
    """``Trainer.prepare`` builds the next tile's index (cell sort, sampling adjoint, cell counts) on a side stream while the
    current step runs; the step on the prebuilt index is the step on the raw cloud, bit for bit (same kernels, same order)."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.tile import TileIndex
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    tiles = [{"inputs": synth_cloud(40000, seed=700 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(4)]

    def run(ahead):
        model = det_init_(TomoSAR2Height(cfg), seed=15).to(_dev())
        model.set_channels_last(True)
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=100, use_cloud=True)
        tr.coalesce_tiles = 1                     # (a prebuilt index is per tile: both runs go tile by tile)
        side = torch.cuda.Stream() if ahead else None
        nxt = tr.prepare(tiles[0], side) if ahead else tiles[0]
        for i in range(len(tiles)):
            cur = nxt
            if i + 1 < len(tiles):
                nxt = tr.prepare(tiles[i + 1], side) if ahead else tiles[i + 1]       # issued before step i
            assert isinstance(cur["inputs"], TileIndex) == ahead
            tr.train_step(cur)
        tr.flush_gradients()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, float(tr.accumulated_loss)

    (a, la), (b, lb) = run(False), run(True)
    assert la == lb
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_compose_cache_gives_the_same_accumulated_gradients():
    """Trainer's ComposeCache: the composed weight maps of the deferred ALTO levels computed once per optimizer step and their
    gradient back-propagated once on the sum over the step's tiles == composing and back-propagating per tile (the chain is
    linear in its gradient): same losses bit for bit (same forward values), every gradient to fp32 re-association, and the
    optimizer step sees the complete gradient."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    tiles = [{"inputs": synth_cloud(40000, seed=800 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(3)]

    def run(cached):
        model = det_init_(TomoSAR2Height(cfg), seed=16).to(_dev())
        model.set_channels_last(True)
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=100, use_cloud=True)
        if not cached:
            tr.compose_cache = model.point_encoder.unet.compose_cache = None
        else:
            assert tr.compose_cache is not None
        for t in tiles:
            tr.train_step(t)
        if cached:
            assert len(tr.compose_cache.levels) >= 2, "the tile should be dense enough for deferred levels"
        tr.flush_gradients()
        torch.cuda.synchronize()
        seen = []
        tr.on_reduced = lambda flat: seen.append(flat.clone())
        grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        loss = float(tr.accumulated_loss)
        tr.optimizer_boundary()
        assert torch.equal(seen[0], torch.cat([g.reshape(-1) for g in [seen[0]]]))
        return grads, loss, seen[0]

    (a, la, fa), (b, lb, fb) = run(False), run(True)
    assert la == lb
    assert a.keys() == b.keys()
    for k in a:
        scale = a[k].abs().max().item() + 1e-20
        assert (a[k] - b[k]).abs().max().item() <= 2e-5 * scale, k
    assert (fa - fb).abs().max().item() <= 2e-5 * fa.abs().max().item()


def _cache_setup(n_tiles=2, seed=16):
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    cfg = berlin_config()
    tiles = [{"inputs": synth_cloud(40000, seed=820 + i).to(_dev()),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(_dev())} for i in range(n_tiles)]
    model = det_init_(TomoSAR2Height(cfg), seed=seed).to(_dev())
    model.set_channels_last(True)
    return cfg, model, tiles


def test_compose_cache_is_owned_by_its_trainer():
    """the ComposeCache is visible to the network only inside its own Trainer's step.  (a) a second Trainer
    on the same model (what bench.check_dp builds) neither steals nor loses gradients: both see the complete accumulated
    gradient of their own tiles; (b) a plain ``model(...).backward()`` after a Trainer exists runs plain autograd and leaves
    complete ``.grad`` (compared with a model no Trainer ever touched)."""
    from tomosar2height_amd.trainer import Trainer
    cfg, model, tiles = _cache_setup()
    unet = model.point_encoder.unet
    null = torch.optim.SGD(model.parameters(), lr=0.0)
    seen = {}
    a = Trainer(model, null, device=_dev(), optimize_every=2, use_cloud=True)
    a.on_reduced = lambda flat: seen.__setitem__("a", flat.clone())
    b = Trainer(model, null, device=_dev(), optimize_every=2, use_cloud=True)        # created while a is alive: must not disturb a
    b.on_reduced = lambda flat: seen.__setitem__("b", flat.clone())
    assert a.compose_cache is not None and b.compose_cache is not None and a.compose_cache is not b.compose_cache
    assert getattr(unet, "compose_cache", None) is None
    for t in tiles:
        a.train_step(t)
        assert getattr(unet, "compose_cache", None) is None, "the cache must not stay on the module between steps"
    assert len(a.compose_cache.levels) >= 2 and not a.compose_cache.pending
    for t in tiles:
        b.train_step(t)
    assert (seen["a"] - seen["b"]).abs().max().item() <= 2e-5 * seen["a"].abs().max().item()

    # (b) plain autograd on the same model, compared with a model that never saw a Trainer
    _, fresh, _ = _cache_setup()
    for m in (model, fresh):
        m.zero_grad(set_to_none=True)
        pa, _ = m(input_cloud=tiles[0]["inputs"])
        torch.nn.functional.l1_loss(pa.squeeze(), tiles[0]["dsm"].squeeze()).backward()
    for (k, p), (_, q) in zip(model.named_parameters(), fresh.named_parameters()):
        assert (p.grad is None) == (q.grad is None), k
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), k
    assert not a.compose_cache.pending and not b.compose_cache.pending


@pytest.mark.parametrize("fused", [False, True], ids=["torch_adamw", "flat_adamw"])
def test_optimizer_stepped_outside_the_trainer_is_noticed(fused):
    """an optimizer step issued by the CALLER on a model with a live ComposeCache.  With gradients pending in the
    cache the next train_step raises (the maps they belong to are gone); with nothing pending the maps are recomputed from the
    new weights (both optimizers bump the parameters' version counters -- FlatAdamW writes through raw pointers and bumps them
    explicitly): the next step equals that of a cache-less trainer on the same weights."""
    from tomosar2height_amd.optim import FlatAdamW
    from tomosar2height_amd.trainer import Trainer
    cfg, model, tiles = _cache_setup()
    opt = (FlatAdamW if fused else torch.optim.AdamW)(model.parameters(), lr=1e-3)
    tr = Trainer(model, opt, device=_dev(), optimize_every=100, use_cloud=True)
    tr.train_step(tiles[0])                                # (the very first tile flushes at once: the bucket is laid out from it)
    tr.train_step(tiles[1])
    # (coalescing: tile 1 has been accepted, not issued; without it -- tile pipeline: its backward has not been issued)
    assert tr.compose_cache.pending or tr._pending is not None or tr._coalesced
    opt.step()                                             # the misuse: tile 1 is still held / its gradients are in the cache / the pipeline
    with pytest.raises(RuntimeError, match="unflushed"):
        for t in (tiles[0], tiles[1], tiles[0]):          # (the third held tile fills the micro-batch: issued at the latest here)
            tr.train_step(t)
    for co in (1,):                                        # the same misuse with every tile issued by its own call (r05 form)
        cfg, model, tiles = _cache_setup()
        opt = (FlatAdamW if fused else torch.optim.AdamW)(model.parameters(), lr=1e-3)
        tr = Trainer(model, opt, device=_dev(), optimize_every=100, use_cloud=True)
        tr.coalesce_tiles = co
        tr.train_step(tiles[0])
        tr.train_step(tiles[1])
        assert tr.compose_cache.pending or tr._pending is not None
        opt.step()
        with pytest.raises(RuntimeError, match="unflushed"):
            tr.train_step(tiles[0])

    cfg, model, tiles = _cache_setup()
    opt = (FlatAdamW if fused else torch.optim.AdamW)(model.parameters(), lr=1e-3)
    tr = Trainer(model, opt, device=_dev(), optimize_every=100, use_cloud=True)
    tr.train_step(tiles[0])
    tr.flush_gradients()
    opt.step()                                             # legal: nothing pending; the trainer was not told
    tr.bucket.zero_()
    tr.train_step(tiles[1])
    tr.flush_gradients()
    got = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=False)
    pa, _ = model(input_cloud=tiles[1]["inputs"])           # plain autograd on the stepped weights
    torch.nn.functional.l1_loss(pa.squeeze(), tiles[1]["dsm"].squeeze()).backward()
    for k, p in model.named_parameters():
        if p.grad is not None:
            scale = p.grad.abs().max().item() + 1e-20
            assert (got[k] - p.grad).abs().max().item() <= 2e-5 * scale, k


@pytest.mark.parametrize("pipelined", [True, False])
def test_out_of_domain_points_are_raised_at_the_optimizer_boundary_without_draining_the_queue(pipelined):
    """``Trainer(check_domain=True)`` (default): a tile with points outside [0, 1)^2 -- the reference's scatter would index out of
    range (coordinate.py:12-28) -- makes the optimizer boundary raise BEFORE the optimizer consumes the window, with the
    accumulators reset; a clean window then trains normally.  r05: the count reaches the host through per-tile snapshots taken
    right after each tile's index is built (pointnet.py), so the boundary waits for the last tile's ``tile_build`` only: the read
    must not be a device-wide synchronisation (torch's sync debug mode would raise on ``.item()``), and the totals of BOTH tile
    streams' status pairs count."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    model = det_init_(TomoSAR2Height(cfg), seed=19).to(_dev())
    model.set_channels_last(True)
    tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=1e-3), device=_dev(), optimize_every=4, use_cloud=True)
    tr.pipeline_tiles = pipelined
    dsm = (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(0)) * 30).to(_dev())
    clouds = [synth_cloud(20000, seed=950 + i).to(_dev()) for i in range(12)]
    for c in clouds[:4]:                                           # a clean window (the first tile lays out the bucket)
        stepped = tr.train_step({"inputs": c, "dsm": dsm})
    assert stepped
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    bad = [c.clone() for c in clouds[4:8]]
    bad[1][0, :3, 0] = 1.5                                         # 3 points on one tile stream's tile ...
    bad[2][0, :2, 1] = -0.25                                       # ... 2 on the other's
    for c in bad[:3]:
        assert tr.train_step({"inputs": c, "dsm": dsm}) is False
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                        # the boundary's read may wait for events, not for the device
    try:
        with pytest.raises(ValueError, match=r"5 input point\(s\)"):
            tr.train_step({"inputs": bad[3], "dsm": dsm})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tr.accumulated_steps == 0 and float(tr.bucket.flat.abs().sum()) == 0.0
    for k, p in model.named_parameters():
        assert torch.equal(p, before[k]), k                        # the optimizer has not consumed the bad window
    for c in clouds[8:12]:
        stepped = tr.train_step({"inputs": c, "dsm": dsm})
    assert stepped and any(not torch.equal(p, before[k]) for k, p in model.named_parameters())
