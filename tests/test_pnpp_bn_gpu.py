"""GPU: BatchNorm batch statistics of the PointNet++ encoder (csrc/pnpp.hip: t2h_bn_col_stats, t2h_bn_apply_relu,
t2h_bn_running_update, t2h_bn_bwd_reduce, t2h_bn_bwd_apply) byte for byte against their numpy restatement
(tests/pnpp_bn_ref.py) and within the any-order summation bounds of float64; single stages under ``train()`` against the same
layers in float64 torch; the encoder against the fixture of the reference's own modules under ``train()``
(tests/golden/make_golden_pnpp_train.py): within 4 x max|ref32 - ref64| of float64 under fp32 convolutions; the Trainer tile by
tile against a hand loop.

Measured, encoder: see ``test_encoder_under_train_within_the_reference_tolerance`` and DESIGN.md section 4.9."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pnpp_bn_ref as ref
import pnpp_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("n700", "n700u", "n1536b2")
STAGES = ("sa1", "sa2", "sa3", "fp3", "fp2", "fp1")
U = 2.0 ** -24
_cache = {}


def golden(name):
    if name not in _cache:
        _cache[name] = load_golden(name)
    return _cache[name]


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def same_bytes(t, a):
    got = t.detach().cpu().numpy()
    return got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == a.tobytes()


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ kernels
def rows_case(m, c, ld):
    """Rows with two constant columns (var = 0; one of them zero) and a column whose mean is 1e5 x its spread."""
    rng = np.random.default_rng(1000 * m + c)
    z = (rng.standard_normal((m, ld)) * rng.uniform(0.3, 3.0, ld) + rng.uniform(-2, 2, ld)).astype(np.float32)
    z[:, 0] = 1.75
    z[:, 1] = (1e3 + 1e-2 * rng.standard_normal(m)).astype(np.float32)
    z[:, 3] = 0.0
    return z


@pytest.mark.parametrize("c", (4, 68, 1024))
@pytest.mark.parametrize("m", (2, 63, 64, 65, ref.SLAB - 1, ref.SLAB, ref.SLAB + 1, 3 * ref.SLAB + 17))
def test_kernels_equal_the_restatement_and_stay_within_the_summation_bound(m, c):
    from tomosar2height_amd import pointops
    ld, eps, mom = c + 4, 1e-5, 0.1
    rng = np.random.default_rng(7 * m + c)
    z = rows_case(m, c, ld)
    gamma, beta = rng.uniform(0.75, 1.25, c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)
    zd = dev(z)
    # statistics
    mean, var, rstd = pointops.bn_col_stats(zd, c, eps)
    again = pointops.bn_col_stats(zd, c, eps)
    assert all(torch.equal(a, b) for a, b in zip((mean, var, rstd), again))
    wmean, wvar, wrstd = ref.col_stats(z, c, eps)
    assert same_bytes(mean, wmean) and same_bytes(var, wvar) and same_bytes(rstd, wrstd), (m, c)
    (m64, mb), (v64, vb) = ref.col_stats64(z, c, wmean)
    assert (np.abs(f64(mean) - m64) <= mb).all() and (np.abs(f64(var) - v64) <= vb).all()
    # (the variance about the kernel's own mean is (mean32 - mean64)^2 away from the true one)
    assert (np.abs(f64(var) - np.asarray(z, np.float64)[:, :c].var(0)) <= vb + mb ** 2).all()
    assert float(var[0]) == 0.0 and float(var[3]) == 0.0 and float(mean[0]) == 1.75        # the constant columns
    if m >= 63:                                                                            # mean >> spread: no cancellation
        assert abs(float(var[1]) - v64[1]) <= 1e-3 * v64[1] and 2e-5 < float(var[1]) < 5e-4
    # apply + ReLU
    y = pointops.bn_apply_relu(zd, c, mean, rstd, dev(gamma), dev(beta), ldy=ld)
    wy = ref.apply_relu(z, c, wmean, wrstd, gamma, beta, ld)
    assert same_bytes(y, wy) and not y[:, c:].any() and not np.signbit(y[:, c:].cpu().numpy()).any()
    assert torch.equal(y, pointops.bn_apply_relu(zd, c, mean, rstd, dev(gamma), dev(beta), ldy=ld))
    s64 = gamma.astype(np.float64) * wrstd
    t64 = beta.astype(np.float64) - wmean.astype(np.float64) * s64
    zs = z[:, :c].astype(np.float64) * s64
    ms = np.abs(wmean.astype(np.float64) * s64)
    # roundings: s and z s | s and mean s | t | the sum
    bound = U * (2 * np.abs(zs) + 2 * ms + np.abs(t64) + np.abs(zs + t64)) * (1 + 2.0 ** -10)
    assert (np.abs(f64(y)[:, :c] - np.maximum(zs + t64, 0)) <= bound).all()
    # running statistics
    rm0, rv0 = rng.uniform(-0.1, 0.1, c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32)
    rm, rv = dev(rm0), dev(rv0)
    versions = rm._version, rv._version
    pointops.bn_running_update(mean, var, m, mom, rm, rv)
    wrm, wrv = ref.running_update(wmean, wvar, m, mom, rm0, rv0)
    assert same_bytes(rm, wrm) and same_bytes(rv, wrv) and rm._version > versions[0] and rv._version > versions[1]
    want = 0.9 * rv0.astype(np.float64) + 0.1 * wvar.astype(np.float64) * m / (m - 1)
    assert (np.abs(f64(rv) - want) <= 6 * U * (np.abs(want) + 1)).all()
    # backward
    gy = rng.standard_normal((m, ld)).astype(np.float32)
    for relu in (True, False):
        dbeta, dgamma = pointops.bn_bwd_reduce(dev(gy), y if relu else None, zd, c, mean, rstd, relu)
        wdb, wdg = ref.bwd_reduce(gy, wy, z, c, wmean, wrstd, relu)
        assert same_bytes(dbeta, wdb) and same_bytes(dgamma, wdg), (m, c, relu)
        g = ref._masked(gy, wy, c, relu)
        xhat32 = (z[:, :c] - wmean[None]) * wrstd[None]
        s, b = ref.sum64(g, 0)
        assert (np.abs(f64(dbeta) - s) <= b).all()
        s, b = ref.sum64(g.astype(np.float64) * xhat32.astype(np.float64), 1)             # xhat as the kernel forms it; the product
        assert (np.abs(f64(dgamma) - s) <= b).all()
        dz = pointops.bn_bwd_apply(dev(gy), y if relu else None, zd, c, mean, rstd, dev(gamma), dbeta, dgamma, relu, gld=ld)
        wdz = ref.bwd_apply(gy, wy, z, c, wmean, wrstd, gamma, wdb, wdg, relu, ld)
        assert same_bytes(dz, wdz) and not dz[:, c:].any()
        assert torch.equal(dz, pointops.bn_bwd_apply(dev(gy), y if relu else None, zd, c, mean, rstd, dev(gamma), dbeta, dgamma, relu, gld=ld))
        a64 = gamma.astype(np.float64) * wrstd
        mbq, mgq = wdb.astype(np.float64) / m, wdg.astype(np.float64) / m
        inner = np.abs(g) + np.abs(mbq) + np.abs(xhat32 * mgq)
        want = a64 * ((g - mbq) - xhat32.astype(np.float64) * mgq)
        # roundings: mb, mg, xhat mg (on mg's), g - mb, the difference: <= 5 u inner; a and the final product: 2 u |a| inner
        assert (np.abs(f64(dz)[:, :c] - want) <= 7 * U * np.abs(a64) * inner * (1 + 2.0 ** -10)).all()


def test_one_row_raises_torchs_error():
    from tomosar2height_amd import _lib, pointops
    z = torch.zeros(1, 8, device=DEV)
    v = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        pointops.bn_col_stats(z, 8, 1e-5)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        pointops.bn_apply_relu(z, 8, v, v, v, v)
    scratch = torch.zeros(64, device=DEV)
    with pytest.raises(_lib.T2HLibraryError):                                              # the entry itself refuses M < 2
        _lib.call("t2h_bn_col_stats", _lib.ptr(z), 8, 1, 8, 1e-5, _lib.ptr(scratch), _lib.ptr(v), _lib.ptr(v), _lib.ptr(v),
                  _lib.stream())


# ------------------------------------------------------------------------------------------------ stages
def stage_layers(stage, x, dtype, nsample=0):
    """The stage's layers restated in torch on channels-first ``x`` ([1, K, M] rows as a Conv1d batch): conv + batch_norm(
    training=True) + relu per layer, then the max over groups of ``nsample`` rows.  Returns (out rows, parameters, buffers)."""
    ps, bufs, zs = [], [], []
    h = x.to(dtype)
    for conv, bn in zip(stage.mlp_convs, stage.mlp_bns):
        w = conv.weight.detach().reshape(conv.weight.shape[0], -1, 1).to(dtype).cpu().requires_grad_(True)
        b, ga, be = (t.detach().to(dtype).cpu().requires_grad_(True) for t in (conv.bias, bn.weight, bn.bias))
        rm, rv = bn.running_mean.detach().to(dtype).cpu().clone(), bn.running_var.detach().to(dtype).cpu().clone()
        z = F.conv1d(h, w, b)
        z.retain_grad()
        h = F.relu(F.batch_norm(z, rm, rv, ga, be, training=True, momentum=bn.momentum, eps=bn.eps))
        zs.append(z)
        ps += [w, b, ga, be]
        bufs += [rm, rv]
    out = h[0].t()
    if nsample:
        out = out.reshape(-1, nsample, out.shape[1]).max(1)[0]
    return out, ps, bufs, zs


def check_stage(stage, rows, nsample, run):
    """``run()`` -> the stage's output rows under train(); compares output, parameter gradients and buffers with float64 torch
    on the same rows, each within 4 x the float32-torch deviation from that float64 run."""
    before = copy.deepcopy(stage.state_dict())
    x = rows.detach().cpu().t()[None]
    gen = torch.Generator().manual_seed(3)
    stage.load_state_dict(before)
    o64, p64, b64, z64 = stage_layers(stage, x, torch.float64, nsample)
    o32, p32, b32, _ = stage_layers(stage, x, torch.float32, nsample)
    r = torch.randn(o64.shape, generator=gen, dtype=torch.float32)
    (o64 * r.double()).sum().backward()
    (o32 * r).sum().backward()
    out = run()
    (out.reshape(o64.shape) * r.to(DEV)).sum().backward()
    ours_p = [t for conv, bn in zip(stage.mlp_convs, stage.mlp_bns) for t in (conv.weight, conv.bias, bn.weight, bn.bias)]
    ours_b = [t for bn in stage.mlp_bns for t in (bn.running_mean, bn.running_var)]

    def within(got, t32, t64, what, floor=0.0):
        ref_dev = float((t32.double() - t64).abs().max())
        err = float((got.detach().cpu().double().reshape(t64.shape) - t64).abs().max())
        print(f"{what}: {err:.3g} against 4 x {ref_dev:.3g}")
        assert err <= 4 * ref_dev + floor, what

    within(out, o32.detach(), o64.detach(), "output")
    for k, (got, a, b) in enumerate(zip(ours_p, p32, p64)):
        assert got.grad is not None
        if k % 4 == 1:           # conv bias: exactly 0, rounding noise on every side: |db| <= 2 M 2^-24 sum_r |dz|
            m, l1 = x.shape[2], z64[k // 4].grad.abs().sum(dim=(0, 2))
            assert bool((got.grad.detach().cpu().double().abs() <= 2 * m * U * l1).all()), f"conv bias {k // 4}"
            continue
        within(got.grad, a.grad, b.grad, f"parameter {k}")
    for k, (got, a, b) in enumerate(zip(ours_b, b32, b64)):
        within(got, a, b, f"buffer {k}")
    assert all(int(bn.num_batches_tracked) == int(before[f"mlp_bns.{i}.num_batches_tracked"]) + 1 for i, bn in enumerate(stage.mlp_bns))


def test_propagation_stage_under_train_matches_float64_torch():
    from tomosar2height_amd import _lib
    from tomosar2height_amd.encoder.pointnetpp import PointNetFeaturePropagation
    stage = pnpp_ref.init_pnpp_(PointNetFeaturePropagation(in_channel=8, mlp=[8, 8]), seed=5).to(DEV).train()
    assert stage.batch_statistics is False
    gen = torch.Generator().manual_seed(1)
    xyz1, xyz2 = torch.rand(1, 40, 3, generator=gen).to(DEV), torch.rand(1, 5, 3, generator=gen).to(DEV)
    points2 = torch.randn(1, 5, 8, generator=gen).to(DEV)
    with pytest.raises(NotImplementedError, match="BatchNorm batch statistics"):
        stage.forward_rows(xyz1, xyz2, None, points2)
    stage.batch_statistics = True
    _lib.fallback_counts(reset=True)
    trace = {}
    with torch.no_grad():
        state = copy.deepcopy(stage.state_dict())
        stage.forward_rows(xyz1, xyz2, None, points2, trace)
        stage.load_state_dict(state)
    check_stage(stage, trace["interpolated"].reshape(40, 8), 0, lambda: stage.forward_rows(xyz1, xyz2, None, points2))
    assert _lib.fallback_counts() == {}


def test_set_abstraction_stage_under_train_matches_float64_torch():
    from tomosar2height_amd import _lib, pointops
    from tomosar2height_amd.encoder.pointnetpp import PointNetSetAbstraction
    stage = pnpp_ref.init_pnpp_(PointNetSetAbstraction(npoint=16, radius=0.4, nsample=8, in_channel=3 + 3, mlp=[8, 8],
                                                       group_all=False), seed=6).to(DEV).train()
    stage.batch_statistics = True
    gen = torch.Generator().manual_seed(2)
    xyz = torch.rand(1, 200, 3, generator=gen).to(DEV)
    feats = torch.randn(1, 200, 3, generator=gen).to(DEV)
    _lib.fallback_counts(reset=True)
    fps = pointops.farthest_point_sample(xyz, 16, 0)
    new_xyz = pointops.index_points(xyz, fps).contiguous()
    idx = pointops.query_ball_point(0.4, 8, xyz, new_xyz)
    rows = pointops.group_rows(xyz, new_xyz, feats, idx, 8)[:, :6]
    check_stage(stage, rows, 8, lambda: stage.forward_rows(xyz, feats, 0)[1])
    assert _lib.fallback_counts() == {}


# ------------------------------------------------------------------------------------------------ encoder
def model_for(unet_type, switch=True):
    key = (unet_type, switch)
    if key not in _cache:
        from tomosar2height_amd import TomoSAR2Height
        cfg = pnpp_ref.model_cfg(unet_type, golden("pnpp_encoder"))
        if switch:
            cfg.model.encoder_kwargs["batch_statistics"] = True
        m = pnpp_ref.init_pnpp_(TomoSAR2Height(cfg), seed=41).to(DEV)
        _cache[key] = (m, copy.deepcopy(m.state_dict()))
    m, state = _cache[key]
    m.load_state_dict(state)
    return m


def loss_weights(shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(int(golden("pnpp_train")["r_seed"])),
                       dtype=torch.float32).to(DEV)


def train_run(name):
    """Forward + backward under train(), then a second forward under no_grad: (heights, gradients, buffers after each)."""
    g = golden("pnpp_encoder")
    model = model_for(str(g[f"{name}_unet_type"])).train()
    enc = model.point_encoder
    assert enc.batch_statistics and enc.sa1.batch_statistics and enc.fp1.batch_statistics
    enc.fps_start = (dev(g[f"{name}_start1"], torch.long), dev(g[f"{name}_start2"], torch.long))
    model.zero_grad(set_to_none=True)
    pts = dev(g[f"{name}_points"])
    bufs = lambda: {k: v.detach().clone() for k, v in enc.named_buffers() if k.split(".")[0] in STAGES}
    heights, _ = model(input_cloud=pts)
    buf1 = bufs()
    (heights * loss_weights(heights.shape)).sum().backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in enc.named_parameters()}
    with torch.no_grad():
        again, _ = model(input_cloud=pts)
    assert torch.equal(again, heights) and not again.requires_grad          # the batch statistics do not depend on the buffers
    return heights.detach(), grads, buf1, bufs()


def stored64(gt, key):
    d = float(gt[key + "_dev"])
    return gt[key].astype(np.float64) + gt[key + "_q"].astype(np.float64) * d, d


def ratios(name, heights, grads, buf1, buf2, say=print):
    """max|ours - ref64| / ref32_dev of the heights, every stored gradient and every buffer; conv biases (exact value 0) have
    their own bound, ``conv_bias_excess``, and are left out."""
    gt = golden("pnpp_train")
    out = {}
    want, d = stored64(gt, f"{name}/heights")
    out["heights"] = float(np.abs(f64(heights).reshape(-1) - want).max() / d)
    for pname, numel in zip(gt["param_names"], gt["param_numel"]):
        pname = str(pname)
        assert grads[pname] is not None, pname
        got = f64(grads[pname].reshape(-1)[::-(-int(numel) // int(gt["max_stored"]))])
        if ".mlp_convs." in pname and pname.endswith(".bias"):       # exactly 0: ``conv_bias_excess``
            continue
        want, d = stored64(gt, f"{name}/{pname}")
        out[pname] = float(np.abs(got - want).max() / d)
    for tag, bufs in (("buf1", buf1), ("buf2", buf2)):
        for bname in gt["buffer_names"]:
            want, d = stored64(gt, f"{name}/{tag}/{bname}")
            out[f"{tag}/{bname}"] = float(np.abs(f64(bufs[str(bname)]) - want).max() / d)
    for k, v in out.items():
        say(f"{name} {k}: {v:.3g} x ref32_dev")
    return out


def conv_bias_excess(name, grads):
    """Per conv bias max_c |db[c]| / (2 M 2^-24 l1[c]) with M and l1 = sum_r |dz| of the float64 reference run."""
    gt = golden("pnpp_train")
    out = {}
    for pname in (str(k) for k in gt["param_names"]):
        if ".mlp_convs." in pname and pname.endswith(".bias"):
            assert grads[pname] is not None, pname
            bound = 2 * int(gt[f"{name}/rows/{pname}"]) * U * gt[f"{name}/l1/{pname}"]
            with np.errstate(divide="ignore", invalid="ignore"):
                out[pname] = float(np.nan_to_num(np.abs(f64(grads[pname])) / bound, nan=0.0).max())
            print(f"{name} {pname}: max|db| / (2 M u l1) = {out[pname]:.3g}")
    return out


def worst_per_stage(worst):
    return {s: max(v for k, v in worst.items() if k.split("/")[-1].startswith(s)) for s in STAGES}


@pytest.mark.parametrize("name", CASES)
def test_encoder_under_train_within_the_reference_tolerance(name, monkeypatch):
    """fp32 convolutions: heights, every stored gradient and every running statistic (after one and two forwards) within
    4 x ref32_dev of the float64 reference; num_batches_tracked exact; conv-bias gradients within 2 M 2^-24 l1; two runs the
    same bytes; no fallback."""
    from tomosar2height_amd import _lib, grid
    monkeypatch.setattr(grid, "CONV_PRECISION", "fp32")
    _lib.fallback_counts(reset=True)
    heights, grads, buf1, buf2 = train_run(name)
    h2, g2, b12, b22 = train_run(name)
    assert _lib.fallback_counts() == {}
    assert torch.equal(heights, h2) and all(torch.equal(buf2[k], b22[k]) and torch.equal(buf1[k], b12[k]) for k in buf1)
    gt = golden("pnpp_train")
    for k in (str(k) for k in gt["param_names"]):
        assert torch.equal(grads[k], g2[k]), k
    nbt = lambda b: [int(v) for k, v in b.items() if k.endswith("num_batches_tracked")]
    assert nbt(buf1) == gt[f"{name}/nbt1"].tolist() and nbt(buf2) == gt[f"{name}/nbt2"].tolist()
    worst = ratios(name, heights, grads, buf1, buf2, say=lambda s: None)
    print(f"{name}: heights {worst['heights']:.3g}; per stage {({k: round(v, 3) for k, v in worst_per_stage(worst).items()})}")
    assert max(worst.values()) <= 4.0, {k: v for k, v in worst.items() if v > 4.0}


@pytest.mark.parametrize("name", CASES)
def test_conv_bias_gradients_within_the_summation_bound(name, monkeypatch):
    """The exact gradient of a conv bias under batch statistics is 0; asserted: |db[c]| <= 2 M 2^-24 l1[c], l1 = sum_r |dz[r, c]|
    of the float64 reference.  Measured: at most 0.07 of the bound (``fp3.mlp_convs.0``), 1e-5 .. 1e-3 elsewhere.

    ``sa3`` of the B = 1 cases is the sharp end of this check.  With one cloud, ``sa3``'s single feature row reaches ``fp3``'s
    first BatchNorm as a constant over its 128 rows, which the normalisation removes: the whole gradient of ``sa3`` is exactly
    0 and the float64 reference's dz there is float64 rounding noise (l1 <= 1e-10, with exact zeros, against 1e3 .. 1e7
    everywhere else), so only db == 0 passes -- float32 noise misses the bound by 1e6 (the reference's own float32 gradients
    in the fixture do, by 8e5 .. 1.2e6).  The encoder returns that exact zero (``_RowConstant``)."""
    from tomosar2height_amd import grid
    monkeypatch.setattr(grid, "CONV_PRECISION", "fp32")
    _, grads, _, _ = train_run(name)
    excess = conv_bias_excess(name, grads)
    assert max(excess.values()) <= 1.0, {k: v for k, v in excess.items() if v > 1.0}


def test_one_cloud_gives_sa3_exact_zero_gradients_and_two_clouds_do_not():
    """B = 1: the global feature is a constant to fp3's first BatchNorm, every sa3 gradient is exactly 0 (present, not None);
    B = 2: a constant per cloud only, the ordinary adjoint runs."""
    _, one, _, _ = train_run("n700")
    _, two, _, _ = train_run("n1536b2")
    sa3 = [k for k in one if k.startswith("sa3.")]
    assert len(sa3) == 12
    for k in sa3:
        assert one[k] is not None and one[k].shape == two[k].shape and not bool(one[k].any()), k
        if not (".mlp_convs." in k and k.endswith(".bias")):
            assert bool(two[k].any()), k
    assert all(bool(v.any()) for k, v in one.items() if k.split(".")[0] in ("sa1", "sa2", "fp3") and not k.endswith("convs.0.bias")
               and ".mlp_bns." in k)


@pytest.mark.parametrize("name", CASES)
def test_encoder_under_train_with_the_default_split_precision_is_reported(name):
    """Default ``f16x2`` convolutions: the same ratios are printed, not bounded (the U-Net's split-precision data gradients
    feed every stage).  The buffers do not depend on the U-Net: bounded as above."""
    heights, grads, buf1, buf2 = train_run(name)
    worst = ratios(name, heights, grads, buf1, buf2, say=lambda s: None)
    print(f"{name} (f16x2): heights {worst['heights']:.3g}; per stage {({k: round(v, 3) for k, v in worst_per_stage(worst).items()})}")
    assert all(np.isfinite(v) for v in worst.values())
    assert max(v for k, v in worst.items() if k.startswith("buf")) <= 4.0


def test_eval_ignores_the_switch_and_no_grad_training_saves_nothing():
    g = golden("pnpp_encoder")
    pts = dev(g["n700_points"])
    on, off = model_for("alto", True).eval(), model_for("alto", False).eval()
    assert on.point_encoder.batch_statistics and not off.point_encoder.batch_statistics
    assert list(on.state_dict()) == list(off.state_dict())
    on.point_encoder.fps_start = off.point_encoder.fps_start = 0
    with torch.no_grad():
        assert torch.equal(on(input_cloud=pts)[0], off(input_cloud=pts)[0])
    before = {k: v.clone() for k, v in on.point_encoder.named_buffers()}
    on.train()
    with torch.no_grad():
        heights, _ = on(input_cloud=pts)
    assert not heights.requires_grad and heights.grad_fn is None
    after = dict(on.point_encoder.named_buffers())
    for k, v in before.items():
        if k.split(".")[0] in STAGES:
            assert not torch.equal(after[k], v), k
            if k.endswith("num_batches_tracked"):
                assert int(after[k]) == int(v) + 1
    # the fold of eval() follows the new running statistics
    with torch.no_grad():
        moved = on.eval()(input_cloud=pts)[0]
        off.load_state_dict(on.state_dict())
        assert torch.equal(moved, off(input_cloud=pts)[0])
    with pytest.raises(NotImplementedError, match="BatchNorm batch statistics"):
        off.train()(input_cloud=pts)
    off.eval()


# ------------------------------------------------------------------------------------------------ Trainer
def test_trainer_issues_tiles_one_by_one_and_matches_a_hand_loop(monkeypatch):
    from tomosar2height_amd.trainer import Trainer
    g = golden("pnpp_encoder")
    from tomosar2height_amd import TomoSAR2Height
    model = model_for("alto", True).train()
    model.point_encoder.fps_start = 0
    cfg = pnpp_ref.model_cfg("alto", g)
    cfg.model.encoder_kwargs["batch_statistics"] = True
    hand = TomoSAR2Height(cfg).to(DEV).train()               # (a second model with the same state: the caches are per model)
    hand.load_state_dict(model.state_dict())
    hand.point_encoder.fps_start = 0
    gen = torch.Generator().manual_seed(11)
    base = torch.from_numpy(g["n700_points"])
    with torch.no_grad():
        shape = model.eval()(input_cloud=base.to(DEV))[0].squeeze().shape
        model.train()
    tiles = [{"inputs": base[:, torch.randperm(base.shape[1], generator=gen)].contiguous().to(DEV),
              "dsm": torch.randn(tuple(shape), generator=gen).to(DEV)} for _ in range(4)]
    lr = 1e-3
    trainer = Trainer(model, torch.optim.SGD(model.parameters(), lr=lr), device=DEV, optimize_every=2, use_cloud=True)
    seen, batches = [], []
    # what the optimizer consumes: the bucket's views, parameter by parameter (a view keeps its gradient's own dense layout, so the
    # flat buffer is compared through them, not position by position)
    trainer.on_reduced = lambda flat: seen.append((flat.numel(), [p.grad.detach().clone() for p in trainer.bucket.params]))
    real = trainer._losses
    monkeypatch.setattr(trainer, "_losses", lambda data, thr: (batches.append(len(data) if isinstance(data, (list, tuple)) else 1),
                                                               real(data, thr))[1])
    opt = torch.optim.SGD(hand.parameters(), lr=lr)
    names = {id(p): k for k, p in model.named_parameters()}
    hp = dict(hand.named_parameters())
    for window in range(2):
        stepped = [trainer.train_step(t) for t in tiles[2 * window:2 * window + 2]]
        assert stepped == [False, True]
        opt.zero_grad(set_to_none=True)
        total = 0.0
        for t in tiles[2 * window:2 * window + 2]:
            pa, _ = hand.train()(input_cloud=t["inputs"])
            loss = F.l1_loss(pa.squeeze(), t["dsm"])
            loss.backward()
            total = total + loss.detach()
        numel, got = seen[window]
        want = [hp[names[id(p)]].grad for p in trainer.bucket.params]
        assert numel == sum(-(-p.numel() // 4) * 4 for p in trainer.bucket.params) and all(w is not None for w in want)
        assert sorted(names[id(p)] for p in trainer.bucket.params) == sorted(k for k, q in hp.items() if q.grad is not None)
        top = max(float(w.abs().max()) for w in want)
        worst = max((float((a - w).abs().max()), names[id(p)]) for a, w, p in zip(got, want, trainer.bucket.params))
        print(f"window {window}: worst gradient deviation {worst[0]:.3g} ({worst[1]}) of max-norm {top:.3g}")
        assert worst[0] <= 2e-5 * top, worst
        assert abs(float(trainer.last_avg_loss) - float(total) / 2) <= 1e-6 * max(1.0, abs(float(total) / 2))
        if window == 0:
            for (k, a), (_, b) in zip(model.point_encoder.named_buffers(), hand.point_encoder.named_buffers()):
                assert torch.equal(a, b), k
        opt.step()
    assert batches == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        trainer.train_step([tiles[0], tiles[1]])
    with pytest.raises(NotImplementedError):
        trainer.capture_graph(tiles[0])
    with pytest.raises(NotImplementedError):
        trainer.capture_pipeline_graphs(tiles[0])
