"""GPU: the PointNet++ adjoints (csrc/pnpp.hip: t2h_group_max_bwd, t2h_index_transpose, t2h_rows_gather_bwd) byte for byte
against their numpy restatement (tests/pnpp_grad_ref.py), the differentiable operators of ``pointops`` against the kernels
called directly, and the encoder's parameter gradients in ``eval()`` against the fixture of the reference's own modules
(tests/golden/make_golden_pnpp_grad.py): within 4 x max|ref32 - ref64| of the float64 gradient under fp32 convolutions.

Measured, encoder gradients: see ``test_encoder_gradients_within_the_reference_tolerance`` and DESIGN.md section 4.9."""
import numpy as np
import pytest
import torch

import pnpp_grad_ref as ref
import pnpp_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("n700", "n700u", "n1536b2")
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


# ------------------------------------------------------------------------------------------------ group max
def group_rows_case(nsample, c, ld=36, groups=5):
    """Rows with padded slots (copies of the group's first row), a column that is all zeros and one whose maximum is negative."""
    rng = np.random.default_rng(10 * nsample + c)
    rows = rng.standard_normal((groups, nsample, ld)).astype(np.float32)
    rows[:, nsample - nsample // 3:] = rows[:, :1]                  # the ball query's padding repeats the first index
    rows[1, 1] = rows[1, 0]                                         # and a tie between the first two rows
    rows[:, :, 1] = 0.0
    rows[:, :, 2] = -np.abs(rows[:, :, 2]) - 0.5
    rows[:, :, 3] = np.maximum(rows[:, :, 3], 0)                    # a ReLU output: distinct rows tie at 0
    rows[3, :, 3] = 0.0
    return rows.reshape(groups * nsample, ld)


@pytest.mark.parametrize("nsample", (3, 64))
@pytest.mark.parametrize("c", (4, 33))
def test_group_max_adjoint_equals_the_restatement(nsample, c):
    from tomosar2height_amd import pointops
    rows = group_rows_case(nsample, c)
    gout = np.random.default_rng(c).standard_normal((5, c)).astype(np.float32)
    gout[0, 0] = 0.0
    out = pointops.group_max_rows(dev(rows), nsample, c)
    assert same_bytes(out, pnpp_ref.group_max(rows, nsample)[:, :c].copy())
    for relu in (False, True):
        got = pointops.group_max_bwd(dev(rows), out, dev(gout), nsample, relu=relu, gld=36)
        want = ref.group_max_bwd(rows, nsample, out.cpu().numpy(), gout, relu, gld=36)
        assert same_bytes(got, want), (nsample, c, relu)
        nz = (got.cpu().numpy().reshape(5, nsample, 36) != 0).sum(1)
        live = (gout != 0) & ((out.cpu().numpy() > 0) | (not relu))
        assert np.array_equal(nz[:, :c], live.astype(nz.dtype)) and not nz[:, c:].any()
    assert not live[:, 1].any() and not live[:, 2].any() and not live[3, 3]       # the zero column, the negative one, the tie at 0


# ------------------------------------------------------------------------------------------------ transpose
def transpose_cases():
    from tomosar2height_amd import pointops  # noqa: F401
    cases = {}
    for k, (idx, n) in enumerate(ref.index_cases()):
        flat = np.asarray(idx).reshape(-1)
        cases[f"case{k}"] = (np.stack([flat, np.roll(flat[::-1], 7)]).reshape((2,) + np.asarray(idx).shape), n)
    # one segment longer than T2H_TRANSPOSE_SORT_MAX (the path that re-reads idx), beside one of exactly that length
    long = np.full(8192 + 8192 + 300 + 5, 1, np.int64)
    long[1:2 * 8192:2] = 2
    long[-5:] = 0
    cases["long"] = (long[None], 3)
    return cases


@pytest.mark.parametrize("name", ("case0", "case1", "case2", "long"))
def test_index_transpose_equals_the_stable_argsort(name):
    from tomosar2height_amd import pointops
    idx, n = transpose_cases()[name]
    offsets, entries = pointops.index_transpose(dev(idx, torch.long), n)
    again = pointops.index_transpose(dev(idx, torch.long), n)
    assert offsets.dtype == torch.int32 and tuple(offsets.shape) == (idx.shape[0], n + 1) and entries.dtype == torch.int32
    assert torch.equal(offsets, again[0]) and torch.equal(entries, again[1])
    for b in range(idx.shape[0]):
        flat = idx[b].reshape(-1)
        flat = np.where((flat < 0) | (flat >= n), n - 1, flat)
        assert same_bytes(entries[b], np.argsort(flat, kind="stable").astype(np.int32)), (name, b)
        assert same_bytes(offsets[b], np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n))]).astype(np.int32))
        want = ref.index_transpose(idx[b], n)
        assert same_bytes(offsets[b], want[0]) and same_bytes(entries[b], want[1])
    if name == "long":
        assert np.diff(offsets[0].cpu().numpy()).tolist() == [5, 8192 + 300, 8192]


# ------------------------------------------------------------------------------------------------ gather adjoint
def check_gather(g, col0, d, weight, fan, idx, n):
    """The kernel on (g, weight, idx) of B clouds against the restatement (bytes) and the float64 sum (the derived bound)."""
    from tomosar2height_amd import pointops
    b = idx.shape[0]
    offsets, entries = pointops.index_transpose(dev(idx, torch.long), n)
    got = pointops.rows_gather_bwd(dev(g), col0, d, None if weight is None else dev(weight), fan, offsets, entries, n)
    assert tuple(got.shape) == (b, n, d)
    rows = g.shape[0] // b
    for k in range(b):
        gk, wk = g[k * rows:(k + 1) * rows], None if weight is None else weight[k]
        o, e = offsets[k].cpu().numpy(), entries[k].cpu().numpy()
        assert same_bytes(got[k], ref.rows_gather_bwd(gk, col0, d, wk, fan, o, e, n)), (k, d, fan)
        want, bound = ref.rows_gather_bwd64(gk, col0, d, wk, fan, o, e, n)
        assert (np.abs(got[k].cpu().numpy().astype(np.float64) - want) <= bound).all()
    return got


@pytest.mark.parametrize("d", (1, 5, 128))
def test_gather_adjoint_of_the_grouped_rows(d):
    idx, n = transpose_cases()["case1"]                               # B = 2, E = 1100, N = 70; source 13 unused, 21 in > 4 chunks
    ld = (3 + d + 3) // 4 * 4
    g = np.random.default_rng(d).standard_normal((2 * 1100, ld)).astype(np.float32)
    got = check_gather(g, 3, d, None, 1, idx, n)
    assert not got[:, 13].any() and not np.signbit(got[:, 13].cpu().numpy()).any()       # an empty segment: +0


@pytest.mark.parametrize("s", (3, 1))
@pytest.mark.parametrize("d", (5, 128))
def test_gather_adjoint_of_the_propagation(s, d):
    from tomosar2height_amd import pointops
    gen = torch.Generator().manual_seed(10 * s + d)
    xyz1, xyz2 = torch.rand(2, 130, 3, generator=gen).to(DEV), torch.rand(2, s, 3, generator=gen).to(DEV)
    points2 = torch.randn(2, s, d, generator=gen).to(DEV)
    _, idx, weight = pointops.three_nn_interpolate(xyz1, xyz2, points2)
    g = torch.randn(2 * 130, d, generator=gen).numpy()
    if s == 1:
        assert weight[:, :, 1:].abs().max().item() == 0.0            # only slot 0 of a target counts
    got = check_gather(g, 0, d, weight.cpu().numpy(), 3, idx.cpu().numpy(), s)
    if s == 1:                                                        # the `repeat` branch: the plain sum of the target rows
        want = torch.as_tensor(g).view(2, 130, d).double().sum(1)
        assert torch.allclose(got[:, 0].cpu().double(), want, rtol=0, atol=130 * 2.0 ** -24 * float(np.abs(g).sum(0).max()))
        inf = g.copy()
        inf[:, 1] = np.inf
        offsets, entries = pointops.index_transpose(idx, 1)
        skipped = pointops.rows_gather_bwd(dev(inf), 0, d, weight, 3, offsets, entries, 1)
        assert bool(torch.isinf(skipped[:, 0, 1]).all()) and not bool(torch.isnan(skipped).any())     # no 0 * inf
    with pytest.raises(RuntimeError, match="S = 2"):
        pointops.three_nn_interpolate(xyz1, torch.rand(2, 2, 3, device=DEV), torch.rand(2, 2, d, device=DEV))


# ------------------------------------------------------------------------------------------------ operators
def test_operators_are_differentiable_in_their_features_only():
    from tomosar2height_amd import pointops
    gen = torch.Generator().manual_seed(3)
    xyz = torch.rand(2, 90, 3, generator=gen).to(DEV)
    feats = torch.randn(2, 90, 5, generator=gen).to(DEV)
    centres = pointops.index_points(xyz, pointops.farthest_point_sample(xyz, 9, 0)).contiguous()
    idx = pointops.query_ball_point(0.5, 7, xyz, centres)
    # grouped rows
    plain = pointops.group_rows(xyz, centres, feats, idx, 8)
    leaf = feats.clone().requires_grad_(True)
    rows = pointops.group_rows(xyz, centres, leaf, idx, 8)
    assert not plain.requires_grad and rows.requires_grad and torch.equal(plain, rows)
    grows = torch.randn(rows.shape, generator=gen).to(DEV)
    got, = torch.autograd.grad(rows, leaf, grows)
    offsets, entries = pointops.index_transpose(idx, 90)
    assert torch.equal(got, pointops.rows_gather_bwd(grows, 3, 5, None, 1, offsets, entries, 90))
    assert pointops.group_rows(xyz, centres, None, idx, 4).requires_grad is False
    # grouped max
    rleaf = plain.clone().requires_grad_(True)
    out = pointops.group_max(rleaf.view(2, 9, 7, 8))
    assert out.requires_grad and torch.equal(out, pointops.group_max(plain.view(2, 9, 7, 8)))
    gout = torch.randn(out.shape, generator=gen).to(DEV)
    got, = torch.autograd.grad(out, rleaf, gout)
    assert torch.equal(got, pointops.group_max_bwd(plain, out.detach().view(18, 8), gout.view(18, 8), 7))
    # propagation
    sources = torch.randn(2, 9, 5, generator=gen).to(DEV)
    sleaf = sources.clone().requires_grad_(True)
    plain_out, plain_idx, plain_w = pointops.three_nn_interpolate(xyz, centres, sources)
    interp, nn_idx, w = pointops.three_nn_interpolate(xyz, centres, sleaf)
    assert interp.requires_grad and not nn_idx.requires_grad and not w.requires_grad and not plain_out.requires_grad
    assert torch.equal(interp, plain_out) and torch.equal(nn_idx, plain_idx) and torch.equal(w, plain_w)
    ginterp = torch.randn(interp.shape, generator=gen).to(DEV)
    got, = torch.autograd.grad(interp, sleaf, ginterp)
    offsets, entries = pointops.index_transpose(nn_idx, 9)
    assert torch.equal(got, pointops.rows_gather_bwd(ginterp.view(180, 5), 0, 5, w, 3, offsets, entries, 9))
    with torch.no_grad():
        assert not pointops.three_nn_interpolate(xyz, centres, sleaf)[0].requires_grad


# ------------------------------------------------------------------------------------------------ encoder
def model_for(unet_type):
    if unet_type not in _cache:
        from tomosar2height_amd import TomoSAR2Height
        m = pnpp_ref.init_pnpp_(TomoSAR2Height(pnpp_ref.model_cfg(unet_type, golden("pnpp_encoder"))), seed=41)
        _cache[unet_type] = m.to(DEV).eval()
    return _cache[unet_type]


def loss_weights(shape):
    g = golden("pnpp_grad")
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(int(g["r_seed"])), dtype=torch.float32).to(DEV)


def backward(name):
    """One forward + backward of L = sum(heights * r) in eval(): (heights, {parameter: gradient} of the encoder)."""
    g = golden("pnpp_encoder")
    model = model_for(str(g[f"{name}_unet_type"]))
    enc = model.point_encoder
    enc.fps_start = (dev(g[f"{name}_start1"], torch.long), dev(g[f"{name}_start2"], torch.long))
    model.zero_grad(set_to_none=True)
    pts = dev(g[f"{name}_points"])
    heights, _ = model(input_cloud=pts)
    (heights * loss_weights(heights.shape)).sum().backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in enc.named_parameters()}
    with torch.no_grad():
        plain, _ = model(input_cloud=pts)
    return heights.detach(), plain, grads


def ratios(name, grads, say=print):
    """Per stage parameter max|grad - ref64| / ref32_dev at the stored positions; the worst of each is printed."""
    gg = golden("pnpp_grad")
    out = {}
    for pname, numel in zip(gg["param_names"], gg["param_numel"]):
        pname = str(pname)
        stride = -(-int(numel) // int(gg["max_stored"]))
        dev_ = float(gg[f"{name}/{pname}_dev"])
        want = gg[f"{name}/{pname}"].astype(np.float64) + gg[f"{name}/{pname}_q"].astype(np.float64) * dev_
        got = grads[pname].reshape(-1)[::stride].cpu().numpy().astype(np.float64)
        out[pname] = float(np.abs(got - want).max() / dev_)
        say(f"{name} {pname}: max|grad - ref64| = {out[pname]:.3g} x ref32_dev ({dev_:.3g})")
    return out


@pytest.mark.parametrize("name", CASES)
def test_encoder_gradients_within_the_reference_tolerance(name, monkeypatch):
    """fp32 convolutions: every sa* / fp* parameter's gradient within 4 x ref32_dev of the float64 reference at the stored
    positions, the U-Net's gradients present, two runs the same bytes, heights bit-equal to the no_grad forward, no fallback."""
    from tomosar2height_amd import _lib, grid
    monkeypatch.setattr(grid, "CONV_PRECISION", "fp32")
    _lib.fallback_counts(reset=True)
    heights, plain, grads = backward(name)
    _, _, again = backward(name)
    assert _lib.fallback_counts() == {}
    assert torch.equal(heights, plain)
    want, tol = pnpp_ref.ref64(golden("pnpp_encoder"), name, "heights")
    assert np.abs(heights.cpu().numpy().astype(np.float64) - want).max() <= tol
    gg = golden("pnpp_grad")
    for k in gg[f"{name}/unet_with_grad"]:
        assert grads["unet." + str(k)] is not None, k
    stage = [str(k) for k in gg["param_names"]]
    assert sorted(k for k in grads if k.split(".")[0] != "unet") == sorted(stage)
    for k in stage:
        assert grads[k] is not None and torch.equal(grads[k], again[k]), k
    worst = ratios(name, grads)
    assert max(worst.values()) <= 4.0, {k: v for k, v in worst.items() if v > 4.0}


@pytest.mark.parametrize("name", CASES)
def test_encoder_gradients_under_the_default_split_precision_are_reported(name):
    """Default ``f16x2`` convolutions: the same ratios are printed, none is bounded (the deviation comes from the U-Net's
    split-precision data gradients; figures in DESIGN.md section 4.9).  Asserted: present, finite, deterministic."""
    heights, plain, grads = backward(name)
    assert torch.equal(heights, plain)
    worst = ratios(name, grads, say=lambda s: None)
    for stage in ("sa1", "sa2", "sa3", "fp3", "fp2", "fp1"):
        print(f"{name} {stage}: worst ratio {max(v for k, v in worst.items() if k.startswith(stage)):.3g} x ref32_dev (f16x2)")
    assert all(np.isfinite(v) for v in worst.values())


def test_eval_gives_parameter_gradients_and_train_still_raises():
    g = golden("pnpp_encoder")
    model = model_for("alto")
    enc = model.point_encoder
    enc.fps_start = 0
    pts = dev(g["n700_points"])
    model.zero_grad(set_to_none=True)
    heights, _ = model(input_cloud=pts)
    heights.sum().backward()
    assert enc.sa2.mlp_convs[0].weight.grad is not None
    for k, p in enc.named_parameters():
        if k.split(".")[0] != "unet":
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
    assert all(b.grad is None for b in enc.buffers())
    model.zero_grad(set_to_none=True)
    try:
        with pytest.raises(NotImplementedError, match="BatchNorm batch statistics"):
            model.train()(input_cloud=pts)
    finally:
        model.eval()


def test_frozen_stage_builds_no_graph_and_odd_widths_raise_in_graph_mode_only():
    from tomosar2height_amd.encoder.pointnetpp import PointNetFeaturePropagation
    stage = pnpp_ref.init_pnpp_(PointNetFeaturePropagation(in_channel=8, mlp=[8, 6]), seed=5).to(DEV).eval()
    gen = torch.Generator().manual_seed(1)
    xyz1, xyz2 = torch.rand(1, 40, 3, generator=gen).to(DEV), torch.rand(1, 5, 3, generator=gen).to(DEV)
    points2 = torch.randn(1, 5, 8, generator=gen).to(DEV)
    with torch.no_grad():
        plain = stage.forward_rows(xyz1, xyz2, None, points2)
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        stage.forward_rows(xyz1, xyz2, None, points2)
    for p in stage.parameters():
        p.requires_grad_(False)
    frozen = stage.forward_rows(xyz1, xyz2, None, points2)
    assert not frozen.requires_grad and torch.equal(frozen, plain)
