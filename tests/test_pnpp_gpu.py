"""GPU: the PointNet++ kernels (csrc/pnpp.hip through tomosar2height_amd.pointops) and the encoder built on them against the
fixture of the reference's own modules (tests/golden/make_golden_pnpp.py) and the numpy restatement (tests/pnpp_ref.py).
Discrete stages are compared bit for bit; features within 4 x max|ref32 - ref64| of the float64 reference."""
import numpy as np
import pytest
import torch

import pnpp_ref
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNAMBIGUOUS = ("n700", "n1536b2", "n300")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("pnpp_encoder")
    return _cache["g"]


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def model_for(unet_type):
    if unet_type not in _cache:
        from tomosar2height_amd import TomoSAR2Height
        m = pnpp_ref.init_pnpp_(TomoSAR2Height(pnpp_ref.model_cfg(unet_type, golden())), seed=41)
        _cache[unet_type] = m.to(DEV).eval()
    return _cache[unet_type]


def levels(name):
    """xyz of the three levels of a case on the device, from the fixture's FPS indices."""
    g = golden()
    pts = dev(g[f"{name}_points"])
    from tomosar2height_amd import pointops
    l1 = pointops.index_points(pts, dev(g[f"{name}_sa1_fps"], torch.long)).contiguous()
    l2 = pointops.index_points(l1, dev(g[f"{name}_sa2_fps"], torch.long)).contiguous()
    return pts, l1, l2


# ------------------------------------------------------------------------------------------------ FPS
@pytest.mark.parametrize("name", UNAMBIGUOUS)
def test_fps_equals_the_reference(name):
    from tomosar2height_amd import pointops
    g = golden()
    pts, l1, _ = levels(name)
    got1 = pointops.farthest_point_sample(pts, 512, dev(g[f"{name}_start1"], torch.long))
    got2 = pointops.farthest_point_sample(l1, 128, dev(g[f"{name}_start2"], torch.long))
    assert got1.dtype == torch.long and np.array_equal(got1.cpu().numpy(), g[f"{name}_sa1_fps"])
    assert np.array_equal(got2.cpu().numpy(), g[f"{name}_sa2_fps"])


@pytest.mark.parametrize("name", ("n700", "n1536b2"))
def test_fps_sliced_form_equals_the_one_workgroup_form(name, monkeypatch):
    from tomosar2height_amd import pointops
    g = golden()
    pts = dev(g[f"{name}_points"])
    start = dev(g[f"{name}_start1"], torch.long)
    assert pointops.fps_launches(pts.shape[1], 512) == 1
    one = pointops.farthest_point_sample(pts, 512, start)
    monkeypatch.setenv("T2H_FPS_SLICE", "256")
    assert pointops.fps_launches(pts.shape[1], 512) == 512
    sliced = pointops.farthest_point_sample(pts, 512, start)
    again = pointops.farthest_point_sample(pts, 512, start)
    assert torch.equal(one, sliced) and torch.equal(sliced, again)
    assert np.array_equal(sliced.cpu().numpy(), g[f"{name}_sa1_fps"])


def test_fps_ties_on_the_duplicates_cloud_equal_the_restatement(monkeypatch):
    from tomosar2height_amd import pointops
    g = golden()
    pts = g["dup1024_points"]
    want = pnpp_ref.fps(pts[0], 512, g["dup1024_start1"][0])
    one = pointops.farthest_point_sample(dev(pts), 512, dev(g["dup1024_start1"], torch.long))
    monkeypatch.setenv("T2H_FPS_SLICE", "256")
    sliced = pointops.farthest_point_sample(dev(pts), 512, dev(g["dup1024_start1"], torch.long))
    assert np.array_equal(one[0].cpu().numpy(), want) and torch.equal(one, sliced)
    # every point equal: all distances 0 after the first centroid -> index 0 from then on (the lowest index of the maximum)
    same = torch.full((1, 200, 3), 0.25, device=DEV)
    assert pointops.farthest_point_sample(same, 8, 5).cpu().tolist() == [[5, 0, 0, 0, 0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------------ ball query, rows, max
@pytest.mark.parametrize("name", UNAMBIGUOUS + ("dup1024",))
def test_ball_query_rows_and_max(name):
    from tomosar2height_amd import pointops
    g = golden()
    pts, l1, l2 = levels(name)
    idx1 = pointops.query_ball_point(0.2, 32, pts, l1)
    idx2 = pointops.query_ball_point(0.4, 64, l1, l2)
    assert idx1.dtype == torch.long and tuple(idx1.shape) == (pts.shape[0], 512, 32)
    for b in range(pts.shape[0]):
        p, q1, q2 = g[f"{name}_points"][b], l1[b].cpu().numpy(), l2[b].cpu().numpy()
        if name in UNAMBIGUOUS:
            assert np.array_equal(idx1[b].cpu().numpy(), g[f"{name}_sa1_idx"][b])
            assert np.array_equal(idx2[b].cpu().numpy(), g[f"{name}_sa2_idx"][b])
        assert np.array_equal(idx1[b].cpu().numpy(), pnpp_ref.ball_query(0.2, 32, p, q1))
        assert np.array_equal(idx2[b].cpu().numpy(), pnpp_ref.ball_query(0.4, 64, q1, q2))
    feats = torch.sin(torch.arange(pts.shape[0] * pts.shape[1] * 5, device=DEV, dtype=torch.float32)).view(pts.shape[0], -1, 5)
    rows = pointops.group_rows(pts, l1, feats, idx1, 8)
    new_xyz, new_points = pointops.sample_and_group(512, 0.2, 32, pts, feats, start=dev(g[f"{name}_start1"], torch.long))
    assert torch.equal(new_xyz, l1) and tuple(new_points.shape) == (pts.shape[0], 512, 32, 8)
    assert torch.equal(new_points.reshape(-1, 8), rows)
    for b in range(pts.shape[0]):
        want = pnpp_ref.group_rows(g[f"{name}_points"][b], l1[b].cpu().numpy(), feats[b].cpu().numpy(), idx1[b].cpu().numpy(), 8)
        got = rows.view(pts.shape[0], -1, 8)[b].cpu().numpy()
        assert got.tobytes() == want.tobytes()
        assert pointops.group_max(new_points)[b].cpu().numpy().tobytes() == pnpp_ref.group_max(want, 32).tobytes()


def test_ball_query_pads_with_the_first_index_and_reports_an_empty_group():
    from tomosar2height_amd import pointops
    xyz = torch.zeros(1, 70, 3, device=DEV)
    xyz[0, :, 0] = torch.arange(70, device=DEV) * 0.125              # a line of points 0.125 apart
    query = xyz[:, [66, 3]].contiguous().clone()
    query = torch.cat([query, torch.full((1, 1, 3), 50.0, device=DEV)], 1)
    idx = pointops.query_ball_point(0.25, 8, xyz, query)[0].cpu().tolist()
    assert idx[0] == [64, 65, 66, 67, 68, 64, 64, 64]                # five inside (|dx| <= 0.25 exactly counts), padded with the first
    assert idx[1] == [1, 2, 3, 4, 5, 1, 1, 1]
    assert idx[2] == [70] * 8                                        # no neighbour: N, as the reference
    assert pointops.query_ball_point(0.25, 3, xyz, query)[0, 0].cpu().tolist() == [64, 65, 66]      # early exit at nsample


# ------------------------------------------------------------------------------------------------ 3-NN
@pytest.mark.parametrize("name", UNAMBIGUOUS + ("dup1024",))
def test_three_nn_indices_weights_and_rows(name):
    """Both propagation levels on the reference's own source features (the fixture's float32 l1_points / l2_points).  Indices
    byte-equal to the reference's (to the restatement's on the duplicates cloud); weights and interpolated rows within
    4 x ref32_dev of ref64 on ALL rows and of ref32 on the non-coincident rows, the excluded rows being exactly those with
    float64 d2_min < 1e-12 (counted: at most S per cloud and level); everything byte-equal to the restatement."""
    from tomosar2height_amd import pointops
    g = golden()
    pts, l1, l2 = levels(name)
    f1, f2 = dev(g[f"{name}_l1_points"]), dev(g[f"{name}_l2_points"])
    out1, idx1, w1 = pointops.three_nn_interpolate(pts, l1, f1)
    out2, idx2, w2 = pointops.three_nn_interpolate(l1, l2, f2)
    for b in range(pts.shape[0]):
        p, q1, q2 = g[f"{name}_points"][b], l1[b].cpu().numpy(), l2[b].cpu().numpy()
        for level, targets, sources, feats, idx, w, out, s_max in (("fp1", p, q1, f1, idx1, w1, out1, 512), ("fp2", q1, q2, f2, idx2, w2, out2, 128)):
            got_idx, got_w, got_rows = idx[b].cpu().numpy(), w[b].cpu().numpy(), out[b].cpu().numpy()
            ridx, rw, _ = pnpp_ref.three_nn(targets, sources)
            assert np.array_equal(got_idx, ridx) and got_w.tobytes() == rw.tobytes()
            assert got_rows.tobytes() == pnpp_ref.interpolate(feats[b].cpu().numpy(), ridx, rw).tobytes()
            if name not in UNAMBIGUOUS:
                continue
            want, fps = g[f"{name}_{level}_idx"][b], g[f"{name}_sa1_fps"][b]
            if name == "n300" and level == "fp1":   # repeated centroids: equal distances among the copies of point 0 (test_pnpp_cpu.py)
                got_idx, want = fps[got_idx], fps[want]
            assert np.array_equal(got_idx, want)
            mask = pnpp_ref.check_three_nn(g, name, level, b, got_w, got_rows)
            assert np.array_equal(mask, pnpp_ref.coincident(targets, sources))
            assert int(mask.sum()) <= s_max or name == "n300"


def test_three_nn_single_source_repeats_it():
    from tomosar2height_amd import pointops
    xyz1 = torch.rand(2, 37, 3, device=DEV)
    src = torch.rand(2, 1, 3, device=DEV)
    feats = torch.rand(2, 1, 20, device=DEV)
    out, idx, w = pointops.three_nn_interpolate(xyz1, src, feats)
    assert torch.equal(out, feats.expand(2, 37, 20)) and int(idx.abs().max()) == 0
    assert torch.equal(w, torch.tensor([1.0, 0.0, 0.0], device=DEV).expand(2, 37, 3))
    narrow, _, w1 = pointops.three_nn_interpolate(xyz1, src, feats[:, :, :2].contiguous())
    assert torch.equal(narrow, feats[:, :, :2].expand(2, 37, 2)) and torch.equal(w1, w)
    assert pointops.farthest_point_sample(xyz1, 4, np.int64(3))[:, 0].cpu().tolist() == [3, 3]
    with pytest.raises(RuntimeError, match="S = 2"):
        pointops.three_nn_interpolate(xyz1, torch.rand(2, 2, 3, device=DEV), torch.rand(2, 2, 20, device=DEV))


# ------------------------------------------------------------------------------------------------ encoder, model
def run_model(name, trace=None):
    g = golden()
    model = model_for(str(g[f"{name}_unet_type"]))
    enc = model.point_encoder
    enc.fps_start = (dev(g[f"{name}_start1"], torch.long), dev(g[f"{name}_start2"], torch.long))
    pts = dev(g[f"{name}_points"])
    with torch.no_grad():
        out = enc(pts, trace=trace)["xy"]
        heights, _ = model(input_cloud=pts)
    return out, heights


@pytest.mark.parametrize("name", ("n700", "n700u", "n1536b2", "n300"))
def test_encoder_and_heights_within_the_reference_tolerance(name):
    from tomosar2height_amd import _lib
    g = golden()
    _lib.fallback_counts(reset=True)
    trace = {}
    out, heights = run_model(name, trace)
    assert _lib.fallback_counts() == {}
    case = "n700" if name == "n700u" else name
    for k, want in (("sa1_fps", trace["sa1"]["fps_idx"]), ("sa2_fps", trace["sa2"]["fps_idx"]), ("sa1_idx", trace["sa1"]["idx"]),
                    ("sa2_idx", trace["sa2"]["idx"]), ("fp2_idx", trace["fp2"]["idx"])):
        assert np.array_equal(want.cpu().numpy(), g[f"{case}_{k}"]), k
    tile = trace["tile"]
    got = {"l3_points": trace["l3_points"], "l2_points": trace["l2_points"], "l1_points": trace["l1_points"],
           "l0_points": tile.unsort_rows(trace["l0_points"].reshape(-1, trace["l0_points"].shape[-1])),
           "plane": trace["plane"], "out": out, "heights": heights}
    for k, t in got.items():
        want, tol = pnpp_ref.ref64(g, name, k)
        err = np.abs(t.float().cpu().numpy().astype(np.float64).reshape(want.shape) - want).max()
        print(f"{name} {k}: max err {err:.3g}, tolerance {tol:.3g} (4 x ref32_dev)")
        assert err <= tol, (name, k, err, tol)


def test_whole_model_is_deterministic_loads_strictly_and_guards_its_inputs():
    from tomosar2height_amd import TomoSAR2Height, _lib
    from tomosar2height_amd.encoder import encoder_dict
    from tomosar2height_amd.encoder.pointnetpp import PointNetPlusPlus
    g = golden()
    assert encoder_dict["pointnet_plus_plus"] is PointNetPlusPlus
    _lib.fallback_counts(reset=True)
    a_out, a_h = run_model("n1536b2")
    b_out, b_h = run_model("n1536b2")
    assert torch.equal(a_out, b_out) and torch.equal(a_h, b_h) and _lib.fallback_counts() == {}
    model = model_for("alto")
    enc, pts = model.point_encoder, dev(g["n1536b2_points"])
    enc.fps_start = None                                     # the reference's behaviour: a draw per level, sa1 then sa2
    with torch.no_grad():
        torch.manual_seed(3)
        c = enc(pts)["xy"]
        torch.manual_seed(3)
        d = enc(pts)["xy"]
        torch.manual_seed(4)
        e = enc(pts)["xy"]
    assert torch.equal(c, d) and not torch.equal(c, e)
    fresh = TomoSAR2Height(pnpp_ref.model_cfg("alto", g))
    assert list(fresh.point_encoder.state_dict().keys()) == [str(k) for k in g["state_keys"]]
    fresh.load_state_dict(model.state_dict(), strict=True)
    fresh = fresh.to(DEV).eval()
    fresh.point_encoder.fps_start = 0
    enc.fps_start = 0
    with torch.no_grad():
        assert torch.equal(fresh(input_cloud=pts)[0], model(input_cloud=pts)[0])
    with pytest.raises(NotImplementedError, match="BatchNorm batch statistics"):
        fresh.train()(input_cloud=pts)
    with pytest.raises(RuntimeError, match="cuda device"):
        fresh.eval()(input_cloud=pts.cpu())


def test_folded_weights_follow_the_weights():
    """The folded layers are cached per weight version: an in-place change of a running statistic is seen by the next forward."""
    g = golden()
    model = model_for("alto")
    enc, pts = model.point_encoder, dev(g["n700_points"])
    enc.fps_start = 0
    with torch.no_grad():
        a = enc(pts)["xy"].clone()
        assert enc.fp1.folded() is enc.fp1.folded()
        saved = enc.fp1.mlp_bns[2].running_mean.clone()
        enc.fp1.mlp_bns[2].running_mean.add_(0.05)
        b = enc(pts)["xy"].clone()
        enc.fp1.mlp_bns[2].running_mean.copy_(saved)
        c = enc(pts)["xy"]
    assert not torch.equal(a, b) and torch.equal(a, c)
