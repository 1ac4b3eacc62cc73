"""Device building-wise metrics (tomosar2height_amd.instances, csrc/dsm_instances.hip) against the fixture made from the
reference's scripts/evaluator_instance.py and against the numpy restatement tests/inst_ref.py.

Label planes, per-building counts and medians are compared byte for byte (any NaN equals any NaN).  The aggregates are compared
with inst_ref's float64 ones computed from the same medians to 1e-12 relative (fixed-order float64 sums of exact terms), and
with the reference's three numbers absolutely to 16 float32 ulps of the largest median, 2^-20 max|median| (sklearn works in
float32 there).  On the fixture that gap is 1.2e-7 against a bound of 2.1e-5 (printed by tests/golden/make_golden_instances.py).
"""
import numpy as np
import pytest
import torch

import inst_ref
from conftest import load_golden
from test_instances_cpu import THREE, reference_bound

pytestmark = pytest.mark.gpu

STRUCTURAL = ("corner_diagonals", "seam_lines", "u_shape", "serpentine", "spiral", "full", "empty", "checker_8x8",
              "checker_67x131", "one_pixel", "row_1x200", "col_200x1")


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def device_labels(mask, connectivity=2):
    from tomosar2height_amd import label_components
    labels, K = label_components(to_dev(mask), connectivity)
    assert labels.is_cuda and labels.dtype == torch.int32 and tuple(labels.shape) == mask.shape and isinstance(K, int)
    return labels.cpu().numpy(), K


def evaluator(mask, gt, **kw):
    from tomosar2height_amd import BuildingEvaluator
    return BuildingEvaluator(to_dev(mask), to_dev(gt), bounds=(0.0, 0.0), **kw)


def check_eval(ev, pred, gt, mask, t_row=0, l_col=0):
    """One eval against the restatement on the cropped rasters; returns (metrics, record as numpy)."""
    H, W = pred.shape
    got, rec = ev.eval(to_dev(pred), top_left=(l_col + 0.5, -t_row - 0.5))
    win = (slice(t_row, t_row + H), slice(l_col, l_col + W))
    want, labels, counts, pm, gm = inst_ref.evaluate(pred, gt[win], mask[win])
    rec = {k: v.cpu().numpy() for k, v in rec.items()}
    assert rec["labels"].tobytes() == labels.tobytes()
    assert rec["counts"].tobytes() == counts.tobytes()
    assert inst_ref.same_floats(rec["pred_median"], pm) and inst_ref.same_floats(rec["gt_median"], gm)
    inst_ref.assert_metrics(got, want)
    return got, rec


def test_fixture_case_matches_the_reference():
    g = load_golden("building_instances")
    labels, K = device_labels(g["mask"])
    assert K == 145 and labels.tobytes() == g["labels"].tobytes()
    ev = evaluator(g["mask"], g["gt"])
    for pred, suffix in ((g["pred"], ""), (g["pred64"], "64")):
        got, rec = check_eval(ev, pred, g["gt"], g["mask"])
        assert rec["labels"].tobytes() == g["labels"].tobytes()
        assert rec["pred_median"].tobytes() == g["pred" + suffix + "_median"].tobytes()
        assert rec["gt_median"].tobytes() == g["gt_median"].tobytes()
        bound = reference_bound(rec["pred_median"], rec["gt_median"])
        for key, want in zip(THREE, g["three" + suffix]):
            print(key, got[key], float(want), abs(got[key] - float(want)), bound)
            assert abs(got[key] - float(want)) <= bound, (key, got[key], float(want), bound)
        assert got["n_buildings"] == got["n_valid"] == 145 and got["n_nan"] == 0


@pytest.mark.parametrize("connectivity", (1, 2))
@pytest.mark.parametrize("name", STRUCTURAL)
def test_structural_masks(name, connectivity):
    """Tile seams on 70 x 101 = 3 x 4 ragged tiles of 32 x 32, the checkerboards that separate the two connectivities, and the
    degenerate planes: the scipy label planes of the fixture, byte for byte."""
    g = load_golden("building_instances")
    assert sorted(str(n) for n in g["structural"]) == sorted(STRUCTURAL)
    want = g[f"s_{name}_labels{connectivity}"]
    labels, K = device_labels(g[f"s_{name}"], connectivity)
    assert K == int(want.max()) and labels.tobytes() == want.tobytes()
    if name.startswith("checker"):
        assert K == (1 if connectivity == 2 else int(g[f"s_{name}"].sum()))
    if name == "full":
        assert K == 1 and (labels == 1).all()
    if name == "empty":
        assert K == 0 and not labels.any()


def test_mask_dtypes_and_refusals():
    from tomosar2height_amd import label_components
    g = load_golden("building_instances")
    want = g["labels"]
    for m in (g["mask"].astype(bool), g["mask"].astype(np.int32) * 7, g["mask"].astype(np.float32) * -2.5):
        labels, K = label_components(to_dev(m))
        assert K == 145 and labels.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="connectivity"):
        label_components(to_dev(g["mask"]), connectivity=3)


def test_more_components_than_16_bits():
    mask = np.zeros((600, 600), np.uint8)
    mask[::2, ::2] = 1
    labels, K = device_labels(mask)
    assert K == 90000
    want = np.zeros((600, 600), np.int32)
    want[::2, ::2] = np.arange(1, 90001, dtype=np.int32).reshape(300, 300)
    assert labels.tobytes() == want.tobytes()
    values = np.random.default_rng(0).standard_normal((600, 600)).astype(np.float32)
    got, rec = check_eval(evaluator(mask, values), values * 2, values, mask)
    assert (rec["counts"] == 1).all() and rec["pred_median"].tobytes() == (values * 2)[::2, ::2].tobytes()


def pack(segments, seed, width=257, dtype=np.float32):
    """A values plane and a labels plane whose segment k holds ``segments[k - 1]``, pixels in shuffled places, some background."""
    rng = np.random.default_rng(seed)
    n = sum(len(s) for s in segments)
    rows = (n + n // 7 + width) // width
    lab = np.zeros(rows * width, np.int32)
    val = rng.standard_normal(rows * width).astype(dtype)
    place = rng.permutation(rows * width)[:n]
    at = 0
    for k, s in enumerate(segments, 1):
        lab[place[at:at + len(s)]] = k
        val[place[at:at + len(s)]] = np.asarray(s, dtype)
        at += len(s)
    return val.reshape(rows, width), lab.reshape(rows, width)


def check_medians(segments, seed=0, dtype=np.float32):
    from tomosar2height_amd import segment_medians
    val, lab = pack(segments, seed, dtype=dtype)
    counts, med = segment_medians(to_dev(val), to_dev(lab), len(segments))
    want_counts, want = inst_ref.segment_medians(val, lab, len(segments))
    assert counts.cpu().numpy().tobytes() == want_counts.tobytes()
    assert [len(s) for s in segments] == want_counts.tolist()
    got = med.cpu().numpy()
    assert inst_ref.same_floats(got, want), np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:10]
    with np.errstate(invalid="ignore"):
        for s, m in zip(segments, want):                      # the restatement is numpy's median of the float32 values
            assert inst_ref.same_floats(m, np.median(np.asarray(s, dtype).astype(np.float32)))
    return got


def test_medians_every_size_class():
    """1, 2, 3; the one-wave class up to 64; the LDS sort up to 2 048; the radix select above: each threshold - 1, at it, + 1."""
    rng = np.random.default_rng(7)
    sizes = [1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 2047, 2048, 2049, 2050, 4097]
    check_medians([rng.standard_normal(n) * 10 for n in sizes], seed=1)
    check_medians([rng.integers(-3, 4, n).astype(np.float32) for n in sizes], seed=2)          # ties everywhere


def test_medians_one_large_segment_beside_thousands_of_tiny_ones():
    rng = np.random.default_rng(8)
    segments = [rng.standard_normal(int(n)) for n in rng.integers(1, 9, 1500)]
    segments.insert(700, rng.standard_normal(100000) * 5 + 20)
    segments += [rng.standard_normal(int(n)) for n in rng.integers(1, 9, 1500)] + [rng.standard_normal(5000), rng.standard_normal(3001)]
    check_medians(segments, seed=3)


def test_medians_special_values():
    rng = np.random.default_rng(9)
    inf, nan = np.inf, np.nan
    last_digit = lambda n: (np.float32(1.0) + np.arange(n, dtype=np.float32) * np.float32(2.0 ** -23))[rng.permutation(n)]
    segments = [
        np.full(5, 3.25), np.full(70, 3.25), np.full(2500, -3.25),                                # all equal
        last_digit(64), last_digit(255), last_digit(256), last_digit(4096), -last_digit(4095),    # the last key digit decides
        [-1.5, -2.5, -0.25, -7.0], -np.abs(rng.standard_normal(3000)) - 1,                        # negative
        [-0.0], [-0.0, 0.0], [0.0, -0.0, -0.0], np.where(rng.random(2600) < 0.5, -0.0, 0.0),      # signed zeros
        [inf], [-inf, inf], [-inf, -inf, 1.0], [1.0, inf, inf, 2.0], np.r_[rng.standard_normal(2100), np.full(2200, inf)],
        np.r_[rng.standard_normal(2100), np.full(2200, -inf)],
        [1.0, nan, 2.0], [nan, 1.0], [nan], np.r_[rng.standard_normal(99), nan], np.r_[rng.standard_normal(100), -nan],   # odd / even
        np.r_[rng.standard_normal(2999), nan], np.r_[rng.standard_normal(3000), nan], np.r_[np.full(2500, inf), nan],
    ]
    got = check_medians(segments, seed=4)
    assert np.nonzero(np.isnan(got))[0].tolist() == [15] + list(range(20, 28))                    # (-inf + inf) / 2, and the NaNs
    assert got[10:14].view(np.uint32).tolist() == [0, 0, 0, 0]                                    # +0, as numpy's mean


def test_medians_float64_input_rounds_to_float32_first():
    rng = np.random.default_rng(10)
    tie = [1.0 + 2.0 ** -25, 1.0 - 2.0 ** -26, 1.0, 5.0, -5.0]               # three values that are 1.0f: the median is exact 1
    segments = [tie, 1.0 + rng.standard_normal(64) * 1e-9, 1.0 + rng.standard_normal(300) * 1e-9,
                1.0 + rng.standard_normal(3000) * 1e-9, rng.standard_normal(2049) * 100]
    got = check_medians(segments, seed=5, dtype=np.float64)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == 1.0 and got[3] == 1.0


def test_nan_buildings_are_counted_and_excluded():
    g = load_golden("building_instances")
    pred, gt = g["pred"].copy(), g["gt"].copy()
    labels = g["labels"]
    sizes = np.bincount(labels.ravel())
    odd, even = int(np.nonzero((sizes % 2 == 1) & (sizes > 2))[0][1]), int(np.nonzero((sizes % 2 == 0) & (sizes > 2))[0][1])
    pred[tuple(np.argwhere(labels == odd)[1])] = np.nan
    gt[tuple(np.argwhere(labels == even)[0])] = np.nan
    got, rec = check_eval(evaluator(g["mask"], gt), pred, gt, g["mask"])
    assert got["n_nan"] == 2 and got["n_valid"] == 143 and got["n_buildings"] == 145
    assert np.isnan(rec["pred_median"][odd - 1]) and np.isnan(rec["gt_median"][even - 1])
    pred[g["mask"] != 0] = np.nan                                                                 # no valid building at all
    got, _ = check_eval(evaluator(g["mask"], gt), pred, gt, g["mask"])
    assert got["n_valid"] == 0 and got["n_nan"] == 145 and got["RMSE-B"] is None and got["MedAE-B"] is None


def test_windows_cache_and_refusals():
    from tomosar2height_amd import BuildingEvaluator
    g = load_golden("building_instances")
    t_row, l_col, H, W = (int(v) for v in g["window"])
    pred = np.ascontiguousarray(g["pred"][t_row:t_row + H, l_col:l_col + W])
    ev = BuildingEvaluator(to_dev(g["mask"]), to_dev(g["gt"]), bounds=(100.0, 50.0), pixel_size=(0.5, 0.5))
    top_left = (100.0 + 0.5 * l_col + 0.1, 50.0 - 0.5 * t_row - 0.1)
    assert ev.window(top_left) == (l_col, t_row)
    first, rec = ev.eval(to_dev(pred), top_left=top_left)
    assert rec["labels"].cpu().numpy().tobytes() == g["labels_window"].tobytes()
    assert rec["pred_median"].cpu().numpy().tobytes() == g["pred_median_window"].tobytes()
    assert rec["gt_median"].cpu().numpy().tobytes() == g["gt_median_window"].tobytes()
    for key, want in zip(THREE, g["three_window"]):
        assert abs(first[key] - float(want)) <= reference_bound(g["pred_median_window"], g["gt_median_window"]), key
    ev0 = evaluator(g["mask"], g["gt"])
    a, rec_a = check_eval(ev0, pred, g["gt"], g["mask"], t_row, l_col)
    assert a == first
    other = np.ascontiguousarray(g["pred"][3:3 + 50, 60:60 + 97])
    check_eval(ev0, other, g["gt"], g["mask"], 3, 60)
    b, rec_b = check_eval(ev0, pred, g["gt"], g["mask"], t_row, l_col)                            # the first window again
    assert b == a and rec_b["gt_median"].tobytes() == rec_a["gt_median"].tobytes() and len(ev0._windows) == 2
    cached, _ = ev0.eval(to_dev(pred), top_left=(l_col + 0.5, -t_row - 0.5))
    assert ev0.buildings(t_row, l_col, H, W)[3] is ev0.buildings(t_row, l_col, H, W)[3] and cached == a
    R, C = g["mask"].shape
    target = torch.zeros(8, 8, dtype=torch.float64, device=dev())
    ev0.eval(target, top_left=(C - 8 + 0.5, -(R - 8) - 0.5))                                      # the last window that fits
    for top_left in ((C - 7 + 0.5, -0.5), (0.5, -(R - 7) - 0.5), (-0.5, -0.5), (0.5, 0.5)):
        with pytest.raises(ValueError, match="not inside"):
            ev0.eval(target, top_left=top_left)
    empty, rec = evaluator(np.zeros((9, 11), np.uint8), g["gt"][:9, :11]).eval(to_dev(g["pred"][:9, :11]))
    assert empty == {"RMSE-B": None, "MAE-B": None, "MedAE-B": None, "max_abs": None, "n_buildings": 0, "n_valid": 0, "n_nan": 0}
    assert rec["counts"].numel() == 0 and not rec["labels"].any()


def berlin_case():
    """The Berlin test chunk's shape with a synthetic footprint: rectangles, L-shapes and salt."""
    rng = np.random.default_rng(22)
    H, W = 1660, 1990
    mask = np.zeros((H, W), np.uint8)
    for i in range(2500):
        y, x, h, w = rng.integers(0, H - 60), rng.integers(0, W - 60), rng.integers(6, 50), rng.integers(6, 50)
        mask[y:y + h, x:x + w] = 1
        if i % 3 == 0:
            mask[y + h // 2:y + h, x + w // 2:x + w] = 0                                          # an L
    mask[rng.random((H, W)) < 0.002] = 1
    gt = ((rng.standard_normal((H, W)) * 3 + 15) * mask).astype(np.float32)
    pred = gt.astype(np.float64) + rng.standard_normal((H, W)) * 1.7 + 0.3
    pred[rng.random((H, W)) < 1e-5] = np.nan
    return pred, gt, mask


def test_berlin_chunk_shape_and_run_to_run_identity():
    pred, gt, mask = berlin_case()
    ev = evaluator(mask, gt)
    first, rec = check_eval(ev, pred, gt, mask)
    assert first["n_buildings"] > 3000 and first["n_nan"] > 0 and rec["counts"].max() > 2048
    again, rec2 = evaluator(mask, gt).eval(to_dev(pred))
    assert again == first
    for key in rec:
        assert rec2[key].cpu().numpy().tobytes() == rec[key].tobytes(), key


def test_mosaic_feeds_the_building_evaluator():
    """The mosaic of test_mosaic_accumulate_finalize_vs_oracle (model=None, random 64 x 64 tiles, uncovered pixels NaN) goes
    straight into eval: a building that reaches an uncovered pixel has a NaN median and drops out."""
    from tomosar2height_amd import BuildingEvaluator, _lib
    from tomosar2height_amd.generator import DSMGenerator
    d = dev()
    gen = DSMGenerator(model=None, device=d, tiles=[], bounds=(0.0, 0.0, 160.0, 130.0), patch_size=(64.0, 64.0))
    g = torch.Generator().manual_seed(0)
    tiles = [(torch.randn(1, 64, 64, 1, generator=g) * 20, t, l) for t, l in ((0, 0), (0, 32), (32, 0), (32, 32), (60, 96), (66, 40))]
    dsm = torch.zeros(gen.dsm_shape, dtype=torch.float64, device=d)
    weight = torch.zeros_like(dsm)
    for h, t, l in tiles:
        gen.accumulate(dsm, weight, h.to(d), t, l)
    _lib.call("t2h_mosaic_finalize", _lib.ptr(dsm), _lib.ptr(weight), dsm.numel(), _lib.stream())
    rng = np.random.default_rng(2)
    gt = (rng.standard_normal((150, 170)) * 5 + 10).astype(np.float32)
    mask = np.zeros((150, 170), np.uint8)
    for _ in range(30):
        y, x = rng.integers(0, 140), rng.integers(0, 160)
        mask[y:y + rng.integers(2, 12), x:x + rng.integers(2, 12)] = 1
    ev = BuildingEvaluator(to_dev(mask), to_dev(gt), bounds=(-4.0, 140.0))
    got, rec = ev.eval(dsm, top_left=(gen.l_bound, gen.t_bound))                                 # rows 10.., cols 4..
    host = dsm.cpu().numpy()
    H, W = host.shape
    want, labels, counts, pm, gm = inst_ref.evaluate(host, gt[10:10 + H, 4:4 + W], mask[10:10 + H, 4:4 + W])
    assert rec["labels"].cpu().numpy().tobytes() == labels.tobytes() and rec["counts"].cpu().numpy().tobytes() == counts.tobytes()
    assert inst_ref.same_floats(rec["pred_median"].cpu().numpy(), pm) and inst_ref.same_floats(rec["gt_median"].cpu().numpy(), gm)
    inst_ref.assert_metrics(got, want)
    assert 0 < got["n_nan"] < got["n_buildings"]
