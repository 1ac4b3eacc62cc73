"""Device DSM evaluator (tomosar2height_amd.evaluator, csrc/dsm_eval.hip) against the numpy restatement tests/eval_ref.py,
and against the reference's own outputs for the fixture case.  Tolerances: order statistics, extrema, counts and the residual
plane are exact (selections and single float64 operations); MAE / RMSE to rtol 1e-12 (float64 sums of non-negative terms,
at most 2 048 sequential terms per thread plus a tree)."""
import numpy as np
import pytest
import torch

import eval_ref
from conftest import load_golden
from test_evaluator_cpu import fixture_masks, fixture_stats

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def run(target, gt, gt_mask=None, other=None, t_row=0, l_col=0, check=True):
    """One evaluator + eval on the device for numpy inputs; compared with the restatement unless ``check`` is False."""
    from tomosar2height_amd import DSMEvaluator
    d = dev()
    ev = DSMEvaluator(torch.from_numpy(gt).to(d), bounds=(0.0, 0.0), pixel_size=(1.0, 1.0),
                      gt_mask=None if gt_mask is None else torch.from_numpy(gt_mask).to(d),
                      other_masks=None if other is None else {k: torch.from_numpy(v).to(d) for k, v in other.items()})
    stats, diff = ev.eval(torch.from_numpy(target).to(d), top_left=(l_col + 0.5, -t_row - 0.5))
    assert diff.is_cuda and diff.dtype == torch.float64
    if check:
        want, want_diff = eval_ref.evaluate(target, gt, gt_mask, other, t_row, l_col)
        eval_ref.assert_stats(stats, want)
        eval_ref.assert_diff(diff.cpu().numpy(), want_diff)
    return stats, diff, ev


def test_fixture_case_matches_the_reference():
    from tomosar2height_amd import DSMEvaluator
    g = load_golden("dsm_evaluator")
    d = dev()
    left, top, px, py = (float(v) for v in g["geo"])
    masks = {k: torch.from_numpy(v).to(d) for k, v in fixture_masks(g).items()}
    ev = DSMEvaluator(torch.from_numpy(g["gt"]).to(d), bounds=(left, top), pixel_size=(px, py),
                      gt_mask=torch.from_numpy(g["gt_mask"]).to(d), other_masks=masks)
    assert ev.has_binary_building and ev.has_ternary_building
    assert ev.window(tuple(g["top_left"])) == (int(g["window"][1]), int(g["window"][0]))
    stats, diff = ev.eval(torch.from_numpy(g["target"]).to(d), top_left=tuple(g["top_left"]))
    eval_ref.assert_stats(stats, fixture_stats(g))
    eval_ref.assert_diff(diff.cpu().numpy(), g["diff"])


@pytest.mark.parametrize("odd", (True, False))
@pytest.mark.parametrize("kind", ("six_values", "one_value"))
def test_ties(kind, odd):
    rng = np.random.default_rng(3)
    H, W = 33, 31                                                    # 1 023 pixels: odd; one knocked out: even
    if kind == "six_values":
        target = rng.choice(np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0]) * 0.25, size=(H, W))
    else:
        target = np.full((H, W), -0.375)
    gt = np.zeros((H, W))
    gt_mask = np.ones((H, W), bool)
    if not odd:
        gt_mask[17, 5] = False
    other = {"a": rng.random((H, W)) < 0.5, "b": rng.random((H, W)) < 0.11}
    stats, _, _ = run(target, gt, gt_mask, other)
    assert stats["overall"]["n_pixel"] == (1023 if odd else 1022)


def test_last_digit_decides_and_full_range():
    rng = np.random.default_rng(5)
    k = np.arange(4096, dtype=np.float64)
    v = np.concatenate([1.0 + k * 2.0 ** -52, -(1.0 + k * 2.0 ** -52)])
    rng.shuffle(v)
    target = v.reshape(64, 128)
    gt = np.zeros_like(target)
    other = {"positive": target > 0, "negative": target < 0, "some": rng.random(target.shape) < 0.37,
             "odd_count": (target > 0) & (target != 1.0)}
    stats, _, _ = run(target, gt, None, other)
    assert stats["positive"]["n_pixel"] == 4096 and stats["odd_count"]["n_pixel"] == 4095
    wide = np.array([1e300, -1e300, 3e300, -2e300, 1e-300, -1e-300, 5e-324, -5e-324, 1.5e-310, -2.5e-310, 0.0, -0.0, 1.0, -1.0,
                     2.2250738585072014e-308, 1.7e308, 123.456, -7.0, 4e-320, -4e-320, 6.02e23])
    rng.shuffle(wide)
    target = wide.reshape(3, 7)
    other = {"tiny": np.abs(target) < 1e-200, "huge": np.abs(target) > 1e200, "rest": rng.random(target.shape) < 0.5}
    run(target, np.zeros_like(target), None, other)


@pytest.mark.parametrize("shape", ((1, 1), (1, 257), (257, 1)))
@pytest.mark.parametrize("dtypes", ((np.float64, np.float32), (np.float32, np.float64), (np.float32, np.float32)))
def test_degenerate_planes(shape, dtypes):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    target = (rng.standard_normal(shape) * 3).astype(dtypes[0])
    gt = rng.standard_normal(shape).astype(dtypes[1])
    n = shape[0] * shape[1]
    flat = lambda idx: np.isin(np.arange(n), idx).reshape(shape)
    other = {"none": flat([]), "one": flat([n // 2]), "two": flat([0, n - 1]), "type": rng.integers(0, 3, shape).astype(np.int32)}
    stats, _, _ = run(target, gt, None, other)
    assert stats["none"]["n_pixel"] is None and stats["one"]["n_pixel"] == 1
    assert stats["two"]["n_pixel"] == (2 if n > 1 else 1)


def test_all_nan_target():
    target = np.full((9, 11), np.nan)
    gt = np.ones((9, 11), np.float32)
    stats, diff, _ = run(target, gt, None, {"building": np.ones((9, 11), np.uint8)})
    assert list(stats) == ["overall", "building", "terrain"]
    assert all(v is None for row in stats.values() for v in row.values())
    assert torch.isnan(diff).all()


def test_many_workgroups_sixteen_classes():
    rng = np.random.default_rng(11)
    R, C, H, W = 640, 720, 600, 700
    gt = (rng.standard_normal((R, C)) * 10 + 40).astype(np.float32)
    target = gt[13:13 + H, 9:9 + W].astype(np.float64) + rng.standard_normal((H, W)) * 2
    target[rng.random((H, W)) < 0.03] = np.nan
    gt_mask = rng.random((R, C)) < 0.95
    other = {f"c{i}": rng.random((R, C)) < p for i, p in enumerate(np.linspace(0.02, 0.9, 15))}
    stats, _, ev = run(target, gt, gt_mask, other, t_row=13, l_col=9)
    assert len(ev.class_names) == 16 and len(stats) == 16


def berlin_case():
    """The Berlin test chunk's shape with the seven Berlin classes from a synthetic footprint: rectangles of two types."""
    rng = np.random.default_rng(21)
    H, W = 1660, 1990
    type_plane = np.zeros((H, W), np.uint8)
    for _ in range(900):
        y, x, h, w = rng.integers(0, H - 40), rng.integers(0, W - 40), rng.integers(6, 40), rng.integers(6, 40)
        type_plane[y:y + h, x:x + w] = rng.integers(1, 3)
    building = (type_plane > 0).astype(np.uint8)
    gt = (rng.standard_normal((H, W)) * 6 + 20).astype(np.float32) * (1 + building)
    target = gt.astype(np.float64) + rng.standard_normal((H, W)) * 1.7 + 0.3 * building
    target[rng.random((H, W)) < 0.01] = np.nan
    return target, gt, {"building": building, "type": type_plane}


def test_berlin_chunk_shape_and_run_to_run_identity():
    target, gt, other = berlin_case()
    stats, diff, ev = run(target, gt, None, other)
    assert list(stats) == ["overall", "building", "terrain", "non_building", "residential", "non_residential", "building_combined"]
    again, diff2 = ev.eval(torch.from_numpy(target).to(dev()), top_left=(0.5, -0.5))
    eval_ref.assert_stats(again, stats, exact_sums=True)
    assert torch.equal(diff.view(torch.int64), diff2.view(torch.int64))          # the bytes, NaNs included


def test_dilation():
    from tomosar2height_amd import dilate_mask
    g = load_golden("dsm_evaluator")
    d = dev()
    for plane in ("corners", "line", "building"):
        m = torch.from_numpy(g[plane].astype(bool)).to(d)
        assert tuple(m.shape) in ((67, 131), (1, 64), (90, 150))
        for k in (1, 2, 3):
            got = dilate_mask(m, iterations=k)
            assert got.is_cuda and got.dtype == torch.bool
            assert np.array_equal(got.cpu().numpy(), g[f"{plane}_dilated{k}"]), (plane, k)
            assert np.array_equal(got.cpu().numpy(), eval_ref.dilate(g[plane], k)), (plane, k)
    assert np.array_equal(dilate_mask(torch.from_numpy(g["corners"]).to(d)).cpu().numpy(), g["corners_dilated1"])   # default 1


def test_refusals():
    from tomosar2height_amd import DSMEvaluator, dilate_mask
    d = dev()
    gt = torch.zeros(20, 30, device=d)
    ev = DSMEvaluator(gt, bounds=(100.0, 50.0))
    target = torch.zeros(8, 8, dtype=torch.float64, device=d)
    ev.eval(target, top_left=(122.0, 42.0))                                       # rows 8..16, cols 22..30: the last that fits
    for top_left in ((123.0, 42.0), (122.0, 37.0), (99.5, 42.0), (122.0, 50.5)):
        with pytest.raises(ValueError, match="not inside"):
            ev.eval(target, top_left=top_left)
    masks = {f"m{i}": torch.ones(20, 30, dtype=torch.bool, device=d) for i in range(16)}
    with pytest.raises(ValueError, match="17 classes"):
        DSMEvaluator(gt, bounds=(0.0, 0.0), other_masks=masks)
    masks.pop("m0")
    assert len(DSMEvaluator(gt, bounds=(0.0, 0.0), other_masks=masks).class_names) == 16
    for it in (0, -1):
        with pytest.raises(ValueError, match="iterations"):
            dilate_mask(torch.ones(4, 4, dtype=torch.bool, device=d), iterations=it)


def test_mosaic_feeds_the_evaluator():
    """The mosaic of test_mosaic_accumulate_finalize_vs_oracle (model=None, random 64 x 64 tiles, uncovered pixels NaN) goes
    straight into eval: the uncovered pixels drop out of every class."""
    from tomosar2height_amd import DSMEvaluator, _lib
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
    other = {"building": (rng.random((150, 170)) < 0.05).astype(np.uint8), "type": rng.integers(0, 3, (150, 170)).astype(np.uint8)}
    ev = DSMEvaluator(torch.from_numpy(gt).to(d), bounds=(-4.0, 140.0), other_masks={k: torch.from_numpy(v).to(d) for k, v in other.items()})
    stats, diff = ev.eval(dsm, top_left=(gen.l_bound, gen.t_bound))              # rows 10.., cols 4..
    host = dsm.cpu().numpy()
    covered = int((~np.isnan(host)).sum())
    assert 0 < covered < host.size and stats["overall"]["n_pixel"] == covered
    want, want_diff = eval_ref.evaluate(host, gt, None, other, t_row=10, l_col=4)
    eval_ref.assert_stats(stats, want)
    eval_ref.assert_diff(diff.cpu().numpy(), want_diff)
