"""CPU: the float64 restatement of the resamplers (tests/resample_ref.py) and its bars, before any kernel is compared with them.

1.  The restatement against an independent implementation: ``F.interpolate`` (bicubic, bilinear; align_corners=True) and
    ``F.grid_sample`` (bicubic, nearest; border, align_corners=True) in float64, forward and autograd adjoint, at every case.  Bar:
    the derived bar of resample_ref.py evaluated at u = 2^-53 -- a few float64 ulps of sum|w||x| plus the coordinate term -- since
    ATen's float64 code performs the same operations; 'nearest' must agree exactly.
2.  Condition (a): ATen's own float32 result lies within the float32 bar of the float64 restatement at every case, so the bar does
    not ask a float32 kernel for more than a careful float32 implementation delivers.
3.  Condition (b): mutants of the restatement -- the mistakes a kernel of this kind makes -- exceed the bar on the named cases, so
    the bar is not too wide to notice them.
4.  The 'nearest' inputs: float32 and float64 coordinates select the same pixel at every point that is not a tie, and the ties
    are exact in float32 (so the kernel's float32 product decides them by its rounding rule and nothing else).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_ref as rr

MODE = {"cubic": "bicubic", "linear": "bilinear"}
PRECISIONS = ((torch.float64, rr.U64), (torch.float32, rr.U))
ids = lambda s: "x".join(map(str, s))      # noqa: E731
_cache = {}


def aten_upsample(x, g, shape, kind, dtype):
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    y = F.interpolate(xt, size=shape[2:], mode=MODE[kind], align_corners=True)
    y.backward(torch.from_numpy(g).to(dtype))
    return y.detach().numpy(), xt.grad.numpy()


def aten_sample(plane, pts, g, mode, dtype):
    """([B, N, C], plane gradient) of F.grid_sample at vgrid = 2 p - 1, formed in float64 (exact there) and cast."""
    pl = torch.from_numpy(plane).to(dtype).requires_grad_(True)
    grid = (2.0 * torch.from_numpy(pts[..., :2].astype(np.float64)) - 1.0).to(dtype)[:, :, None]
    y = F.grid_sample(pl, grid, mode=mode, padding_mode="border", align_corners=True)
    y.backward(torch.from_numpy(g).to(dtype).permute(0, 2, 1)[..., None])
    return y.detach()[..., 0].permute(0, 2, 1).numpy(), pl.grad.numpy()


def matrices(shape, kind):
    h, w, hh, ww = shape
    return rr.rows(rr.source_coords(h, hh), h, kind), rr.rows(rr.source_coords(w, ww), w, kind)


def restated(shape, kind, channels):
    key = (shape, kind, channels)
    if key not in _cache:
        x, g, _ = rr.case(shape, channels)
        ay, ax = matrices(shape, kind)
        _cache[key] = (x, g, rr.upsample(x, ay, ax), rr.upsample_adjoint(g, ay, ax))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ 1 and 2
@pytest.mark.parametrize("kind", ["cubic", "linear"])
@pytest.mark.parametrize("shape", rr.SHAPES, ids=ids)
def test_matrix_form_against_aten_in_float64_and_aten_float32_within_the_bar(shape, kind):
    for channels in rr.CHANNELS:
        x, g, y64, gx64 = restated(shape, kind, channels)
        for dtype, u in PRECISIONS:
            y, gx = aten_upsample(x, g, shape, kind, dtype)
            fwd = rr.worst_ratio(y, y64, rr.upsample_bar(x, shape, kind, u=u))
            bwd = rr.worst_ratio(gx, gx64, rr.upsample_adjoint_bar(g, shape, kind, u=u))
            print(f"{kind} {shape} C={channels} {dtype}: forward err / bar {fwd:.3f}, adjoint err / bar {bwd:.3f}")
            assert fwd <= 1.0 and bwd <= 1.0, (kind, shape, channels, dtype, fwd, bwd)


def test_weights_sum_to_one_and_the_exact_shapes_are_exact():
    for kind in MODE:
        for shape in rr.SHAPES:
            for m in matrices(shape, kind):
                # four float64 coefficients, each within EVAL u of its polynomial, and their sum
                assert np.abs(m.sum(axis=1) - 1.0).max() <= (sum(rr.EVAL[kind]) + 4) * rr.U64
    for kind in MODE:
        ay, ax = matrices((4, 4, 4, 4), kind)
        assert np.array_equal(ay, np.eye(4)) and np.array_equal(ax, np.eye(4))
        ay, ax = matrices((5, 3, 9, 5), kind)
        assert np.array_equal(ay[::2], np.eye(5)) and np.array_equal(ax[::2], np.eye(3))
    assert np.array_equal(rr.cubic_matrix(5, 1), np.eye(5)[:1]) and np.array_equal(rr.cubic_matrix(1, 2), np.ones((2, 1)))


@pytest.mark.parametrize("case", rr.POINT_CASES, ids=ids)
def test_samplers_against_grid_sample_in_float64_and_float32_within_the_bar(case):
    r, channels, dim, n = case
    plane, pts, g = rr.point_case(case)
    assert pts.shape == (rr.B, n, dim) and pts.dtype == np.float32
    y64, gp64 = rr.sample_bicubic(plane, pts), rr.sample_bicubic_adjoint(g, pts, r)
    for dtype, u in PRECISIONS:
        y, gp = aten_sample(plane, pts, g, "bicubic", dtype)
        fwd = rr.worst_ratio(y, y64, rr.sample_bicubic_bar(plane, pts, u=u))
        bwd = rr.worst_ratio(gp, gp64, rr.sample_bicubic_adjoint_bar(g, pts, r, u=u)[0])
        print(f"bicubic points {case} {dtype}: forward err / bar {fwd:.3f}, adjoint err / bar {bwd:.3f}")
        assert fwd <= 1.0 and bwd <= 1.0, (case, dtype, fwd, bwd)
    grad, mag, count = rr.sample_nearest_adjoint(g, pts, r)
    assert count.sum() == rr.B * n
    y, gp = aten_sample(plane, pts, g, "nearest", torch.float64)
    assert np.array_equal(y, rr.sample_nearest(plane, pts).astype(np.float64))
    assert rr.worst_ratio(gp, grad, rr.gamma(count, rr.U64)[:, None] * mag) <= 1.0
    y, gp = aten_sample(plane, pts, g, "nearest", torch.float32)        # (exact ties and exact products: see the inputs test)
    assert np.array_equal(y, rr.sample_nearest(plane, pts))
    assert rr.worst_ratio(gp, grad, rr.gamma(count)[:, None] * mag) <= 1.0


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("name, mutant, shapes", [
    ("A = -0.5", dict(a=-0.5), ((2, 2, 4, 4), (16, 16, 40, 32))),
    ("taps zero-padded instead of clamped", dict(clamp=False), ((1, 2, 2, 4), (3, 5, 6, 10))),
    ("align_corners=False source coordinates", dict(align_corners=False), ((2, 2, 4, 4), (9, 6, 3, 2))),
])
def test_bicubic_matrix_mutants_exceed_the_bar(name, mutant, shapes):
    for shape in shapes:
        h, w, hh, ww = shape
        x, g, y64, gx64 = restated(shape, "cubic", 5)
        my, mx = rr.cubic_matrix(h, hh, **mutant), rr.cubic_matrix(w, ww, **mutant)
        fwd = rr.worst_ratio(rr.upsample(x, my, mx), y64, rr.upsample_bar(x, shape, "cubic"))
        bwd = rr.worst_ratio(rr.upsample_adjoint(g, my, mx), gx64, rr.upsample_adjoint_bar(g, shape, "cubic"))
        print(f"mutant '{name}' at {shape}: forward err / bar {fwd:.3g}, adjoint err / bar {bwd:.3g}")
        assert fwd > 1.0 and bwd > 1.0, (name, shape)


@pytest.mark.parametrize("kind", ["cubic", "linear"])
@pytest.mark.parametrize("shape", [(2, 2, 4, 4), (9, 6, 3, 2), (33, 17, 66, 34)], ids=ids)
def test_adjoint_with_a_window_one_pixel_short_exceeds_the_bar(shape, kind):
    _, g, _, gx64 = restated(shape, kind, 5)
    ay, ax = matrices(shape, kind)
    bar = rr.upsample_adjoint_bar(g, shape, kind)
    rows_short = rr.worst_ratio(rr.upsample_adjoint(g, rr.adjoint_window_short(ay), ax), gx64, bar)
    cols_short = rr.worst_ratio(rr.upsample_adjoint(g, ay, rr.adjoint_window_short(ax)), gx64, bar)
    print(f"{kind} {shape}: window short along y err / bar {rows_short:.3g}, along x {cols_short:.3g}")
    assert rows_short > 1.0 and cols_short > 1.0


@pytest.mark.parametrize("r", [5, 16])
def test_samplers_with_x_and_y_swapped_exceed_the_bar(r):
    plane, pts, _ = rr.point_case((r, 5, 2, rr.N_POINTS))
    got = rr.worst_ratio(rr.sample_bicubic(plane, pts, swap=True), rr.sample_bicubic(plane, pts), rr.sample_bicubic_bar(plane, pts))
    assert got > 1.0
    assert not np.array_equal(rr.sample_nearest(plane, pts, swap=True), rr.sample_nearest(plane, pts))
    for mutant in (dict(a=-0.5), dict(clamp=False)):
        assert rr.worst_ratio(rr.sample_bicubic(plane, pts, **mutant), rr.sample_bicubic(plane, pts),
                              rr.sample_bicubic_bar(plane, pts)) > 1.0


@pytest.mark.parametrize("r", [5, 9])
def test_nearest_rounding_half_away_from_zero_differs_at_the_ties_only(r):
    plane, pts, _ = rr.point_case((r, 5, 2, rr.N_POINTS))
    tie = rr.is_tie(pts, r).any(axis=-1)
    differs = (rr.sample_nearest(plane, pts, ties="away") != rr.sample_nearest(plane, pts)).any(axis=-1)
    assert differs.any() and not (differs & ~tie).any()
    # r = 5: x = 0.125 -> 0.5 -> column 0 and x = 0.625 -> 2.5 -> column 2 (half to even); half away from zero gives 1 and 3
    if r == 5:
        two = np.array([[[0.125, 0.0], [0.625, 0.0]]], np.float32)
        assert rr.nearest_index(two, 5)[1].tolist() == [[0, 2]] and rr.nearest_index(two, 5, ties="away")[1].tolist() == [[1, 3]]


@pytest.mark.parametrize("r", [3, 16])
def test_nearest_without_the_clip_differs_at_the_outside_points_only(r):
    plane, pts, _ = rr.point_case((r, 5, 2, rr.N_POINTS))
    outside = ((pts[..., :2] < 0) | (pts[..., :2] > 1)).any(axis=-1)
    differs = (rr.sample_nearest(plane, pts, clip=False) != rr.sample_nearest(plane, pts)).any(axis=-1)
    assert differs.any() and not (differs & ~outside).any()


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("case", rr.POINT_CASES, ids=ids)
def test_nearest_inputs_round_alike_in_float32_and_ties_are_exact(case):
    r, _, dim, n = case
    pts = rr.points(r, dim, n)
    xy = pts[..., :2]
    in32 = np.clip(xy * np.float32(r - 1), np.float32(0), np.float32(r - 1))          # the kernel's float32 product, clipped
    assert in32.dtype == np.float32
    in64 = np.clip(xy.astype(np.float64) * (r - 1), 0.0, r - 1.0)
    tie = rr.is_tie(pts, r)
    assert np.array_equal(in32[tie].astype(np.float64), in64[tie])
    assert np.array_equal(np.rint(in32[~tie]).astype(np.int64), np.rint(in64[~tie]).astype(np.int64))
    assert not (np.abs(in32 - np.floor(in32) - np.float32(0.5)) == 0)[~tie].any()       # no tie appears in float32 only
    if n:
        want = {5: 16, 9: 16}.get(r, 0)                                # four points, two coordinates, two samples
        assert int(tie.sum()) == want, (r, int(tie.sum()))
        flat = [tuple(p) for p in xy[0].astype(np.float64).round(12).tolist()]
        for p in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)) + rr.OUTSIDE:
            assert tuple(np.float32(p).astype(np.float64).round(12).tolist()) in flat
        assert (xy == np.float32(rr.BELOW_ONE)).any() and rr.BELOW_ONE == 1.0 - 2.0 ** -24
        assert ((xy < 0) | (xy > 1)).any(axis=-1).sum() >= 2 * rr.B
