"""GPU: the resamplers against the float64 restatement of tests/resample_ref.py, through ``_lib.call`` on the raw entry points so
that rectangular planes, one-pixel planes and downsampling are reachable:

    t2h_upsample_bicubic_fwd / _bwd                          (csrc/bicubic.hip; the hourglass encoder's up path and its adjoint)
    t2h_upsample_bilinear_fwd / _bwd and the _nhwc_ pair     (csrc/raster.hip, csrc/grid_fused.hip)
    t2h_sample_bicubic_fwd / _bwd, t2h_sample_nearest_fwd / _bwd

Bars: derived in resample_ref.py (source coordinate, coefficient evaluation, rounded sums), evaluated elementwise in float64;
tests/test_resample_cpu.py shows that ATen's float32 code meets them and that the usual mistakes do not.  Every operand and every
output lives inside a banded buffer of tests/scratch_guard.py: outputs start as NaN and none may remain, and a write outside a
buffer fails the test.  Every row prints ``resample-ratio <entry point> <case> <worst error / bar>`` (reported, not a threshold).
"""
import numpy as np
import pytest
import torch

import resample_ref as rr
from scratch_guard import guarded_scratch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ids = lambda s: "x".join(map(str, s))      # noqa: E731
_cache = {}


# ------------------------------------------------------------------------------------------------ banded operands
def room(n):
    """``max(n, 1)`` floats inside guard bands (call inside ``guarded_scratch(fill="nan")``: they start as NaN)."""
    from tomosar2height_amd import _lib
    n = max(int(n), 1)
    return _lib.workspace(4 * n, DEV).view(torch.float32)[:n]


def put(a):
    buf = room(a.size)
    if a.size:
        buf[:a.size].copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel()))
    return buf


def to_memory(a, cl):
    """[B, C, h, w] -> the array in memory order (NHWC when ``cl``)."""
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if cl else np.ascontiguousarray(a)


def from_memory(buf, shape, cl):
    b, c, h, w = shape
    a = buf[:b * c * h * w].cpu().numpy()
    return a.reshape(b, h, w, c).transpose(0, 3, 1, 2) if cl else a.reshape(b, c, h, w)


def call(name, *args):
    from tomosar2height_amd import _lib
    _lib.call(name, *args, _lib.stream())


def ptr(t):
    return t.data_ptr() if t is not None else None


def report(entry, case, got, want, bar):
    assert not np.isnan(got).any(), f"{entry} {case}: an output element was never written"
    ratio = rr.worst_ratio(got, want, bar)
    print(f"resample-ratio {entry} {case} {ratio:.4f}")
    return ratio


def upsample_reference(shape, kind, channels):
    key = (shape, kind, channels)
    if key not in _cache:
        x, g, addend = rr.case(shape, channels)
        h, w, hh, ww = shape
        ay, ax = rr.rows(rr.source_coords(h, hh), h, kind), rr.rows(rr.source_coords(w, ww), w, kind)
        y = rr.upsample(x, ay, ax)
        _cache[key] = dict(x=x, g=g, addend=addend, y=y, y_add=y + addend.astype(np.float64), gx=rr.upsample_adjoint(g, ay, ax),
                           bar=rr.upsample_bar(x, shape, kind), bar_add=rr.upsample_bar(x, shape, kind, addend),
                           bar_gx=rr.upsample_adjoint_bar(g, shape, kind))
    return _cache[key]


def run_upsample(entry, shape, channels, cl, with_addend, extra=()):
    """Forward of ``entry`` on the case of (shape, channels) in the given memory layout -> [B, C, H, W] host array."""
    h, w, hh, ww = shape
    ref = upsample_reference(shape, "cubic" if "bicubic" in entry else "linear", channels)
    with guarded_scratch(fill="nan"):
        x = put(to_memory(ref["x"], cl))
        addend = put(to_memory(ref["addend"], cl)) if with_addend else None
        out = room(rr.B * channels * hh * ww)
        call(entry, ptr(x), ptr(addend), rr.B, channels, h, w, hh, ww, *extra, ptr(out))
        got = from_memory(out, (rr.B, channels, hh, ww), cl)
    return got


def run_upsample_adjoint(entry, shape, channels, cl, extra=()):
    """Adjoint of ``entry``, run twice into two buffers (equal bits asserted) -> [B, C, h, w] host array."""
    h, w, hh, ww = shape
    ref = upsample_reference(shape, "cubic" if "bicubic" in entry else "linear", channels)
    with guarded_scratch(fill="nan"):
        g = put(to_memory(ref["g"], cl))
        first, second = room(rr.B * channels * h * w), room(rr.B * channels * h * w)
        call(entry, ptr(g), rr.B, channels, h, w, hh, ww, *extra, ptr(first))
        call(entry, ptr(g), rr.B, channels, h, w, hh, ww, *extra, ptr(second))
        assert torch.equal(first.view(torch.int32), second.view(torch.int32)), f"{entry} {shape}: two runs differ"
        got = from_memory(first, (rr.B, channels, h, w), cl)
    return got


# ------------------------------------------------------------------------------------------------ bicubic resampler
@pytest.mark.parametrize("shape", rr.SHAPES, ids=ids)
def test_upsample_bicubic_forward_against_float64(shape):
    worst = 0.0
    for channels in rr.CHANNELS:
        ref = upsample_reference(shape, "cubic", channels)
        for cl in (0, 1):
            for with_addend in (False, True):
                got = run_upsample("t2h_upsample_bicubic_fwd", shape, channels, cl, with_addend, extra=(cl,))
                want, bar = (ref["y_add"], ref["bar_add"]) if with_addend else (ref["y"], ref["bar"])
                worst = max(worst, report("t2h_upsample_bicubic_fwd", f"{ids(shape)} C={channels} cl={cl} addend={with_addend}",
                                          got, want, bar))
    assert worst <= 1.0


@pytest.mark.parametrize("shape", rr.SHAPES, ids=ids)
def test_upsample_bicubic_adjoint_against_float64_and_deterministic(shape):
    worst = 0.0
    for channels in rr.CHANNELS:
        ref = upsample_reference(shape, "cubic", channels)
        for cl in (0, 1):
            got = run_upsample_adjoint("t2h_upsample_bicubic_bwd", shape, channels, cl, extra=(cl,))
            worst = max(worst, report("t2h_upsample_bicubic_bwd", f"{ids(shape)} C={channels} cl={cl}", got, ref["gx"], ref["bar_gx"]))
    assert worst <= 1.0


@pytest.mark.parametrize("cl", [0, 1])
def test_upsample_bicubic_is_exact_where_the_source_coordinate_is_a_pixel(cl):
    """4 x 4 -> 4 x 4: the scale is 1 and the coefficients are 0, 1, 0, 0, so out == in; 5 x 3 -> 9 x 5: the scale is exactly 1 / 2,
    so the even output rows and columns are the input pixels.  Bit for bit, on finite inputs."""
    for channels in rr.CHANNELS:
        x = upsample_reference((4, 4, 4, 4), "cubic", channels)["x"]
        got = run_upsample("t2h_upsample_bicubic_fwd", (4, 4, 4, 4), channels, cl, False, extra=(cl,))
        assert np.isfinite(x).all() and np.array_equal(got.view(np.int32), x.view(np.int32))
        x = upsample_reference((5, 3, 9, 5), "cubic", channels)["x"]
        got = run_upsample("t2h_upsample_bicubic_fwd", (5, 3, 9, 5), channels, cl, False, extra=(cl,))
        assert np.array_equal(np.ascontiguousarray(got[:, :, ::2, ::2]).view(np.int32), x.view(np.int32))


# ------------------------------------------------------------------------------------------------ bilinear resamplers
@pytest.mark.parametrize("shape", rr.SHAPES, ids=ids)
def test_upsample_bilinear_nchw_against_float64(shape):
    worst = 0.0
    for channels in rr.CHANNELS:
        ref = upsample_reference(shape, "linear", channels)
        for with_addend in (False, True):
            got = run_upsample("t2h_upsample_bilinear_fwd", shape, channels, 0, with_addend)
            want, bar = (ref["y_add"], ref["bar_add"]) if with_addend else (ref["y"], ref["bar"])
            worst = max(worst, report("t2h_upsample_bilinear_fwd", f"{ids(shape)} C={channels} addend={with_addend}", got, want, bar))
        got = run_upsample_adjoint("t2h_upsample_bilinear_bwd", shape, channels, 0)
        worst = max(worst, report("t2h_upsample_bilinear_bwd", f"{ids(shape)} C={channels}", got, ref["gx"], ref["bar_gx"]))
    assert worst <= 1.0


@pytest.mark.parametrize("shape", rr.SHAPES, ids=ids)
def test_upsample_bilinear_nhwc_against_float64(shape):
    worst = 0.0
    for channels in rr.BILINEAR_NHWC_CHANNELS:
        ref = upsample_reference(shape, "linear", channels)
        for with_addend in (False, True):
            got = run_upsample("t2h_upsample_bilinear_nhwc_fwd", shape, channels, 1, with_addend)
            want, bar = (ref["y_add"], ref["bar_add"]) if with_addend else (ref["y"], ref["bar"])
            worst = max(worst, report("t2h_upsample_bilinear_nhwc_fwd", f"{ids(shape)} C={channels} addend={with_addend}", got, want, bar))
        got = run_upsample_adjoint("t2h_upsample_bilinear_nhwc_bwd", shape, channels, 1)
        worst = max(worst, report("t2h_upsample_bilinear_nhwc_bwd", f"{ids(shape)} C={channels}", got, ref["gx"], ref["bar_gx"]))
    assert worst <= 1.0


def test_upsample_bilinear_nhwc_refuses_what_its_header_excludes():
    """include/t2h.h: the NHWC pair takes C % 4 == 0 only; rectangular planes are not excluded (the tests above run them)."""
    from tomosar2height_amd import _lib
    with guarded_scratch(fill="nan"):
        x, out = room(rr.B * 5 * 3 * 5), room(rr.B * 5 * 6 * 10)
        for entry, args in (("t2h_upsample_bilinear_nhwc_fwd", (ptr(x), None, rr.B, 5, 3, 5, 6, 10, ptr(out))),
                            ("t2h_upsample_bilinear_nhwc_bwd", (ptr(out), rr.B, 5, 3, 5, 6, 10, ptr(x)))):
            with pytest.raises(_lib.T2HLibraryError, match="C % 4 == 0"):
                call(entry, *args)
        torch.cuda.synchronize()
        assert bool(torch.isnan(x).all()) and bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ point samplers
def point_reference(case):
    if case not in _cache:
        r, channels, dim, n = case
        plane, pts, g = rr.point_case(case)
        near_grad, near_mag, near_count = rr.sample_nearest_adjoint(g, pts, r)
        bar_adj, _ = rr.sample_bicubic_adjoint_bar(g, pts, r)
        _cache[case] = dict(plane=plane, pts=pts, g=g, y=rr.sample_bicubic(plane, pts), bar=rr.sample_bicubic_bar(plane, pts),
                            gp=rr.sample_bicubic_adjoint(g, pts, r), bar_gp=bar_adj, near=rr.sample_nearest(plane, pts),
                            near_gp=near_grad, bar_near_gp=rr.gamma(near_count)[:, None] * near_mag)
    return _cache[case]


@pytest.mark.parametrize("case", rr.POINT_CASES, ids=ids)
def test_point_samplers_against_float64(case):
    r, channels, dim, n = case
    ref = point_reference(case)
    worst = 0.0
    for cl in (0, 1):
        tag = f"{ids(case)} cl={cl}"
        with guarded_scratch(fill="nan"):
            plane, pts, g = put(to_memory(ref["plane"], cl)), put(ref["pts"]), put(ref["g"])
            out = {mode: room(rr.B * n * channels) for mode in ("bicubic", "nearest")}
            grad = {mode: room(rr.B * channels * r * r) for mode in ("bicubic", "nearest")}
            for mode in ("bicubic", "nearest"):
                call(f"t2h_sample_{mode}_fwd", ptr(plane), ptr(pts), dim, rr.B, n, r, channels, cl, ptr(out[mode]))
                call(f"t2h_sample_{mode}_bwd", ptr(g), ptr(pts), dim, rr.B, n, r, channels, cl, ptr(grad[mode]))
            got = {mode: out[mode][:rr.B * n * channels].cpu().numpy().reshape(rr.B, n, channels) for mode in out}
            got_grad = {mode: from_memory(grad[mode], (rr.B, channels, r, r), cl) for mode in grad}
            untouched = bool(torch.isnan(out["bicubic"]).all()) and bool(torch.isnan(out["nearest"]).all())
        if n == 0:                                                       # nothing to sample: no output, an all-zero plane gradient
            assert untouched
            assert not got_grad["bicubic"].any() and not got_grad["nearest"].any()
            assert not np.signbit(got_grad["bicubic"]).any() and not np.signbit(got_grad["nearest"]).any()
            continue
        worst = max(worst, report("t2h_sample_bicubic_fwd", tag, got["bicubic"], ref["y"], ref["bar"]))
        worst = max(worst, report("t2h_sample_bicubic_bwd", tag, got_grad["bicubic"], ref["gp"], ref["bar_gp"]))
        assert not np.isnan(got["nearest"]).any()
        assert np.array_equal(got["nearest"].view(np.int32), ref["near"].view(np.int32)), f"t2h_sample_nearest_fwd {tag}"
        worst = max(worst, report("t2h_sample_nearest_bwd", tag, got_grad["nearest"], ref["near_gp"], ref["bar_near_gp"]))
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ wrappers
@pytest.mark.parametrize("hw", [(1, 1), (3, 5)], ids=ids)
def test_hourglass_upsample_add_wrapper_with_nchw_inputs(hw):
    from tomosar2height_amd.encoder import hourglass
    h, w = hw
    shape, channels = (h, w, 2 * h, 2 * w), 5
    x, g, addend = rr.case(shape, channels)
    ay, ax = rr.cubic_matrix(h, 2 * h), rr.cubic_matrix(w, 2 * w)
    xd, ad, gd = (torch.from_numpy(a).to(DEV) for a in (x, addend, g))
    xd.requires_grad_(True), ad.requires_grad_(True)
    y = hourglass._Upsample2xAdd.apply(xd, ad)
    y.backward(gd)
    fwd = report("hourglass._Upsample2xAdd", ids(shape), y.detach().cpu().numpy(), rr.upsample(x, ay, ax) + addend,
                 rr.upsample_bar(x, shape, "cubic", addend))
    bwd = report("hourglass._Upsample2xAdd.backward", ids(shape), xd.grad.cpu().numpy(), rr.upsample_adjoint(g, ay, ax),
                 rr.upsample_adjoint_bar(g, shape, "cubic"))
    assert fwd <= 1.0 and bwd <= 1.0
    assert tuple(y.shape) == (rr.B, channels, 2 * h, 2 * w) and tuple(xd.grad.shape) == tuple(xd.shape)
    assert torch.equal(ad.grad, gd)


@pytest.mark.parametrize("channels_last", [False, True])
def test_ops_bicubic_wrappers_at_three_to_six(channels_last):
    from tomosar2height_amd import ops
    shape, channels = (3, 3, 6, 6), 5
    x, g, _ = rr.case(shape, channels)
    a = rr.cubic_matrix(3, 6)
    for name, fn in (("ops.upsample_bicubic", lambda t: ops.upsample_bicubic(t, 6)),
                     ("ops.interpolate", lambda t: ops.interpolate(t, size=(6, 6), mode="bicubic", align_corners=True))):
        xd, gd = torch.from_numpy(x).to(DEV), torch.from_numpy(g).to(DEV)
        if channels_last:
            xd, gd = xd.contiguous(memory_format=torch.channels_last), gd.contiguous(memory_format=torch.channels_last)
        xd.requires_grad_(True)
        y = fn(xd)
        y.backward(gd)
        fwd = report(name, ids(shape), y.detach().cpu().numpy(), rr.upsample(x, a, a), rr.upsample_bar(x, shape, "cubic"))
        bwd = report(name + ".backward", ids(shape), xd.grad.cpu().numpy(), rr.upsample_adjoint(g, a, a),
                     rr.upsample_adjoint_bar(g, shape, "cubic"))
        assert fwd <= 1.0 and bwd <= 1.0 and tuple(y.shape) == (rr.B, channels, 6, 6)


@pytest.mark.parametrize("channels_last", [False, True])
def test_ops_grid_sample_modes_on_a_point_case(channels_last):
    from tomosar2height_amd import ops
    case = (5, 5, 2, rr.N_POINTS)
    r, channels, _, n = case
    plane, pts, g = rr.point_case(case)
    vgrid = (2.0 * pts.astype(np.float64) - 1.0).astype(np.float32)
    used = ((vgrid.astype(np.float64) + 1.0) * 0.5).astype(np.float32)          # the coordinates ops.grid_sample hands the kernels
    assert np.array_equal(used[rr.is_tie(pts, r)], pts[rr.is_tie(pts, r)])
    for mode in ("bicubic", "nearest"):
        pd = torch.from_numpy(plane).to(DEV)
        if channels_last:
            pd = pd.contiguous(memory_format=torch.channels_last)
        pd.requires_grad_(True)
        y = ops.grid_sample(pd, torch.from_numpy(vgrid).to(DEV)[:, :, None], mode=mode, padding_mode="border", align_corners=True)
        assert tuple(y.shape) == (rr.B, channels, n, 1)
        y.backward(torch.from_numpy(g).to(DEV).permute(0, 2, 1)[..., None])
        got, got_grad = y.detach()[..., 0].permute(0, 2, 1).cpu().numpy(), pd.grad.cpu().numpy()
        if mode == "bicubic":
            fwd = report("ops.grid_sample[bicubic]", ids(case), got, rr.sample_bicubic(plane, used), rr.sample_bicubic_bar(plane, used))
            bwd = report("ops.grid_sample[bicubic].backward", ids(case), got_grad, rr.sample_bicubic_adjoint(g, used, r),
                         rr.sample_bicubic_adjoint_bar(g, used, r)[0])
            assert fwd <= 1.0 and bwd <= 1.0
        else:
            assert np.array_equal(np.ascontiguousarray(got).view(np.int32), rr.sample_nearest(plane, used).view(np.int32))
            grad, mag, count = rr.sample_nearest_adjoint(g, used, r)
            assert report("ops.grid_sample[nearest].backward", ids(case), got_grad, grad, rr.gamma(count)[:, None] * mag) <= 1.0
