"""GPU: the stride-2 convolution's data and weight gradient kernels (csrc/hourglass.hip: t2h_hg_conv_s2_dgrad / _wgrad) against
float64 ``F.conv2d`` autograd on the host, and ``HGFilter(trainable=True, stem_gradients=True)`` built on them against the fixture
of the reference's own ``HGFilter`` (tests/golden/make_golden_hourglass_stem_grad.py) and the restatement under float64 autograd.

Bars.  Kernels: derived, not measured -- any summation order of n rounded products stays inside them (tests/hg_stem_ref.py,
``bars``): |dw - dw64| <= (n + 1) 2^-24 sum|x||gy| with n = B OH OW, |dbias - dbias64| <= n 2^-24 sum|gy|, |dx - dx64| <=
(m + 1) 2^-24 sum|gy||w| with m the terms of that element, evaluated elementwise in float64; with an addend, one more term and one
more rounding: (m + 2) 2^-24 (sum|gy||w| + |addend|).  Every row also prints its worst error as a multiple of the deviation of
torch's own float32 autograd on the host from float64 (``ref32_dev``; reported, not asserted).  Modules, under ``fp32``: the stem's
gradients within 4 x max|ref32 - ref64| of the reference's float64; every other gradient within 4 x the restatement's own float32
deviation from its float64 (the bars of test_hourglass_grad_gpu.py).  The ``f16x2`` leg is printed only.
"""
import numpy as np
import pytest
import torch

import hg_ref
import hg_stem_ref as sr
from conftest import load_golden
from scratch_guard import guarded_scratch
from test_hourglass_grad_gpu import cl, device_grads, host, precision

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden(sr.FIXTURE)
    return _cache["g"]


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ kernels
def kernel_run(shape):
    """Everything the kernel rows compare, computed once per shape: the device results (host copies) and the host references."""
    from tomosar2height_amd.encoder import hourglass as hg
    if shape in _cache:
        return _cache[shape]
    b, cin, h, w, cout, k, pad = shape
    x, weight, _, gy, addend = sr.kernel_case(shape)
    xd, gyd, ad = cl(x), cl(gy), cl(addend)
    wk = weight.permute(2, 3, 1, 0).contiguous().to(DEV)
    out = {"dx": hg.conv_s2_dgrad(gyd, wk, h, w, k, pad), "dx_add": hg.conv_s2_dgrad(gyd, wk, h, w, k, pad, ad)}
    out["dw"], out["dbias"] = hg.conv_s2_wgrad(xd, gyd, k, pad)
    out["dw_only"], none = hg.conv_s2_wgrad(xd, gyd, k, pad, with_bias=False)
    assert none is None
    again = {"dx": hg.conv_s2_dgrad(gyd, wk, h, w, k, pad), "dx_add": hg.conv_s2_dgrad(gyd, wk, h, w, k, pad, ad)}
    again["dw"], again["dbias"] = hg.conv_s2_wgrad(xd, gyd, k, pad)
    for key in again:
        assert torch.equal(bits(out[key]), bits(again[key])), key                  # two runs give equal bytes
    assert torch.equal(bits(out["dw"]), bits(out["dw_only"]))                      # with and without dbias
    assert tuple(out["dx"].shape) == (b, cin, h, w) and tuple(out["dw"].shape) == (k, k, cin, cout)
    got = {"dx": host(out["dx"]), "dx_add": host(out["dx_add"]), "dw": host(out["dw"].permute(3, 2, 0, 1)), "dbias": host(out["dbias"])}
    ref64 = dict(zip(("dx", "dw", "dbias"), sr.autograd_adjoints(x, weight, gy, pad, torch.float64)))
    ref32 = dict(zip(("dx", "dw", "dbias"), sr.autograd_adjoints(x, weight, gy, pad, torch.float32)))
    _cache[shape] = (got, ref64, ref32, (x, weight, gy, addend))
    return _cache[shape]


def report(shape, key, mine, want, bar, theirs):
    err = (mine.double() - want).abs()
    dev = max(sr.worst(theirs, want), 1e-300)
    print(f"conv_s2 {shape} {key}: max err {float(err.max()):.3g} = {float(err.max()) / dev:.2f} x ref32_dev ({dev:.3g}), "
          f"worst err / bar {float((err / bar.clamp_min(1e-300)).max()):.3f}, max|ref| {float(want.abs().max()):.3g}")
    return bool((err <= bar).all())


@pytest.mark.parametrize("shape", sr.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_weight_gradient_against_float64(shape):
    from tomosar2height_amd.encoder import hourglass as hg
    got, ref64, ref32, (x, weight, gy, _) = kernel_run(shape)
    _, bar_dw, bar_db, _ = sr.bars(x, weight, gy, shape[6])
    ok_w = report(shape, "dw", got["dw"], ref64["dw"], bar_dw, ref32["dw"])
    ok_b = report(shape, "dbias", got["dbias"], ref64["dbias"], bar_db, ref32["dbias"])
    assert ok_w and ok_b
    b, cin, h, w, cout, k, pad = shape
    slabs = hg.conv_s2_wgrad_partial_floats(b, h, w, cin, cout, k, pad) // ((k * k * cin + 1) * cout)
    assert slabs >= b and (slabs >= 3 * b) == (shape == (1, 4, 34, 6, 64, 3, 1))


@pytest.mark.parametrize("shape", sr.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_data_gradient_against_float64(shape):
    got, ref64, ref32, (x, weight, gy, addend) = kernel_run(shape)
    bar, _, _, m = sr.bars(x, weight, gy, shape[6])
    bar_add, _, _, _ = sr.bars(x, weight, gy, shape[6], addend)
    ok = report(shape, "dx", got["dx"], ref64["dx"], bar, ref32["dx"])
    ok_add = report(shape, "dx+addend", got["dx_add"], ref64["dx"] + addend.double(), bar_add, ref32["dx"] + addend)
    assert ok and ok_add
    # an element no tap reaches: +0 bit for bit, or the addend bit for bit
    untouched = m == 0
    assert bool(untouched.any()) == (shape in ((1, 5, 8, 10, 64, 3, 0), (2, 8, 5, 6, 64, 1, 0)))
    assert bool((bits(got["dx"])[untouched] == 0).all())
    assert torch.equal(bits(got["dx_add"])[untouched], bits(addend)[untouched])


def test_bad_arguments_are_refused_before_a_launch():
    from tomosar2height_amd import _lib
    from tomosar2height_amd.encoder import hourglass as hg
    x, gy = cl(torch.zeros(1, 3, 8, 8)), cl(torch.zeros(1, 64, 4, 4))
    torch.cuda.synchronize()
    lib = hg.load()
    lib.t2h_clear_kernel_name()
    for k, pad, cout in ((4, 1, 64), (9, 4, 64), (3, 2, 64), (3, 1, 60)):
        wk, g = torch.zeros(k, k, 3, cout, device=DEV), cl(torch.zeros(1, cout, 4, 4))
        with pytest.raises(_lib.T2HLibraryError, match=r"code -1.*no kernel for K="):
            hg.conv_s2_dgrad(g, wk, 8, 8, k, pad)
        with pytest.raises(_lib.T2HLibraryError, match=r"code -1.*no kernel for K="):
            hg.conv_s2_wgrad(x, g, k, pad)
    with pytest.raises(ValueError, match="is not the output of"):                  # the wrappers check what the C side cannot see
        hg.conv_s2_wgrad(cl(torch.zeros(1, 3, 2, 8)), gy, 7, 2)
    with pytest.raises(ValueError, match="weight expected"):
        hg.conv_s2_dgrad(gy, torch.zeros(3, 3, 3, 128, device=DEV), 8, 8, 3, 1)
    assert lib.t2h_last_kernel_name().decode() == ""                               # nothing was launched
    torch.cuda.synchronize()


def test_conv2d_stride2_is_its_kernels():
    """The public function under autograd: the forward's bytes are ``conv_s2``'s, the gradients the raw entries', in the
    parameter's own [Cout, Cin, K, K] shape; an input that needs no gradient gets none."""
    from tomosar2height_amd.encoder import hourglass as hg
    shape = (2, 3, 18, 22, 64, 7, 3)
    x, weight, bias, gy, _ = sr.kernel_case(shape)
    xd, gyd = cl(x).requires_grad_(True), cl(gy)
    wd, bd = weight.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    y = hg.conv2d_stride2(xd, wd, bd, padding=3)
    y.backward(gyd)
    wk = weight.permute(2, 3, 1, 0).contiguous().to(DEV)
    assert torch.equal(bits(y.detach()), bits(hg.conv_s2(xd.detach(), wk, bd.detach(), 7, 3)))
    dw, db = hg.conv_s2_wgrad(xd.detach(), gyd, 7, 3)
    assert tuple(wd.grad.shape) == (64, 3, 7, 7) and torch.equal(wd.grad, dw.permute(3, 2, 0, 1)) and torch.equal(bd.grad, db)
    assert torch.equal(bits(xd.grad), bits(hg.conv_s2_dgrad(gyd, wk, 18, 22, 7, 3)))
    frozen = weight.to(DEV)
    x2 = cl(x).requires_grad_(True)
    hg.conv2d_stride2(x2, frozen, None, padding=3).backward(gyd)
    assert torch.equal(bits(x2.grad), bits(xd.grad)) and frozen.grad is None


# ------------------------------------------------------------------------------------------------ modules
def fixture_case(name):
    from tomosar2height_amd.encoder import hourglass
    seed = int(golden()[f"{name}_seed"])
    if name not in _cache:
        _cache[name] = hg_ref.init_hg_(sr.build(hourglass, name, trainable=True, stem_gradients=True), seed).to(DEV)
    return _cache[name], sr.case_input(name, seed), sr.case_cotangent(name, seed), seed


def restated(name):
    """The restatement's float64 and float32 gradients of the case on the host, computed once."""
    key = (name, "restated")
    if key not in _cache:
        module, _, _, seed = fixture_case(name)
        _cache[key] = tuple(sr.restated_grads(name, module, seed, dt) for dt in (torch.float64, torch.float32))
    return _cache[key]


def stem_errors(name):
    """{gradient: (error, bar)} of a fixture case under the conv precision in force: the stem against the reference's float64
    (4 x ref32_dev), everything behind it against the restatement's float64 (4 x its float32 deviation).  The step runs in
    ``train()`` and in ``eval()``: equal bytes; the graph forward's output is the inference output bit for bit."""
    from tomosar2height_amd import grid
    g = golden()
    module, x, c, _ = fixture_case(name)
    r64, r32 = restated(name)
    before = grid.fallback_count()
    got, out = device_grads(module.train(), x, c)
    again, out2 = device_grads(module.eval(), x, c)
    with torch.no_grad():
        plain = module(x.to(DEV))
    assert grid.fallback_count() == before
    assert sorted(got) == sorted(str(k) for k in g[f"{name}_all_names"]) == sorted(again) == sorted(r64)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(out), bits(plain)) and plain.grad_fn is None
    assert all(torch.equal(bits(got[k]), bits(again[k])) for k in got) and all(bool(torch.isfinite(v).all()) for v in got.values())
    stem = {str(k) for k in g[f"{name}_names"]}
    errors = {}
    for key, mine in got.items():
        if key in stem:
            want, tol = hg_ref.ref64(g, name, key)
            errors[key] = (sr.worst(mine.numpy(), want), tol)
        else:
            errors[key] = (sr.worst(mine.numpy(), r64[key].numpy()), 4 * sr.worst(r32[key].numpy(), r64[key].numpy()))
    return errors, stem


@pytest.mark.parametrize("name", tuple(sr.CASES))
def test_stem_gradients_within_the_reference_tolerance(name):
    with precision("fp32"):
        errors, stem = stem_errors(name)
    for key, (err, bar) in errors.items():
        print(f"{name} fp32 d/d{key} ({'stem, 4 x ref32_dev' if key in stem else '4 x restated float32 dev'}): err {err:.3g}, bar {bar:.3g}, "
              f"multiple of the bar {err / bar:.2f}")
    assert {"input", "conv1.weight", "conv1.bias", "bn1.weight", "conv2.conv1.weight"} <= stem
    assert ("down_conv2.weight" in stem) == (name == "stem_c128")
    bad = {k: v for k, v in errors.items() if not v[0] <= v[1]}
    assert not bad, (name, bad)


def test_default_split_precision_stem_gradients_are_reported():
    """No bar under ``f16x2`` (as test_hourglass_grad_gpu.py): printed as multiples of the fp32 leg's bars."""
    with precision("f16x2"):
        report_ = {name: stem_errors(name)[0] for name in sr.CASES}
    for name, errors in report_.items():
        for key, (err, bar) in errors.items():
            print(f"{name} f16x2 d/d{key}: err {err:.3g}, multiple of the bar {err / bar:.2f}")
        worst_key = max(errors, key=lambda k: errors[k][0] / errors[k][1])
        print(f"{name} f16x2: worst multiple {errors[worst_key][0] / errors[worst_key][1]:.2f} (d/d{worst_key})")


def launches(module, x, c, input_grad):
    """{kernel: launches} of the stride-2 convolution's three kernels over one forward + backward (the launch notes)."""
    from tomosar2height_amd import _lib
    with _lib.KernelTimeline() as tl:
        got, _ = device_grads(module, x, c, input_grad)
    torch.cuda.synchronize()
    names = [r[5] for r in tl.records]
    return {k: names.count(k) for k in ("conv_s2_kernel", "conv_s2_dgrad_kernel", "conv_s2_wgrad_kernel")}, got


def test_only_the_gradients_that_are_needed_are_launched():
    with precision("fp32"):
        for name, down in (("stem_ave", 0), ("stem_c128", 1)):
            module, x, c, _ = fixture_case(name)
            full, got_full = launches(module, x, c, True)
            assert full == {"conv_s2_kernel": 1 + down, "conv_s2_dgrad_kernel": 1 + down, "conv_s2_wgrad_kernel": 1 + down}
            no_image, got = launches(module, x, c, False)                           # the usual case: the image needs no gradient
            assert no_image == {"conv_s2_kernel": 1 + down, "conv_s2_dgrad_kernel": down, "conv_s2_wgrad_kernel": 1 + down}
            assert "input" not in got and all(torch.equal(bits(got[k]), bits(got_full[k])) for k in got)
            module.conv1.requires_grad_(False)                                      # a user-frozen conv1: no gradient, no launch
            try:
                frozen, got = launches(module, x, c, False)
                assert frozen == {"conv_s2_kernel": 1 + down, "conv_s2_dgrad_kernel": down, "conv_s2_wgrad_kernel": down}
                assert module.conv1.weight.grad is None and module.conv1.bias.grad is None and "conv1.weight" not in got
                assert torch.equal(bits(got["bn1.weight"]), bits(got_full["bn1.weight"])) and module.bn1.weight.grad is not None
            finally:
                module.conv1.requires_grad_(True)


def test_switched_off_the_stem_stays_frozen_on_the_device():
    from tomosar2height_amd.encoder import hourglass
    module, x, c, seed = fixture_case("stem_ave")
    off = hg_ref.init_hg_(sr.build(hourglass, "stem_ave", trainable=True), seed).to(DEV)
    with pytest.raises(NotImplementedError, match=r"conv1\.weight, conv1\.bias.*stride-2"):
        off(x.to(DEV))
    off.conv1.requires_grad_(False)
    with precision("fp32"):
        got_off, out_off = device_grads(off, x, c, False)
        got_on, out_on = device_grads(module, x, c, False)
    assert torch.equal(bits(out_off), bits(out_on)) and "conv1.weight" not in got_off
    assert all(torch.equal(bits(got_off[k]), bits(got_on[k])) for k in got_off)      # the same graph behind conv1


def test_stem_backward_over_poisoned_guarded_scratch():
    from tomosar2height_amd import grid
    from tomosar2height_amd.encoder import hourglass as hg
    module, x, c, _ = fixture_case("stem_c128")
    with precision("fp32"):
        clean, out = device_grads(module, x, c)
        before = grid.fallback_count()
        with guarded_scratch("nan", ("cuda",)) as guard:
            got, out2 = device_grads(module, x, c)
        assert guard.damaged() == [] and grid.fallback_count() == before
    sites = [(e[1], e[5]) for e in guard.log if e[0] == "ws" and "(conv_s2_wgrad)" in e[5]]
    want = sorted(4 * hg.conv_s2_wgrad_partial_floats(*s) for s in ((2, 16, 16, 3, 64, 7, 3), (2, 8, 8, 128, 128, 3, 1)))
    assert sorted(n for n, _ in sites) == want and all("hourglass.py" in s for _, s in sites)
    assert torch.equal(bits(out), bits(out2)) and sorted(got) == sorted(clean)
    for key in clean:
        assert torch.equal(bits(got[key]), bits(clean[key])), key
