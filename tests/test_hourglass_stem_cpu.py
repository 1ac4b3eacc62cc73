"""CPU (no GPU needed): the ``stem_gradients`` switch of ``HGFilter`` adds no state and changes no refusal while it is off; the
header, the signature table and the scratch formula of the stride-2 convolution's adjoints agree; the restatement of the two
adjoints (tests/hg_stem_ref.py, the parity decomposition written out) reproduces float64 ``F.conv2d`` autograd; the stem fixture
(tests/golden/make_golden_hourglass_stem_grad.py) is complete and the restated filter reproduces it."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import hg_grad_ref
import hg_ref
import hg_stem_ref as sr
from abi_ref import declared_symbols
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "t2h_hg.h")
NEW_ENTRIES = ("t2h_hg_conv_s2_dgrad", "t2h_hg_conv_s2_wgrad")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden(sr.FIXTURE)
    return _cache["g"]


def restated(name, dtype):
    from tomosar2height_amd.encoder import hourglass
    key = (name, dtype)
    if key not in _cache:
        seed = int(golden()[f"{name}_seed"])
        module = hg_ref.init_hg_(sr.build(hourglass, name, trainable=True, stem_gradients=True), seed)
        _cache[key] = {k: v.numpy() for k, v in sr.restated_grads(name, module, seed, dtype).items()}
    return _cache[key]


# ------------------------------------------------------------------------------------------------ the switch
def test_the_switch_is_a_keyword_only_plain_attribute():
    from tomosar2height_amd.encoder.hourglass import HGFilter
    kw = dict(in_channel=3, feature_dim=32, num_stack=1, num_hourglass=1)
    off, on = HGFilter(**kw, trainable=True), HGFilter(**kw, trainable=True, stem_gradients=True)
    assert off.stem_gradients is False and on.stem_gradients is True and HGFilter(**kw).stem_gradients is False
    assert list(off.state_dict()) == list(on.state_dict())
    assert [k for k, _ in off.named_parameters()] == [k for k, _ in on.named_parameters()]
    assert [k for k, _ in off.named_buffers()] == [k for k, _ in on.named_buffers()]
    assert "stem_gradients" not in on._parameters and "stem_gradients" not in on._buffers and "stem_gradients" not in on._modules
    params = inspect.signature(HGFilter.__init__).parameters
    assert params["stem_gradients"].kind is inspect.Parameter.KEYWORD_ONLY and params["stem_gradients"].default is False
    with pytest.raises(TypeError):
        HGFilter(3, 32, 1, 1, "group", "ave_pool", True, True)
    # through the model's encoder2_kwargs
    from tomosar2height_amd.encoder import encoder_dict
    assert encoder_dict["hourglass"](**dict(kw, trainable=True, stem_gradients=True)).stem_gradients is True


def test_switched_on_the_trainable_forward_reaches_the_device_and_off_it_refuses_as_before():
    from tomosar2height_amd.encoder.hourglass import HGFilter
    x = torch.zeros(1, 3, 32, 32)
    for hg_down in ("ave_pool", "conv128"):
        on = HGFilter(3, 32, 1, 1, hg_down=hg_down, trainable=True, stem_gradients=True)
        with pytest.raises(RuntimeError, match="cuda device"):          # no stem refusal: the next stop is the device
            on(x)
        with pytest.raises(RuntimeError, match="cuda device"):
            on(x.clone().requires_grad_(True))
    off = HGFilter(3, 32, 1, 1, trainable=True)
    text = ("HGFilter(trainable=True) runs with a frozen stem: conv1.weight, conv1.bias require a gradient, but the stride-2 "
            "convolution's weight / data gradient is not built (conv1); call requires_grad_(False) on them")
    with pytest.raises(NotImplementedError) as err:
        off(x)
    assert str(err.value) == text
    down = HGFilter(3, 32, 1, 1, hg_down="conv128", trainable=True)
    down.conv1.requires_grad_(False)
    with pytest.raises(NotImplementedError, match=r"frozen stem: bn1\.weight, bn1\.bias, conv2\..*down_conv2\.bias require a gradient.*"
                                                  r"\(conv1, down_conv2 and what lies in front of it\)"):
        down(x)
    # consulted by the trainable forward only: without ``trainable`` the switch changes nothing
    with pytest.raises(NotImplementedError, match="inference only"):
        HGFilter(3, 32, 1, 1, stem_gradients=True)(x)
    with pytest.raises(NotImplementedError, match="norm='batch'"):
        HGFilter(3, 32, 1, 1, norm="batch", trainable=True, stem_gradients=True)(x)


def test_trainer_still_refuses_a_trainable_image_encoder():
    from tomosar2height_amd.encoder.hourglass import HGFilter
    from tomosar2height_amd.trainer import Trainer

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.image_encoder = HGFilter(3, 32, 1, 1, trainable=True, stem_gradients=True)

    class Optimizer:
        def zero_grad(self):
            pass

    with pytest.raises(NotImplementedError, match="trainable=True"):
        Trainer(Model(), Optimizer())


# ------------------------------------------------------------------------------------------------ header, table, formula
def test_header_signatures_and_the_partial_formula_agree():
    from tomosar2height_amd.encoder import hourglass
    assert sorted(hourglass.SIGNATURES) == declared_symbols(HEADER) and set(NEW_ENTRIES) <= set(hourglass.SIGNATURES)
    lib = hourglass.load()
    assert all(hasattr(lib, name) for name in NEW_ENTRIES)
    assert len(hourglass.SIGNATURES["t2h_hg_conv_s2_dgrad"][1]) == 12 and len(hourglass.SIGNATURES["t2h_hg_conv_s2_wgrad"][1]) == 13
    text = open(HEADER).read()
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(T2H_CS2_\w+)\s+(\d+)\b", text, flags=re.M)}
    assert defines == {"T2H_CS2_SLAB_ROWS": hourglass.CS2_SLAB_ROWS, "T2H_CS2_SLAB_COLS": hourglass.CS2_SLAB_COLS}
    assert re.search(r"B \* ceil\(OH / T2H_CS2_SLAB_ROWS\) \* ceil\(OW / T2H_CS2_SLAB_COLS\) \* \(K \* K \* Cin \+ 1\) \* Cout\s+floats", text)
    rows, cols = defines["T2H_CS2_SLAB_ROWS"], defines["T2H_CS2_SLAB_COLS"]
    for b, cin, h, w, cout, k, pad in sr.KERNEL_SHAPES + ((1, 3, 512, 512, 64, 7, 3), (4, 128, 256, 256, 128, 3, 1), (1, 7, 66, 130, 192, 5, 1)):
        oh, ow = (h + 2 * pad - k) // 2 + 1, (w + 2 * pad - k) // 2 + 1
        want = b * ((oh + rows - 1) // rows) * ((ow + cols - 1) // cols) * (k * k * cin + 1) * cout
        assert hourglass.conv_s2_wgrad_partial_floats(b, h, w, cin, cout, k, pad) == want, (b, cin, h, w, cout, k, pad)
    assert hourglass.conv_s2_wgrad_partial_floats(1, 34, 6, 4, 64, 3, 1) == 3 * 37 * 64          # three slabs of one sample
    # no new size query and no new T2H_HG_ constant: the scratch is the typed ``partial`` argument, taken from _lib.workspace
    src = open(os.path.join(ROOT, "tomosar2height_amd", "csrc", "hourglass.hip")).read()
    assert re.findall(r"^T2H_API\s+size_t\s+(\w+)\s*\(", src, flags=re.M) == ["t2h_hg_groupnorm_workspace_bytes"]
    assert re.findall(r"^#define\s+(T2H_HG_\w+)\s+\d+", text, flags=re.M) == ["T2H_HG_GNB_PIXELS"]
    assert "partial = _lib.workspace(" in inspect.getsource(hourglass.conv_s2_wgrad)


def test_bad_arguments_return_the_error_code_on_the_host():
    """Validation precedes any launch, so it runs without a device: non-null dummy pointers, every shape outside the domain."""
    from tomosar2height_amd.encoder import hourglass
    lib = hourglass.load()
    p = 4096
    for b, cin, h, w, cout, k, pad in sr.BAD_ARGUMENTS:
        assert lib.t2h_hg_conv_s2_dgrad(p, p, None, p, b, h, w, cin, cout, k, pad, None) == -1, (b, cin, h, w, cout, k, pad)
        assert lib.t2h_hg_conv_s2_wgrad(p, p, p, p, None, b, h, w, cin, cout, k, pad, None) == -1, (b, cin, h, w, cout, k, pad)
    assert lib.t2h_hg_conv_s2_dgrad(None, p, None, p, 1, 8, 8, 3, 64, 3, 1, None) == -1          # null gy
    assert lib.t2h_hg_conv_s2_dgrad(p, p + 4, None, p, 1, 8, 8, 3, 64, 3, 1, None) == -1         # misaligned weight
    assert lib.t2h_hg_conv_s2_wgrad(p, p, None, p, None, 1, 8, 8, 3, 64, 3, 1, None) == -1       # no partial
    assert lib.t2h_hg_conv_s2_wgrad(p, p, p + 8, p, None, 1, 8, 8, 3, 64, 3, 1, None) == -1      # misaligned partial


# ------------------------------------------------------------------------------------------------ the adjoints restated
@pytest.mark.parametrize("shape", sr.KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restated_adjoints_reproduce_float64_autograd(shape):
    b, cin, h, w, cout, k, pad = shape
    x, weight, _, gy, _ = (t.double() for t in sr.kernel_case(shape))
    dx64, dw64, db64 = sr.autograd_adjoints(x, weight, gy, pad, torch.float64)
    dx = sr.dgrad_by_parity(gy, weight, h, w, pad)
    dw, db = sr.wgrad_by_taps(x, gy, k, pad)
    for key, mine, want in (("dx", dx, dx64), ("dw", dw, dw64), ("dbias", db, db64)):
        err, scale = sr.worst(mine, want), float(want.abs().max())
        print(f"{shape} {key}: max err {err:.3g} of {scale:.3g}")
        assert err <= 1e-12 * max(scale, 1.0), (key, err)
    # an element no tap reaches is exactly +0 in both, and the term count says which those are
    _, _, _, m = sr.bars(x, weight, gy, pad)
    untouched = m == 0
    assert bool((dx[untouched] == 0).all()) and bool((dx64[untouched] == 0).all())
    assert bool(untouched.any()) == (shape in ((1, 5, 8, 10, 64, 3, 0), (2, 8, 5, 6, 64, 1, 0)))      # (K = 1: every odd pixel)
    # the float32 restatement stays inside the derived bars
    x32, w32, _, g32, _ = sr.kernel_case(shape)
    bar_dx, bar_dw, bar_db, _ = sr.bars(x32, w32, g32, pad)
    dx64, dw64, db64 = sr.autograd_adjoints(x32, w32, g32, pad, torch.float64)
    dw32, db32 = sr.wgrad_by_taps(x32, g32, k, pad)
    assert bool(((sr.dgrad_by_parity(g32, w32, h, w, pad).double() - dx64).abs() <= bar_dx).all())
    assert bool(((dw32.double() - dw64).abs() <= bar_dw).all()) and bool(((db32.double() - db64).abs() <= bar_db).all())


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_complete():
    from tomosar2height_amd.encoder import hourglass
    g = golden()
    assert [str(c) for c in g["cases"]] == list(sr.CASES) and int(g["relu_margin"]) == hg_grad_ref.RELU_MARGIN
    for name in sr.CASES:
        seed = int(g[f"{name}_seed"])
        assert hg_ref.SEED <= seed < hg_ref.SEED + 64
        module = sr.build(hourglass, name, trainable=True, stem_gradients=True)
        unused = {f"{n}.bn4.{k}".lstrip(".") for n, m in module.named_modules()
                  if isinstance(m, hourglass.ConvBlock) and m.downsample is None for k in ("weight", "bias")}
        used = {k: p for k, p in module.named_parameters() if k not in unused}
        assert sorted(str(k) for k in g[f"{name}_all_names"]) == sorted(list(used) + ["input"])
        names = [str(k) for k in g[f"{name}_names"]]
        assert sorted(names) == sorted(k for k in list(used) + ["input"] if sr.is_stem(k))
        assert ("down_conv2.weight" in names) == (sr.CASES[name] == "conv128") and "conv1.weight" in names and "conv2.bn4.bias" in names
        for key in names:
            a = g[f"{name}_{key}"]
            shape = sr.SHAPE if key == "input" else tuple(used[key].shape)
            assert a.dtype == np.float32 and a.shape == shape and g[f"{name}_{key}_q"].dtype == np.float16
            assert 0 < float(g[f"{name}_{key}_dev"]) < 1e-4 * np.abs(a).max()
        assert sr.restated_margin(name, hg_ref.init_hg_(module, seed), seed) >= hg_grad_ref.RELU_MARGIN


@pytest.mark.parametrize("name", tuple(sr.CASES))
def test_restated_stem_gradients_reproduce_the_fixture(name):
    """float64: to the quantisation of ``*_q``; float32: within 4 x ref32_dev, the factor the GPU path is given."""
    g = golden()
    r64, r32 = restated(name, torch.float64), restated(name, torch.float32)
    assert sorted(r64) == sorted(str(k) for k in g[f"{name}_all_names"])
    for key in (str(k) for k in g[f"{name}_names"]):
        want, tol4 = hg_ref.ref64(g, name, key)
        err64, err32 = np.abs(r64[key] - want).max(), np.abs(r32[key].astype(np.float64) - want).max()
        print(f"{name} d/d{key}: float64 err {err64:.3g} (bound {tol4 / 4 * 2.0 ** -11 + 1e-12:.3g}), float32 err {err32:.3g} (tolerance {tol4:.3g})")
        assert err64 <= tol4 / 4 * 2.0 ** -11 + 1e-12, (name, key, err64)
        assert err32 <= tol4, (name, key, err32, tol4)
