"""CPU (no GPU needed): the plain-torch restatement of the hourglass image encoder (tests/hg_ref.py) reproduces the fixture made
from the reference's own modules in float32 and float64 (tests/golden/make_golden_hourglass.py), and the encoder's constructor,
parameter names and shapes are the reference's."""
import io

import numpy as np
import pytest
import torch

import hg_ref
from abi_ref import declared_symbols
from conftest import load_golden

CASES = tuple(hg_ref.CASES)
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("hourglass_encoder")
    return _cache["g"]


def encoder(name):
    from tomosar2height_amd.encoder import encoder_dict
    key = ("enc", name)
    if key not in _cache:
        _cache[key] = hg_ref.init_hg_(encoder_dict["hourglass"](**hg_ref.case_kwargs(name))).eval()
    return _cache[key]


def restated(name, dtype):
    """Every compared tensor of a case from the restatement on this package's parameters, computed once and shared."""
    key = (name, dtype)
    if key not in _cache:
        enc, trace = encoder(name), {}
        with torch.no_grad():
            hg_ref.hg_filter(hg_ref.case_image(name).to(dtype), hg_ref.params_of(enc, dtype), trace=trace, **hg_ref.case_kwargs(name))
        _cache[key] = {k: v.numpy() for k, v in trace.items()}
    return _cache[key]


def test_fixture_holds_every_case_and_tensor():
    g = golden()
    assert [str(c) for c in g["cases"]] == list(CASES) + ["model64"]
    for name in CASES:
        b, h, w, kw = hg_ref.CASES[name]
        for key in hg_ref.tensor_names(kw.get("num_stack", 4)):
            a = g[f"{name}_{key}"]
            assert a.dtype == np.float32 and a.shape[0] == b and g[f"{name}_{key}_q"].dtype == np.float16
            assert 0 < float(g[f"{name}_{key}_dev"]) < 1e-5 * np.abs(a).max()
        assert g[f"{name}_out"].shape == (b, 32, h // 4, w // 4)
    assert g["model64_heights"].shape == (1, 64, 64, 1) and g["model64_out"].shape == (1, 32, 16, 16)
    assert g["c128_hg0"].shape == (1, 256, 16, 8) and int(g["model_num_stack"]) == 4 and int(g["model_num_hourglass"]) == 2


@pytest.mark.parametrize("name", CASES)
def test_restatement_in_float64_reproduces_ref64(name):
    """To the quantisation of ``*_q``: ref64 is stored as ref32 + q dev with q in float16 (2^-11 relative, |q| <= 1), so
    |stored - ref64| <= 2^-11 dev; the restatement's own float64 rounding is twelve orders below that."""
    g = golden()
    for key, got in restated(name, torch.float64).items():
        want, tol4 = hg_ref.ref64(g, name, key)
        err = np.abs(got - want).max()
        bound = tol4 / 4 * 2.0 ** -11 + 1e-12
        print(f"{name} {key}: max err {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (name, key, err, bound)


@pytest.mark.parametrize("name", CASES)
def test_restatement_in_float32_stays_within_ref32_dev(name):
    """Within 4 x max|ref32 - ref64| of ref64 -- the factor the GPU path is given: same precision, another accumulation order."""
    g = golden()
    for key, got in restated(name, torch.float32).items():
        want, tol = hg_ref.ref64(g, name, key)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{name} {key}: max err {err:.3g}, tolerance {tol:.3g} (4 x ref32_dev)")
        assert err <= tol, (name, key, err, tol)


def test_constructs_with_the_references_state_dict():
    from tomosar2height_amd.encoder import encoder_dict
    from tomosar2height_amd.encoder.hourglass import HGFilter
    g = golden()
    assert encoder_dict["hourglass"] is HGFilter
    enc = encoder(CASES[0])
    sd = enc.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["state_shapes"]]
    # bn4 is also downsample.0: both keys, one storage; and it exists unused where the channel count does not change
    assert sd["conv2.bn4.weight"].data_ptr() == sd["conv2.downsample.0.weight"].data_ptr()
    assert "conv3.bn4.weight" in sd and "conv3.downsample.0.weight" not in sd and enc.conv3.downsample is None
    for k in ("m0.b1_2.conv1.weight", "m0.b2_plus_1.bn1.bias", "m0.b3_1.conv3.weight", "top_m_1.bn2.weight", "conv_last0.bias",
              "bn_end1.weight", "l1.weight", "bl0.weight", "al0.bias"):
        assert k in sd, k
    assert "bl1.weight" not in sd and tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7) and tuple(sd["al0.weight"].shape) == (256, 32, 1, 1)
    defaults = HGFilter(2)
    assert (defaults.out_feature_dim, defaults.num_hourglass, defaults.num_modules, defaults.norm, defaults.hg_down) == (
        256, 2, 4, "group", "ave_pool")
    assert "bn_end0.running_mean" in encoder("bn32").state_dict() and "down_conv2.bias" in encoder("bn32").state_dict()


def test_state_dict_round_trip_is_strict():
    from tomosar2height_amd.encoder import encoder_dict
    src = encoder("bn32")
    buf = io.BytesIO()
    torch.save(src.state_dict(), buf)
    buf.seek(0)
    dst = encoder_dict["hourglass"](**hg_ref.case_kwargs("bn32"))
    result = dst.load_state_dict(torch.load(buf), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    for (ka, a), (kb, b) in zip(src.state_dict().items(), dst.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    assert dst.conv3.bn4.weight is not None and dst.conv4.downsample[0] is dst.conv4.bn4


def test_constructor_refusals_are_the_references():
    from tomosar2height_amd.encoder import encoder_dict
    with pytest.raises(NameError, match="Unknown HGFilter downsampling method"):
        encoder_dict["hourglass"](3, hg_down="max_pool")
    with pytest.raises(ValueError, match=r"num_channels \(16\) must be divisible by num_groups \(32\)"):      # GroupNorm(32, 16)
        encoder_dict["hourglass"](3, norm="group", hg_down="conv64")
    encoder_dict["hourglass"](3, norm="batch", hg_down="conv64", num_stack=1)


def test_forward_refuses_what_is_not_built_before_touching_the_device():
    enc = encoder("g64")
    with pytest.raises(NotImplementedError, match="inference only"):
        enc(torch.zeros(1, 3, 64, 64))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="cuda device"):
            enc(torch.zeros(1, 3, 64, 64))
        with pytest.raises(NotImplementedError, match="batch statistics"):
            encoder("bn32").train()(torch.zeros(1, 3, 32, 32))
    encoder("bn32").eval()


def test_header_declares_exactly_the_typed_entry_points():
    from tomosar2height_amd import _lib, pointops
    from tomosar2height_amd.csrc import build
    from tomosar2height_amd.encoder import hourglass
    headers = [h for h in build.PUBLIC_HEADERS if h.endswith("t2h_hg.h")]
    assert len(headers) == 1
    assert sorted(hourglass.SIGNATURES) == declared_symbols(headers[0])
    assert not set(hourglass.SIGNATURES) & (set(_lib.SIGNATURES) | set(pointops.SIGNATURES))
    assert any(s.endswith("hourglass.hip") for s in build.sources())
    lib = hourglass.load()
    assert all(hasattr(lib, name) for name in hourglass.SIGNATURES)
    # shapes without a kernel report no workspace
    assert lib.t2h_hg_groupnorm_workspace_bytes(1, 16, 16, 30, 3) == 0 and lib.t2h_hg_groupnorm_workspace_bytes(1, 16, 16, 64, 48) == 0
    assert lib.t2h_hg_groupnorm_workspace_bytes(2, 16, 16, 64, 32) == 1
    assert lib.t2h_hg_groupnorm_workspace_bytes(2, 128, 128, 64, 32) == 2 * 16 * 32 * 3 * 4
