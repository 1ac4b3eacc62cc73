"""CPU (no GPU needed): the gradients of the plain-torch restatement of the hourglass blocks (tests/hg_ref.py under autograd,
tests/hg_grad_ref.py) reproduce the fixture made from the reference's own modules in float32 and float64
(tests/golden/make_golden_hourglass_grad.py); the ``trainable`` switch of the encoder's modules adds no state and refuses what
is not built before it touches a device; the header, the signature table and the scratch formula agree."""
import os
import re

import numpy as np
import pytest
import torch

import hg_grad_ref
import hg_ref
from abi_ref import declared_symbols
from conftest import load_golden

CASES = tuple(hg_grad_ref.CASES)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2h_hg.h")
NEW_ENTRIES = ("t2h_hg_groupnorm_bwd_reduce", "t2h_hg_groupnorm_bwd_apply", "t2h_hg_avgpool2x2_bwd", "t2h_hg_block_tail_bwd")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("hourglass_grad")
    return _cache["g"]


def restated(name, dtype):
    """The restatement's gradients of a case on this package's module, computed once and shared."""
    from tomosar2height_amd.encoder import hourglass
    key = (name, dtype)
    if key not in _cache:
        seed = int(golden()["seed"])
        module = hg_ref.init_hg_(hg_grad_ref.build(hourglass, name, trainable=True), seed)
        _cache[key] = {k: v.numpy() for k, v in hg_grad_ref.ref_grads(name, module, dtype, seed).items()}
    return _cache[key]


def test_fixture_holds_every_case_and_gradient():
    from tomosar2height_amd.encoder import hourglass
    g = golden()
    assert [str(c) for c in g["cases"]] == list(CASES) and int(g["seed"]) >= hg_ref.SEED and int(g["relu_margin"]) == hg_grad_ref.RELU_MARGIN
    for name in CASES:
        module = hg_grad_ref.build(hourglass, name, trainable=True)
        names = [str(k) for k in g[f"{name}_names"]]
        unused = {f"{n}.bn4.{k}".lstrip(".") for n, m in module.named_modules()          # bn4 where the channel count stays
                  if isinstance(m, hourglass.ConvBlock) and m.downsample is None for k in ("weight", "bias")}
        used = {k: p for k, p in module.named_parameters() if k not in unused}
        assert sorted(names) == sorted(list(used) + ["input"])
        for key in names:
            a = g[f"{name}_{key}"]
            shape = tuple(hg_grad_ref.case_input(name, 0).shape) if key == "input" else tuple(used[key].shape)
            assert a.dtype == np.float32 and a.shape == shape and g[f"{name}_{key}_q"].dtype == np.float16
            assert 0 < float(g[f"{name}_{key}_dev"]) < 1e-4 * np.abs(a).max()
    assert sum(p.numel() for p in hg_grad_ref.build(hourglass, "hourglass128").parameters()) > 400_000


@pytest.mark.parametrize("name", CASES)
def test_restated_gradients_in_float64_reproduce_ref64(name):
    """To the quantisation of ``*_q`` (2^-11 dev, as test_hourglass_cpu.py::test_restatement_in_float64_reproduces_ref64 argues)."""
    g = golden()
    got = restated(name, torch.float64)
    assert sorted(got) == sorted(str(k) for k in g[f"{name}_names"])
    for key, mine in got.items():
        want, tol4 = hg_ref.ref64(g, name, key)
        err = np.abs(mine - want).max()
        bound = tol4 / 4 * 2.0 ** -11 + 1e-12
        print(f"{name} d/d{key}: max err {err:.3g}, bound {bound:.3g}")
        assert err <= bound, (name, key, err, bound)


@pytest.mark.parametrize("name", CASES)
def test_restated_gradients_in_float32_stay_within_ref32_dev(name):
    """Within 4 x max|ref32 - ref64| of ref64 -- the factor the GPU path is given."""
    g = golden()
    for key, mine in restated(name, torch.float32).items():
        want, tol = hg_ref.ref64(g, name, key)
        err = np.abs(mine.astype(np.float64) - want).max()
        print(f"{name} d/d{key}: max err {err:.3g}, tolerance {tol:.3g} (4 x ref32_dev)")
        assert err <= tol, (name, key, err, tol)


def test_the_switch_is_a_plain_attribute_passed_down():
    from tomosar2height_amd.encoder.hourglass import ConvBlock, HGFilter, HourGlass
    kw = dict(in_channel=3, feature_dim=32, num_stack=2, num_hourglass=2)
    off, on = HGFilter(**kw), HGFilter(**kw, trainable=True)
    assert list(off.state_dict()) == list(on.state_dict())
    assert [k for k, _ in off.named_parameters()] == [k for k, _ in on.named_parameters()]
    assert [k for k, _ in off.named_buffers()] == [k for k, _ in on.named_buffers()]
    mine = lambda net: [m.trainable for m in net.modules() if isinstance(m, (ConvBlock, HourGlass, HGFilter))]
    assert len(mine(on)) == 1 + 3 + 2 * (1 + 7 + 1) and all(mine(on)) and not any(mine(off))
    off.trainable = True                                            # set after construction: reaches every module below
    assert all(mine(off)) and list(off.state_dict()) == list(on.state_dict())
    off.m0.trainable = False
    assert not any(mine(off.m0)) and off.trainable and off.top_m_0.trainable
    assert ConvBlock(64, 128, "group").trainable is False and HourGlass(1, 1, 128, "group", trainable=True).b3_1.trainable is True
    with pytest.raises(TypeError):
        ConvBlock(64, 128, "group", True)                           # keyword-only


def test_trainable_refuses_what_is_not_built_before_touching_the_device():
    from tomosar2height_amd.encoder.hourglass import ConvBlock, HGFilter, HourGlass
    for module, x in ((ConvBlock(64, 128, "batch", trainable=True), torch.zeros(1, 64, 4, 4)),
                      (HourGlass(1, 1, 128, "batch", trainable=True), torch.zeros(1, 128, 4, 4)),
                      (HGFilter(3, 32, 1, 1, norm="batch", trainable=True), torch.zeros(1, 3, 32, 32))):
        for mode in (module.train, module.eval):
            with pytest.raises(NotImplementedError, match="norm='batch'"):
                mode()(x)
    enc = HGFilter(3, 32, 2, 2, trainable=True)
    with pytest.raises(NotImplementedError, match=r"conv1\.weight, conv1\.bias.*stride-2"):
        enc(torch.zeros(1, 3, 32, 32))
    enc.conv1.requires_grad_(False)
    with pytest.raises(RuntimeError, match="cuda device"):          # nothing left to refuse: the next stop is the device
        enc(torch.zeros(1, 3, 32, 32))
    down = HGFilter(3, 32, 1, 1, hg_down="conv128", trainable=True)
    down.conv1.requires_grad_(False)
    with pytest.raises(NotImplementedError, match=r"down_conv2\.weight.*stride-2"):
        down(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match="cuda device"):
        ConvBlock(64, 128, "group", trainable=True)(torch.zeros(1, 64, 4, 4))
    with torch.no_grad(), pytest.raises(RuntimeError, match="cuda device"):      # no_grad: the inference path, no refusal
        enc(torch.zeros(1, 3, 32, 32))
    # the default is unchanged
    with pytest.raises(NotImplementedError, match="inference only"):
        ConvBlock(64, 128, "group")(torch.zeros(1, 64, 4, 4))


def test_trainer_refuses_a_trainable_image_encoder():
    from tomosar2height_amd.encoder.hourglass import HGFilter
    from tomosar2height_amd.trainer import Trainer

    class Model(torch.nn.Module):
        def __init__(self, trainable):
            super().__init__()
            self.image_encoder = HGFilter(3, 32, 1, 1, trainable=trainable)

    class Optimizer:
        def zero_grad(self):
            pass

    with pytest.raises(NotImplementedError, match="trainable=True"):
        Trainer(Model(True), Optimizer())
    Trainer(Model(False), Optimizer())


def test_header_signatures_and_the_partial_formula_agree():
    from tomosar2height_amd.encoder import hourglass
    assert sorted(hourglass.SIGNATURES) == declared_symbols(HEADER) and set(NEW_ENTRIES) <= set(hourglass.SIGNATURES)
    lib = hourglass.load()
    assert all(hasattr(lib, name) for name in NEW_ENTRIES)
    text = open(HEADER).read()
    assert "Forward only" not in text
    defines = {k: int(v) for k, v in re.findall(r"^#define\s+(T2H_HG_\w+)\s+(\d+)\b", text, flags=re.M)}
    assert defines == {"T2H_HG_GNB_PIXELS": hourglass.GNB_PIXELS}
    assert re.search(r"B \* ceil\(H \* W / T2H_HG_GNB_PIXELS\) \* 2 \* C\s+floats", text)
    pixels = defines["T2H_HG_GNB_PIXELS"]
    for b, h, w, c in ((1, 1, 1, 32), (2, 4, 2, 64), (2, 8, 8, 256), (2, 10, 13, 64), (1, 128, 128, 256), (3, 8, 8 + 1, 1024)):
        want = b * ((h * w + pixels - 1) // pixels) * 2 * c
        assert hourglass.gn_bwd_partial_floats(b, h, w, c) == want, (b, h, w, c)
    # no new size query: the scratch of the new entries is the typed ``partial`` argument
    src = open(os.path.join(os.path.dirname(HEADER), "..", "tomosar2height_amd", "csrc", "hourglass.hip")).read()
    assert re.findall(r"^T2H_API\s+size_t\s+(\w+)\s*\(", src, flags=re.M) == ["t2h_hg_groupnorm_workspace_bytes"]
