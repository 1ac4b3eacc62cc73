"""Gradients of the hourglass blocks from the plain-torch restatement (tests/hg_ref.py, differentiable as it stands), and the
cases of the gradient fixture (tests/golden/make_golden_hourglass_grad.py -> tests/golden/hourglass_grad*.npz).

A case is a module with ``hg_ref.init_hg_`` parameters, an input ``randn`` and a cotangent ``randn`` of the output's shape, all
three keyed by the fixture's seed; the loss is sum(out * cotangent).  ``ref_grads`` returns the gradient of that loss with
respect to the input (key ``input``) and every parameter that gets one (keys: the module's ``named_parameters`` names; ``bn4``
of a block whose channel count does not change is unused and has none).
"""
import zlib

import numpy as np
import torch

import hg_ref

# name -> (kind, constructor arguments, B, H, W)
CASES = {
    "block64_128": ("block", (64, 128, "group"), 2, 8, 4),
    "block128": ("block", (128, 128, "group"), 2, 4, 4),
    "hourglass128": ("hourglass", (1, 1, 128, "group"), 2, 4, 8),          # ~0.4 M parameters, the largest case
}
RELU_MARGIN = 8          # the generator refuses a seed with a float64 ReLU input closer to 0 than this many float32 deviations


def build(namespace, name, **kwargs):
    """The case's module from ``namespace`` (the reference's hourglass module, or tomosar2height_amd.encoder.hourglass)."""
    kind, args = CASES[name][:2]
    return (namespace.ConvBlock if kind == "block" else namespace.HourGlass)(*args, **kwargs)


def _randn(tag, name, seed, shape):
    g = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(f"{tag}:{name}".encode())) % (2 ** 31))
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def case_input(name, seed):
    _, args, b, h, w = CASES[name]
    return _randn("grad-input", name, seed, (b, args[0] if CASES[name][0] == "block" else args[2], h, w))


def case_cotangent(name, seed):
    kind, args, b, h, w = CASES[name]
    return _randn("grad-cotangent", name, seed, (b, args[1] if kind == "block" else args[2], h, w))


def restated(kind, x, params, depth=None):
    """The restatement of a block / an hourglass / the whole filter (``depth``: its constructor arguments) on ``params`` (the
    module's ``state_dict`` keys, no prefix)."""
    if kind == "filter":
        return hg_ref.hg_filter(x, params, **depth)
    p = {"m." + k: v for k, v in params.items()}
    return hg_ref.block(x, p, "m") if kind == "block" else hg_ref.hourglass(x, p, "m", depth)


def grads_of(kind, module, x, cotangent, dtype, depth=None, input_grad=True):
    """{name: gradient} of sum(restated(x) * cotangent) in ``dtype`` on the host: ``input`` and every parameter that gets one."""
    params = {k: v.cpu().clone().requires_grad_(True) for k, v in hg_ref.params_of(module, dtype).items()}
    x = x.detach().cpu().to(dtype).clone().requires_grad_(input_grad)
    out = restated(kind, x, params, depth)
    (out * cotangent.detach().cpu().to(dtype)).sum().backward()
    named = [k for k, _ in module.named_parameters()]
    got = {k: params[k].grad for k in named if params[k].grad is not None}
    if input_grad:
        got["input"] = x.grad
    return {k: v.detach() for k, v in got.items()}


class relu_inputs:
    """``with relu_inputs() as seen:`` every GroupNorm output the restatement hands to a ReLU inside the block is appended to
    ``seen`` (the same arithmetic: the clamp follows the recorded tensor)."""

    def __enter__(self):
        self.real, seen = hg_ref.group_norm, []

        def recording(x, groups, gamma, beta, eps=1e-5, relu=False, stats=False):
            if stats or not relu:
                return self.real(x, groups, gamma, beta, eps, relu, stats)
            y = self.real(x, groups, gamma, beta, eps)
            seen.append(y.detach())
            return torch.clamp_min(y, 0)

        hg_ref.group_norm = recording
        return seen

    def __exit__(self, *exc):
        hg_ref.group_norm = self.real


def relu_margin(kind, module, x, depth=None):
    """The closest float64 ReLU input of the restatement, as a multiple of its tensor's max|float32 - float64| on the host."""
    seen = {}
    for dtype in (torch.float32, torch.float64):
        with relu_inputs() as seen[dtype], torch.no_grad():
            restated(kind, x.detach().cpu().to(dtype), hg_ref.params_of(module, dtype, "cpu"), depth)
    return min(float(b.abs().min()) / max(float((a.double() - b).abs().max()), 1e-300) for a, b in zip(seen[torch.float32], seen[torch.float64]))


def walk_seed(make, start=hg_ref.SEED, tries=64):
    """The first seed >= ``start`` whose case ``make(seed) -> (kind, module, x, depth)`` keeps every float64 ReLU input at least
    RELU_MARGIN float32 deviations from zero (the fixture generator's rule: a gradient is discontinuous there, and neither the
    host's float32 run nor the device's may sit on the other side) -> (seed, kind, module, x, depth)."""
    for seed in range(start, start + tries):
        case = make(seed)
        if relu_margin(*case) >= RELU_MARGIN:
            return (seed,) + tuple(case)
    raise AssertionError("no seed keeps every ReLU input away from zero")


def ref_grads(name, module, dtype, seed):
    kind, args = CASES[name][:2]
    return grads_of(kind, module, case_input(name, seed), case_cotangent(name, seed), dtype, depth=args[1] if kind == "hourglass" else None)


def worst(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(ref, np.float64)).max())
