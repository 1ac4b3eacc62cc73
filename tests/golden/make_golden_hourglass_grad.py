"""Gradient fixture of the hourglass blocks (tests/golden/hourglass_grad*.npz), made from the reference's own modules
(tomosar2height/encoder/hourglass.py: ConvBlock, HourGlass) in float32 and, the same modules after ``.double()``, in float64.
Build container only, on the CPU:

    python tests/golden/make_golden_hourglass_grad.py

Cases: ``hg_grad_ref.CASES``.  Weights, inputs and cotangents are not stored: ``hg_ref.init_hg_``, ``hg_grad_ref.case_input`` and
``hg_grad_ref.case_cotangent`` re-create them from the stored ``seed``.  The loss is sum(out * cotangent); per case the file holds
``{case}_names`` (``input`` and every parameter that gets a gradient) and per name the float32 gradient, ``*_dev`` =
max|ref32 - ref64| (the tests allow 4 x that) and the float64 one as ``*_q`` = (ref64 - ref32) / dev in float16, the scheme of
make_golden_hourglass.py.

The seed.  A gradient is discontinuous where a ReLU input crosses zero, and the float32 run must not sit on the other side of
one than the float64 run: every GroupNorm output that feeds a ReLU is recorded in both precisions, and a seed is refused when
any float64 value lies closer to zero than ``hg_grad_ref.RELU_MARGIN`` x that tensor's max|float32 - float64|.  Seeds are walked
upward from ``hg_ref.SEED`` until every case passes with the same seed; the run fails if none of the first 64 does.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ref_import import import_reference  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_hourglass import store  # noqa: E402
import hg_ref  # noqa: E402
import hg_grad_ref  # noqa: E402


def run(module, x, cotangent):
    """One forward and backward of a reference module -> ({name: gradient}, {GroupNorm name: its output, a ReLU's input})."""
    relu_in, hooks = {}, []
    for name, m in module.named_modules():
        if isinstance(m, torch.nn.GroupNorm):          # (named_modules lists bn4 once, under its own name; unused layers never fire)
            hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: relu_in.__setitem__(name, o.detach().clone())))
    x = x.clone().requires_grad_(True)
    try:
        (module(x) * cotangent).sum().backward()
    finally:
        for h in hooks:
            h.remove()
    grads = {k: p.grad.detach().clone() for k, p in module.named_parameters() if p.grad is not None}
    grads["input"] = x.grad.detach().clone()
    return grads, relu_in


def case(ref_hg, name, seed):
    """(grads32, grads64, the closest ReLU input as a multiple of its tensor's float32 deviation) of one case."""
    m32 = hg_ref.init_hg_(hg_grad_ref.build(ref_hg, name), seed).eval()
    m64 = copy.deepcopy(m32).double()
    x, c = hg_grad_ref.case_input(name, seed), hg_grad_ref.case_cotangent(name, seed)
    g32, r32 = run(m32, x, c)
    g64, r64 = run(m64, x.double(), c.double())
    assert sorted(g32) == sorted(g64) and sorted(r32) == sorted(r64) and r64
    closest = min(float(r64[k].abs().min()) / float((r32[k].double() - r64[k]).abs().max()) for k in r64)
    return g32, g64, closest


def main():
    import_reference()
    from tomosar2height.encoder import hourglass as ref_hg
    for seed in range(hg_ref.SEED, hg_ref.SEED + 64):
        results = {}
        for name in hg_grad_ref.CASES:
            g32, g64, closest = case(ref_hg, name, seed)
            print(f"seed {seed} {name}: closest ReLU input at {closest:.3g} float32 deviations (at least {hg_grad_ref.RELU_MARGIN} wanted)")
            if closest < hg_grad_ref.RELU_MARGIN:
                break
            results[name] = (g32, g64)
        if len(results) == len(hg_grad_ref.CASES):
            break
    else:
        raise SystemExit("no seed keeps every ReLU input away from zero")
    arrays = {"cases": np.array(list(hg_grad_ref.CASES)), "seed": seed, "relu_margin": hg_grad_ref.RELU_MARGIN}
    for name, (g32, g64) in results.items():
        arrays[f"{name}_names"] = np.array(sorted(g32))
        for key in sorted(g32):
            store(arrays, name, key, g32[key], g64[key])
    save("hourglass_grad", **arrays)


if __name__ == "__main__":
    main()
