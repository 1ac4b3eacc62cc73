"""Gradient fixture of the hourglass encoder's stem (tests/golden/hourglass_stem_grad*.npz), made from the reference's own
``HGFilter`` (tomosar2height/encoder/hourglass.py) in float32 and, the same module after ``.double()``, in float64.  Build
container only, on the CPU:

    python tests/golden/make_golden_hourglass_stem_grad.py

Cases: ``hg_stem_ref.CASES`` -- ``HGFilter(3, 32, num_hourglass=1, num_stack=1)`` with ``hg_down='ave_pool'`` and ``'conv128'`` on
2 x 3 x 16 x 16.  Weights, inputs and cotangents are not stored (``hg_ref.init_hg_``, ``hg_stem_ref.case_input`` / ``case_cotangent``
re-create them from the case's stored seed).  The loss is sum(out * cotangent).  Per case the file holds ``{case}_seed``,
``{case}_all_names`` (``input`` and every parameter that gets a gradient: the set the tests compare), ``{case}_names`` (the stem's:
``input``, ``conv1.*``, ``bn1.*``, ``conv2.*``, ``down_conv2.*``) and for each of the latter the float32 gradient, ``*_dev`` =
max|ref32 - ref64| and the float64 one as ``*_q``, the scheme of make_golden_hourglass.py.  The gradients behind the stem are not
stored: the tests take them from the restatement (tests/hg_grad_ref.py).

The seed of a case is the first from ``hg_ref.SEED`` on that keeps every float64 ReLU input ``hg_grad_ref.RELU_MARGIN`` float32
deviations from zero (the rule of make_golden_hourglass_grad.py); the run fails if none of the first 64 does.
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ref_import import import_reference  # noqa: E402
from make_golden import save  # noqa: E402
from make_golden_hourglass import store  # noqa: E402
from make_golden_hourglass_grad import run  # noqa: E402
import hg_ref  # noqa: E402
import hg_grad_ref  # noqa: E402
import hg_stem_ref  # noqa: E402


def case(ref_hg, name, seed):
    """(grads32, grads64, the closest ReLU input as a multiple of its tensor's float32 deviation) of one case."""
    m32 = hg_ref.init_hg_(hg_stem_ref.build(ref_hg, name), seed).eval()
    m64 = copy.deepcopy(m32).double()
    x, c = hg_stem_ref.case_input(name, seed), hg_stem_ref.case_cotangent(name, seed)
    g32, r32 = run(m32, x, c)
    g64, r64 = run(m64, x.double(), c.double())
    assert sorted(g32) == sorted(g64) and sorted(r32) == sorted(r64) and r64
    closest = min(float(r64[k].abs().min()) / float((r32[k].double() - r64[k]).abs().max()) for k in r64)
    return g32, g64, closest


def main():
    import_reference()
    from tomosar2height.encoder import hourglass as ref_hg
    arrays = {"cases": np.array(list(hg_stem_ref.CASES)), "relu_margin": hg_grad_ref.RELU_MARGIN}
    for name in hg_stem_ref.CASES:
        for seed in range(hg_ref.SEED, hg_ref.SEED + 64):
            g32, g64, closest = case(ref_hg, name, seed)
            print(f"seed {seed} {name}: closest ReLU input at {closest:.3g} float32 deviations (at least {hg_grad_ref.RELU_MARGIN} wanted)")
            if closest >= hg_grad_ref.RELU_MARGIN:
                break
        else:
            raise SystemExit(f"{name}: no seed keeps every ReLU input away from zero")
        stem = sorted(k for k in g32 if hg_stem_ref.is_stem(k))
        arrays[f"{name}_seed"] = seed
        arrays[f"{name}_all_names"] = np.array(sorted(g32))
        arrays[f"{name}_names"] = np.array(stem)
        for key in stem:
            store(arrays, name, key, g32[key], g64[key])
    save(hg_stem_ref.FIXTURE, **arrays)


if __name__ == "__main__":
    main()
