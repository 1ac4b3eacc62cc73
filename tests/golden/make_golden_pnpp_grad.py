"""Fixture of the PointNet++ encoder's parameter gradients in ``eval()`` (tests/golden/pnpp_grad*.npz), made from the
reference's own modules inside a full TomoSAR2Height with autograd on, in float32 and, after ``.double()``, in float64.  Build
container only:

    python tests/golden/make_golden_pnpp_grad.py

Clouds, FPS starts and weights are those of the ``pnpp_encoder`` fixture (``pnpp_ref.init_pnpp_(seed=41)``; the clouds and starts
are read from it), cases ``n700`` (ALTO), ``n700u`` (plain U-Net) and ``n1536b2`` (B = 2): their discrete stages are asserted
unambiguous between the precisions there, and asserted again here.  The reference runs under the patches of
``make_golden_pnpp.run``.  BatchNorm uses its running statistics (``eval()``), so only ``conv.weight``, ``conv.bias``,
``bn.weight`` and ``bn.bias`` have gradients.

Loss: ``L = sum(heights * r)``, ``r = torch.randn(heights.shape, generator=manual_seed(R_SEED))`` in float32 (widened for the
float64 run); the seed is stored, not ``r``.

Per ``point_encoder.sa*`` / ``fp*`` parameter ``P`` of case ``C`` the file holds ``C/P`` = the float32 gradient at the flat
positions ``k * stride``, ``stride = ceil(numel / MAX_STORED)``; ``C/P_dev`` = max|g32 - g64| over those positions (the tests allow
4 x that); ``C/P_q`` = (g64 - g32) / dev in float16, so that g64 = g32 + q * dev.  Every stored gradient has a non-zero entry
(asserted).  ``C/unet_with_grad`` names the ``point_encoder.unet.*`` parameters the reference's backward reaches (layers its forward
never uses keep ``grad is None``).
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
from make_golden_pnpp import cfg_for, fixed_randint  # noqa: E402
import pnpp_ref  # noqa: E402

CASES = ("n700", "n700u", "n1536b2")
R_SEED, MAX_STORED = 97, 8192
STAGES = ("sa1", "sa2", "sa3", "fp3", "fp2", "fp1")


def stride_of(numel):
    return -(-numel // MAX_STORED)


def loss_weights(shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(R_SEED), dtype=torch.float32)


def gradients(model, pts, starts, double):
    """{parameter name: gradient} of the point stages for L = sum(heights * r) on the reference model in eval()."""
    real_sample = torch.nn.functional.grid_sample
    model.zero_grad(set_to_none=True)
    if double:                                                # (the two patches of make_golden_pnpp.run)
        torch.set_default_dtype(torch.float64)
        torch.nn.functional.grid_sample = lambda inp, grid, **kw: real_sample(inp, grid.to(inp.dtype), **kw)
    try:
        with fixed_randint([s.clone() for s in starts]):
            heights, _ = model(input_cloud=pts.double() if double else pts)
        r = loss_weights(heights.shape)
        (heights * r.to(heights.dtype)).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
        torch.nn.functional.grid_sample = real_sample
    out = {}
    for name, p in model.point_encoder.named_parameters():
        if name.split(".")[0] in STAGES:
            assert p.grad is not None, name
            out[name] = p.grad.detach().clone()
    unet = [name for name, p in model.point_encoder.unet.named_parameters() if p.grad is not None]
    return out, heights.detach(), unet


def main():
    ref = import_reference()
    g = {}
    golden_dir = HERE
    import glob
    for part in sorted(glob.glob(os.path.join(golden_dir, "pnpp_encoder.part*.npz"))):
        with np.load(part, allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files})
    arrays = {"cases": np.array(CASES), "r_seed": R_SEED, "max_stored": MAX_STORED}
    names_written = False
    for case in CASES:
        unet_type = str(g[f"{case}_unet_type"])
        model = pnpp_ref.init_pnpp_(ref.TomoSAR2Height(cfg_for(unet_type)), seed=41).eval()
        model64 = copy.deepcopy(model).double().eval()
        pts = torch.from_numpy(g[f"{case}_points"])
        starts = [torch.from_numpy(g[f"{case}_start1"]), torch.from_numpy(g[f"{case}_start2"])]
        g32, h32, unet32 = gradients(model, pts, starts, False)
        g64, h64, unet64 = gradients(model64, pts, starts, True)
        # the U-Net parameters the reference's own backward reaches (its unused layers keep grad None)
        assert unet32 == unet64 and unet32, case
        arrays[f"{case}/unet_with_grad"] = np.array(unet32)
        # the same forward as the pnpp_encoder fixture recorded
        assert np.array_equal(h32.numpy(), g[f"{case}_heights"]), case
        if not names_written:
            arrays["param_names"] = np.array(list(g32))
            arrays["param_numel"] = np.array([v.numel() for v in g32.values()], dtype=np.int64)
            names_written = True
        for name in g32:
            a32 = g32[name].reshape(-1).numpy()
            a64 = g64[name].reshape(-1).numpy()
            assert a64.dtype == np.float64 and a32.dtype == np.float32
            st = stride_of(a32.size)
            a32, a64 = a32[::st].copy(), a64[::st].copy()
            assert np.any(a32 != 0) and np.any(a64 != 0), (case, name)
            dev = float(np.abs(a32.astype(np.float64) - a64).max())
            assert dev > 0, (case, name)
            q = (a64 - a32.astype(np.float64)) / dev
            arrays[f"{case}/{name}"] = a32
            arrays[f"{case}/{name}_dev"] = dev
            arrays[f"{case}/{name}_q"] = q.astype(np.float16)
            print(f"  {case} {name}: {a32.size} of {g32[name].numel()} stored (stride {st}), max|g| {np.abs(a64).max():.3g}, "
                  f"ref32_dev {dev:.3g}")
    save("pnpp_grad", **arrays)


if __name__ == "__main__":
    main()
