"""Fixture of the PointNet++ encoder under ``train()`` -- BatchNorm batch statistics, their backward and the running-average
updates (tests/golden/pnpp_train*.npz) -- made from the reference's own modules inside a full TomoSAR2Height, in float32 and,
after ``.double()``, in float64.  Build container only:

    python tests/golden/make_golden_pnpp_train.py

Clouds, FPS starts, weights (``pnpp_ref.init_pnpp_(seed=41)``), loss (``L = sum(heights * r)``, seed 97) and cases (``n700``,
``n700u``, ``n1536b2``) are those of ``make_golden_pnpp_grad.py``; the discrete stages depend on ``xyz`` only and are asserted to
be those of the ``pnpp_encoder`` fixture.

Stored per case ``C``, every float tensor ``T`` in the form of the gradient fixture -- ``C/T`` = float32 values, ``C/T_dev`` =
max|t32 - t64|, ``C/T_q`` = (t64 - t32) / dev in float16, so that t64 = t32 + q * dev:
  ``heights``; every ``sa*`` / ``fp*`` parameter gradient at the flat positions ``k * stride``, ``stride = ceil(numel /
  MAX_STORED)``; ``buf1/<name>`` and ``buf2/<name>`` = every ``running_mean`` / ``running_var`` after one forward and after a
  second forward on the same cloud (the momentum recurrence); ``C/nbt1``, ``C/nbt2`` = ``num_batches_tracked`` (exact).
The exact gradient of a conv bias is 0 (a shift of z leaves z - mean unchanged): both precisions hold rounding noise, so its
``_dev`` may be anything (0 included; then ``_q`` is 0) and the tests bound it by ``C/l1/<bias>`` [c] = sum_r |dz[r, c]| and
``C/rows/<bias>`` = M of the float64 run (a hook on the convolution's output gradient).  Every other ``_dev`` is > 0 (asserted).
"""
import copy
import glob
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
from make_golden_pnpp import INDEX_KEYS, cfg_for, fixed_randint  # noqa: E402
from make_golden_pnpp_grad import CASES, MAX_STORED, R_SEED, STAGES, loss_weights, stride_of  # noqa: E402
import pnpp_ref  # noqa: E402


def buffers(model):
    return {k: v.detach().clone() for k, v in model.point_encoder.named_buffers() if k.split(".")[0] in STAGES}


def train_run(model, ref_pp, pts, starts, double):
    """Forward + backward under train(), then a second forward on the same cloud: heights, gradients, the buffers after each
    forward, the discrete stages and per conv bias (sum_r |dz|, M)."""
    rec = {"fps": [], "ball": [], "sqd": []}
    orig = {k: getattr(ref_pp, k) for k in ("farthest_point_sample", "query_ball_point", "square_distance")}
    for name, key in (("farthest_point_sample", "fps"), ("query_ball_point", "ball"), ("square_distance", "sqd")):
        setattr(ref_pp, name, lambda *a, _n=name, _k=key, **kw: (rec[_k].append(orig[_n](*a, **kw)), rec[_k][-1])[1])
    l1, hooks = {}, []
    for name, mod in model.point_encoder.named_modules():
        if name.split(".")[0] in STAGES and ".mlp_convs." in name:
            def fwd(m, i, o, name=name):
                if o.requires_grad:
                    o.register_hook(lambda g: l1.__setitem__(name + ".bias", (
                        g.abs().sum(dim=[d for d in range(g.dim()) if d != 1]).detach().clone(), g.numel() // g.shape[1])))
            hooks.append(mod.register_forward_hook(fwd))
    real_sample = torch.nn.functional.grid_sample
    model.train()
    model.zero_grad(set_to_none=True)
    if double:                                                # (the two patches of make_golden_pnpp.run)
        torch.set_default_dtype(torch.float64)
        torch.nn.functional.grid_sample = lambda inp, grid, **kw: real_sample(inp, grid.to(inp.dtype), **kw)
    try:
        x = pts.double() if double else pts
        with fixed_randint([s.clone() for s in starts]):
            heights, _ = model(input_cloud=x)
        buf1 = buffers(model)
        (heights * loss_weights(heights.shape).to(heights.dtype)).sum().backward()
        with torch.no_grad(), fixed_randint([s.clone() for s in starts]):
            model(input_cloud=x)
        buf2 = buffers(model)
    finally:
        torch.set_default_dtype(torch.float32)
        torch.nn.functional.grid_sample = real_sample
        for h in hooks:
            h.remove()
        for k, v in orig.items():
            setattr(ref_pp, k, v)
    nn = lambda d: d.sort(dim=-1)[1][:, :, :3].contiguous()
    index = dict(sa1_fps=rec["fps"][0], sa2_fps=rec["fps"][1], sa1_idx=rec["ball"][0], sa2_idx=rec["ball"][1],
                 fp2_idx=nn(rec["sqd"][2]), fp1_idx=nn(rec["sqd"][3]))
    grads = {}
    for name, p in model.point_encoder.named_parameters():
        if name.split(".")[0] in STAGES:
            assert p.grad is not None, name
            grads[name] = p.grad.detach().clone()
    return heights.detach(), grads, buf1, buf2, index, l1


def store(arrays, key, t32, t64, strided=False, may_vanish=False):
    a32, a64 = t32.reshape(-1).numpy(), t64.reshape(-1).numpy()
    assert a32.dtype == np.float32 and a64.dtype == np.float64, key
    if strided:
        st = stride_of(a32.size)
        a32, a64 = a32[::st].copy(), a64[::st].copy()
    dev = float(np.abs(a32.astype(np.float64) - a64).max())
    assert dev > 0 or may_vanish, key
    arrays[key] = a32
    arrays[key + "_dev"] = dev
    arrays[key + "_q"] = ((a64 - a32.astype(np.float64)) / (dev if dev > 0 else 1.0)).astype(np.float16)
    return dev


def main():
    ref = import_reference()
    import tomosar2height.encoder.pointnetpp as ref_pp
    g = {}
    for part in sorted(glob.glob(os.path.join(HERE, "pnpp_encoder.part*.npz"))):
        with np.load(part, allow_pickle=False) as z:
            g.update({k: z[k] for k in z.files})
    arrays = {"cases": np.array(CASES), "r_seed": R_SEED, "max_stored": MAX_STORED}
    for case in CASES:
        model = pnpp_ref.init_pnpp_(ref.TomoSAR2Height(cfg_for(str(g[f"{case}_unet_type"]))), seed=41)
        model64 = copy.deepcopy(model).double()
        pts = torch.from_numpy(g[f"{case}_points"])
        starts = [torch.from_numpy(g[f"{case}_start1"]), torch.from_numpy(g[f"{case}_start2"])]
        h32, g32, b1_32, b2_32, i32, _ = train_run(model, ref_pp, pts, starts, False)
        h64, g64, b1_64, b2_64, i64, l1 = train_run(model64, ref_pp, pts, starts, True)
        for k in INDEX_KEYS:                                   # the discrete stages depend on xyz only
            for got in (i32[k], i64[k]):
                assert np.array_equal(got.numpy().astype(np.int32), g[f"{case}_{k}"]), (case, k)
        if "param_names" not in arrays:
            arrays["param_names"] = np.array(list(g32))
            arrays["param_numel"] = np.array([v.numel() for v in g32.values()], dtype=np.int64)
            arrays["buffer_names"] = np.array([k for k in b1_32 if not k.endswith("num_batches_tracked")])
        store(arrays, f"{case}/heights", h32, h64)
        for name in g32:
            is_conv_bias = ".mlp_convs." in name and name.endswith(".bias")
            dev = store(arrays, f"{case}/{name}", g32[name], g64[name], strided=True, may_vanish=is_conv_bias)
            if is_conv_bias:
                arrays[f"{case}/l1/{name}"] = l1[name][0].numpy().astype(np.float64)
                arrays[f"{case}/rows/{name}"] = int(l1[name][1])
            print(f"  {case} {name}: max|g| {float(g64[name].abs().max()):.3g}, ref32_dev {dev:.3g}")
        for tag, b32, b64 in (("buf1", b1_32, b1_64), ("buf2", b2_32, b2_64)):
            for name in arrays["buffer_names"]:
                dev = store(arrays, f"{case}/{tag}/{name}", b32[str(name)], b64[str(name)])
                print(f"  {case} {tag} {name}: ref32_dev {dev:.3g}")
        for tag, b32, b64 in (("nbt1", b1_32, b1_64), ("nbt2", b2_32, b2_64)):
            nbt = {k: int(v) for k, v in b32.items() if k.endswith("num_batches_tracked")}
            assert nbt == {k: int(v) for k, v in b64.items() if k.endswith("num_batches_tracked")}
            assert set(nbt.values()) == {8 if tag == "nbt1" else 9}, nbt       # init_pnpp_ starts the counters at 7
            arrays[f"{case}/{tag}"] = np.array(list(nbt.values()), dtype=np.int64)
    save("pnpp_train", **arrays)


if __name__ == "__main__":
    main()
