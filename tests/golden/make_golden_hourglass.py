"""Fixture of the hourglass image encoder (tests/golden/hourglass_encoder*.npz), made from the reference's own modules
(tomosar2height/encoder/hourglass.py; for ``model64`` inside a full TomoSAR2Height) in float32 and, the same modules after
``.double()``, in float64.  Build container only:

    python tests/golden/make_golden_hourglass.py

Weights are not stored: ``hg_ref.init_hg_`` (``detinit.det_init_`` + name-keyed normalisation parameters and running
statistics) re-creates them; images come from ``hg_ref.case_image``.  Cases: ``hg_ref.CASES`` and ``model64``.

Per compared tensor (``hg_ref.tensor_names``: the stem output, the outputs of conv2 / conv3 / conv4, each stack's hg, ll and
tmp_out, the final output; for ``model64`` the decoder's heights and the encoder's output) the file holds the float32 result,
``*_dev`` = max|ref32 - ref64| (the tests allow 4 x that), and the float64 result as ``*_q`` = (ref64 - ref32) / dev in float16:
ref64 = ref32 + q * dev, exact to 2^-11 of dev.  The ``state_dict`` key and shape lists are those of the first case.
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

from ref_import import import_reference, make_cfg  # noqa: E402
from make_golden import save  # noqa: E402
import make_golden_pnpp  # noqa: E402
import hg_ref  # noqa: E402

MODEL_POINTS, MODEL_CLOUD_SEED = 700, 21


def run_encoder(enc, image):
    """One forward of the reference's HGFilter with every compared tensor recorded."""
    outs, hooks = {}, []
    keep = lambda k: (lambda m, i, o: outs.__setitem__(k, o.detach().clone()))
    hooks.append(enc.conv2.register_forward_pre_hook(lambda m, i: outs.__setitem__("stem", i[0].detach().clone())))
    for k in ("conv2", "conv3", "conv4"):
        hooks.append(getattr(enc, k).register_forward_hook(keep(k)))
    for i in range(enc.num_modules):
        mods = enc._modules
        hooks.append(mods[f"m{i}"].register_forward_hook(keep(f"hg{i}")))
        hooks.append(mods[f"l{i}"].register_forward_pre_hook(lambda m, inp, i=i: outs.__setitem__(f"ll{i}", inp[0].detach().clone())))
        hooks.append(mods[f"l{i}"].register_forward_hook(keep(f"tmp_out{i}")))
    try:
        with torch.no_grad():
            outs["out"] = enc(image).detach().clone()
    finally:
        for h in hooks:
            h.remove()
    return outs


def store(arrays, name, key, t32, t64):
    a32, a64 = t32.numpy(), t64.numpy()
    dev = float(np.abs(a32.astype(np.float64) - a64).max())
    q = (a64 - a32.astype(np.float64)) / (dev if dev > 0 else 1.0)
    arrays[f"{name}_{key}"] = a32
    arrays[f"{name}_{key}_dev"] = dev
    arrays[f"{name}_{key}_q"] = q.astype(np.float16)
    print(f"  {name} {key}: shape {a32.shape} max|x| {np.abs(a64).max():.3g} ref32_dev {dev:.3g}")


def main():
    ref = import_reference()
    from tomosar2height.encoder import hourglass as ref_hg
    arrays = {"cases": np.array(list(hg_ref.CASES) + [hg_ref.MODEL_CASE]), "seed": hg_ref.SEED,
              "resolution": make_golden_pnpp.RESO, "feature_dim": make_golden_pnpp.FEAT, "output_size": make_golden_pnpp.OUT_SIZE}
    for n, name in enumerate(hg_ref.CASES):
        enc = hg_ref.init_hg_(ref_hg.HGFilter(**hg_ref.case_kwargs(name))).eval()
        enc64 = copy.deepcopy(enc).double()
        if n == 0:
            sd = enc.state_dict()
            arrays["state_keys"] = np.array(list(sd.keys()))
            arrays["state_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
        image = hg_ref.case_image(name)
        r32, r64 = run_encoder(enc, image), run_encoder(enc64, image.double())
        for key in hg_ref.tensor_names(enc.num_modules):
            store(arrays, name, key, r32[key], r64[key])

    # the full model: cloud + image, the default point encoder on the small cloud configuration, the hourglass image encoder
    name = hg_ref.MODEL_CASE
    cfg = make_cfg(depth=3, reso=make_golden_pnpp.RESO, hidden=make_golden_pnpp.FEAT, use_image=True)
    cfg["model"]["encoder2"] = "hourglass"
    cfg["model"]["encoder2_kwargs"] = dict(in_channel=3, feature_dim=make_golden_pnpp.FEAT)
    cfg["model"]["decoder_pixel_kwargs"]["output_size"] = make_golden_pnpp.OUT_SIZE
    model = hg_ref.init_hg_(ref.TomoSAR2Height(cfg)).eval()
    model64 = copy.deepcopy(model).double()
    arrays["model_num_stack"], arrays["model_num_hourglass"] = model.image_encoder.num_modules, model.image_encoder.num_hourglass
    pts, _ = make_golden_pnpp.cloud(MODEL_POINTS, 1, MODEL_CLOUD_SEED)
    image = hg_ref.case_image(name)
    arrays[f"{name}_points"] = pts.numpy()
    results = []
    real_sample = torch.nn.functional.grid_sample
    for m, double in ((model, False), (model64, True)):
        enc_out = {}
        hook = m.image_encoder.register_forward_hook(lambda mod, i, o: enc_out.__setitem__("out", o.detach().clone()))
        if double:      # alto.py:93 casts the (float32-exact) sampling coordinates with .float(), which grid_sample refuses beside a float64 plane
            torch.nn.functional.grid_sample = lambda inp, grid, **kw: real_sample(inp, grid.to(inp.dtype), **kw)
        try:
            with torch.no_grad():
                heights, _ = m(input_cloud=pts.double() if double else pts, input_image=image.double() if double else image)
        finally:
            torch.nn.functional.grid_sample = real_sample
            hook.remove()
        results.append({"heights": heights.detach().clone(), "out": enc_out["out"]})
    for key in ("out", "heights"):
        store(arrays, name, key, results[0][key], results[1][key])
    save("hourglass_encoder", **arrays)


if __name__ == "__main__":
    main()
