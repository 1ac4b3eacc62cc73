"""Fixture of the PointNet++ encoder (tests/golden/pnpp_encoder*.npz), made from the reference's own modules
(tomosar2height/encoder/pointnetpp.py inside a full TomoSAR2Height) in float32 and, the same modules after ``.double()``, in
float64.  Build container only:

    python tests/golden/make_golden_pnpp.py

Weights are not stored: ``pnpp_ref.init_pnpp_`` (``detinit.det_init_`` + name-keyed BatchNorm statistics) re-creates them.
Clouds: xy uniform in (0, 1), z in [0, 0.6).  FPS starts are drawn from a seeded generator, recorded, and handed to the
reference's ``torch.randint`` call in ``farthest_point_sample`` (sa1 first, then sa2).

Unambiguity.  The discrete stages are compared bit for bit, so on every cloud but ``dup1024`` float32 and float64 must give
the same FPS indices, ball indices and 3-NN indices; that is ASSERTED here.  To get there a cloud is generated with spare
points and exactly that many points FPS never selects are deleted -- first those within 1e-5 (float64 d2 by differences) of a
ball boundary of ``sa1`` and those whose 3-NN indices differ between the precisions, then others -- which does not change what
FPS chooses; a cloud that still fails is reseeded.

Per compared tensor the file holds the float32 result, ``*_dev`` = max|ref32 - ref64| (the tests allow 4 x that), and the
float64 result as ``*_q`` = (ref64 - ref32) / dev in float16: ref64 = ref32 + q * dev, exact to 2^-11 of dev.

The coincident rows.  The sources of a propagation are among its targets; there (float64 d2_min by differences < 1e-12,
``fp1_coincident`` / ``fp2_coincident``) the reference's float32 matmul-form distance is rounding noise.  For the tensors with
one row per target (``l1_points``, ``l0_points``, the 3-NN weights and interpolated rows) ``*_dev`` is taken over the OTHER rows
where there are any (else over all rows), ``*_dev_all`` over all rows.  For the 3-NN weights and rows (``fp{1,2}_w``, ``fp{1,2}_rows``: the reference's
own dist_recip / norm on the distances it computed, and what it handed to the first layer of the propagation, columns
0 .. ROW_COLS) the float32 values of the coincident rows are not stored: float32(ref64) stands in their place.
"""
import contextlib
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
import pnpp_ref  # noqa: E402

RESO, FEAT, OUT_SIZE, SPARE, MARGIN, ROW_COLS = 16, 32, 64, 48, 1e-5, 32
CASES = [  # name, N, B, unet_type, cloud seed
    ("n700", 700, 1, "alto", 11), ("n1536b2", 1536, 2, "alto", 12), ("n300", 300, 1, "alto", 13),
    ("dup1024", 1024, 1, "alto", 14), ("n700u", 700, 1, "unet", 11)]
TENSORS = ("l3_points", "l2_points", "l1_points", "l0_points", "plane", "out", "heights")


def cfg_for(unet_type):
    cfg = make_cfg(depth=3, reso=RESO, hidden=FEAT)
    cfg["model"]["encoder"] = "pointnet_plus_plus"
    cfg["model"]["decoder_pixel_kwargs"]["output_size"] = OUT_SIZE
    cfg["model"]["encoder_kwargs"] = dict(feature_dim=FEAT, plane_resolution=RESO, unet_type=unet_type,
                                          unet_kwargs=dict(depth=3, merge_mode="concat", start_filts=32))
    return cfg


def cloud(n, b, seed, dup=0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(b, n, 2, generator=g).clamp(2.0 ** -20, 1 - 2.0 ** -20)
    z = torch.rand(b, n, 1, generator=g) * 0.6
    pts = torch.cat([xy, z], 2).float()
    if dup:                                                   # `dup` points repeat earlier ones: exact ties everywhere
        src = torch.randint(0, n - dup, (dup,), generator=g)
        pts[:, n - dup:] = pts[:, src]
        pts = pts[:, torch.randperm(n, generator=g)]
    starts = [torch.randint(0, n, (b,), generator=g), torch.randint(0, 128, (b,), generator=g)]
    return pts.contiguous(), starts


@contextlib.contextmanager
def fixed_randint(starts):
    queue, real = list(starts), torch.randint

    def fake(low, high, size, **kw):
        s = queue.pop(0)
        assert tuple(size) == tuple(s.shape) and int(s.max()) < high
        return s.clone()

    torch.randint = fake
    try:
        yield
    finally:
        torch.randint = real


def run(model, ref_pp, pts, starts, double):
    """One forward of the reference with everything the fixture stores recorded."""
    rec = {"fps": [], "ball": [], "sqd": []}
    orig = {k: getattr(ref_pp, k) for k in ("farthest_point_sample", "query_ball_point", "square_distance")}

    def wrap(name, key):
        def f(*a, **kw):
            out = orig[name](*a, **kw)
            rec[key].append(out.clone())
            return out
        setattr(ref_pp, name, f)

    wrap("farthest_point_sample", "fps"), wrap("query_ball_point", "ball"), wrap("square_distance", "sqd")
    enc = model.point_encoder
    outs, hooks = {}, []
    for k in ("sa1", "sa2", "sa3", "fp3", "fp2", "fp1"):
        hooks.append(getattr(enc, k).register_forward_hook(lambda m, i, o, k=k: outs.__setitem__(k, o)))
    gen = enc.generate_plane_features
    enc.generate_plane_features = lambda *a, **kw: outs.setdefault("plane", gen(*a, **kw))
    hooks.append(enc.register_forward_hook(lambda m, i, o: outs.__setitem__("out", o["xy"])))
    for k in ("fp2", "fp1"):          # what the propagation hands to its first layer: [points1 | interpolated], channels first
        hooks.append(getattr(enc, k).mlp_convs[0].register_forward_pre_hook(lambda m, i, k=k: outs.__setitem__(k + "_in", i[0].clone())))
    real_sample = torch.nn.functional.grid_sample
    if double:
        # torch.ones(B, N) of farthest_point_sample follows the default dtype; alto.py:93 casts the (float32-exact) sampling
        # coordinates with .float(), which grid_sample refuses beside a float64 plane: hand them over widened
        torch.set_default_dtype(torch.float64)
        torch.nn.functional.grid_sample = lambda inp, grid, **kw: real_sample(inp, grid.to(inp.dtype), **kw)
    try:
        with torch.no_grad(), fixed_randint(starts):
            heights, _ = model(input_cloud=pts.double() if double else pts)
    finally:
        torch.set_default_dtype(torch.float32)
        torch.nn.functional.grid_sample = real_sample
        for h in hooks:
            h.remove()
        del enc.generate_plane_features
        for k, v in orig.items():
            setattr(ref_pp, k, v)
    pm = lambda t: t.permute(0, 2, 1).contiguous()
    nn = lambda d: d.sort(dim=-1)[1][:, :, :3].contiguous()               # pointnetpp.py:91-92 on the recorded distances

    def weights(d):                                                       # pointnetpp.py:91-96 on the recorded distances
        dists = d.sort(dim=-1)[0][:, :, :3]
        dist_recip = 1.0 / (dists + 1e-8)
        return dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)

    return dict(fp2_w=weights(rec["sqd"][2]), fp1_w=weights(rec["sqd"][3]),
                fp2_rows=pm(outs["fp2_in"])[:, :, 128:128 + ROW_COLS].contiguous(), fp1_rows=pm(outs["fp1_in"])[:, :, :ROW_COLS].contiguous(),
                sa1_fps=rec["fps"][0], sa2_fps=rec["fps"][1], sa1_idx=rec["ball"][0], sa2_idx=rec["ball"][1],
                fp2_idx=nn(rec["sqd"][2]), fp1_idx=nn(rec["sqd"][3]), l3_points=pm(outs["sa3"][1]), l2_points=pm(outs["fp3"]),
                l1_points=pm(outs["fp2"]), l0_points=pm(outs["fp1"]), plane=outs["plane"], out=outs["out"], heights=heights)


INDEX_KEYS = ("sa1_fps", "sa2_fps", "sa1_idx", "sa2_idx", "fp2_idx", "fp1_idx")


def d2_64(a, b):
    d = a.double()[:, :, None, :] - b.double()[:, None, :, :]
    return (d * d).sum(-1)


def thin(pts, starts, r32, r64, n):
    """Delete ``pts.shape[1] - n`` points FPS never selected, the ambiguous ones first; the sa1 start index moves with them."""
    out, new_start = [], []
    for b in range(pts.shape[0]):
        total = pts.shape[1]
        selected = torch.zeros(total, dtype=torch.bool)
        selected[r64["sa1_fps"][b]] = True
        l1 = pts[b][r64["sa1_fps"][b]][None]
        near = ((d2_64(l1, pts[b][None])[0] - 0.2 ** 2).abs() < MARGIN).any(0)
        differ = (r32["fp1_idx"][b] != r64["fp1_idx"][b]).any(-1)
        bad = (near | differ) & ~selected
        spare = total - n
        if int(bad.sum()) > spare:
            return None
        drop = bad.clone()
        for i in range(total - 1, -1, -1):                                # then others, from the end
            if int(drop.sum()) == spare:
                break
            if not selected[i] and not drop[i]:
                drop[i] = True
        if int(drop.sum()) != spare:
            return None
        out.append(pts[b][~drop])
        s = int(starts[0][b])
        new_start.append(s - int(drop[:s].sum()))
    return torch.stack(out).contiguous(), [torch.tensor(new_start, dtype=torch.long), starts[1]]


def main():
    ref = import_reference()
    from tomosar2height.encoder import pointnetpp as ref_pp
    arrays = {"cases": np.array([c[0] for c in CASES]), "margin": MARGIN, "resolution": RESO, "feature_dim": FEAT,
              "output_size": OUT_SIZE, "row_cols": ROW_COLS}
    keys_written = False
    for name, n, b, unet_type, seed in CASES:
        dup = 64 if name.startswith("dup") else 0
        model = pnpp_ref.init_pnpp_(ref.TomoSAR2Height(cfg_for(unet_type)), seed=41).eval()
        model64 = copy.deepcopy(model).double()
        if not keys_written:
            sd = model.point_encoder.state_dict()
            arrays["state_keys"] = np.array(list(sd.keys()))
            arrays["state_shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
            keys_written = True
        for attempt in range(40):
            if dup:
                pts, starts = cloud(n, b, seed + 100 * attempt, dup)
            else:
                big, starts = cloud(n + SPARE, b, seed + 100 * attempt)
                starts[0] = starts[0] % n
                if n < 512:                                               # below npoint every point is selected: nothing to delete
                    pts = big[:, :n].contiguous()
                else:
                    thinned = thin(big, starts, run(model, ref_pp, big, starts, False), run(model64, ref_pp, big, starts, True), n)
                    if thinned is None:
                        continue
                    pts, starts = thinned
            r32, r64 = run(model, ref_pp, pts, starts, False), run(model64, ref_pp, pts, starts, True)
            same = all(torch.equal(r32[k], r64[k]) for k in INDEX_KEYS)
            if same or dup:
                break
            print(f"  {name}: attempt {attempt} ambiguous:", [k for k in INDEX_KEYS if not torch.equal(r32[k], r64[k])])
        assert dup or all(torch.equal(r32[k], r64[k]) for k in INDEX_KEYS), name          # the condition, not the margin
        assert torch.equal(r32["sa1_fps"][:, 0], starts[0]) and torch.equal(r32["sa2_fps"][:, 0], starts[1])
        assert pts.shape == (b, n, 3)
        arrays[f"{name}_points"] = pts.numpy()
        arrays[f"{name}_unet_type"] = unet_type
        arrays[f"{name}_unambiguous"] = not dup
        arrays[f"{name}_attempt"] = attempt
        arrays[f"{name}_start1"], arrays[f"{name}_start2"] = starts[0].numpy(), starts[1].numpy()
        for k in INDEX_KEYS:
            arrays[f"{name}_{k}"] = r32[k].numpy().astype(np.int32)
            if dup:
                arrays[f"{name}_{k}_64"] = r64[k].numpy().astype(np.int32)
        # the coincident rows of the two propagations: float64 d2_min by differences below 1e-12
        l1 = torch.stack([pts[i][r64["sa1_fps"][i]] for i in range(b)])
        l2 = torch.stack([l1[i][r64["sa2_fps"][i]] for i in range(b)])
        arrays[f"{name}_fp1_coincident"] = (d2_64(pts, l1).min(-1)[0] < 1e-12).numpy()
        arrays[f"{name}_fp2_coincident"] = (d2_64(l1, l2).min(-1)[0] < 1e-12).numpy()
        per_target = {"l1_points": "fp2", "l0_points": "fp1", "fp2_w": "fp2", "fp1_w": "fp1", "fp2_rows": "fp2", "fp1_rows": "fp1"}
        for k in TENSORS + tuple(per_target)[2:]:
            a32, a64 = r32[k].numpy().copy(), r64[k].numpy()
            mask = arrays[f"{name}_{per_target[k]}_coincident"] if k in per_target else None
            if mask is not None and k not in TENSORS:
                a32[mask] = a64[mask].astype(np.float32)                  # the reference's float32 noise is not stored
            diff = np.abs(a32.astype(np.float64) - a64)
            dev_all = float(np.abs(r32[k].numpy().astype(np.float64) - a64).max())
            # (a cloud below npoint has no other rows: the figure over all rows, the plain max|ref32 - ref64|, stands)
            dev = float(diff[~mask].max()) if mask is not None and (~mask).any() else dev_all
            arrays[f"{name}_{k}"] = a32
            arrays[f"{name}_{k}_dev"] = dev
            if mask is not None:
                arrays[f"{name}_{k}_dev_all"] = dev_all
            q = (a64 - a32.astype(np.float64)) / (dev if dev > 0 else 1.0)
            assert np.abs(q).max() < 6e4, (name, k)
            arrays[f"{name}_{k}_q"] = q.astype(np.float16)
            print(f"  {name} {k}: shape {a32.shape} max|x| {np.abs(a64).max():.3g} ref32_dev {dev:.3g} (all rows {dev_all:.3g})")
        print(f"{name}: attempt {attempt}, coincident fp1 {int(arrays[f'{name}_fp1_coincident'].sum())} "
              f"fp2 {int(arrays[f'{name}_fp2_coincident'].sum())}")
    save("pnpp_encoder", **arrays)


if __name__ == "__main__":
    main()
