"""numpy restatement of the PointNet++ point stages (include/t2h_pnpp.h, tomosar2height_amd/pointops.py) with their exact fp32
expressions and tie rules, plus the deterministic parameter fill the fixture generator and the tests share.

    d2(p, c) = ((dx * dx + dy * dy) + dz * dz), every operation rounded once in float32
    FPS:   distance = min(distance, d2) from 1e10; next centroid = the lowest index of the largest distance
    ball:  the first nsample indices in index order with NOT (d2 > radius2), padded with the first; N if there is none
    3-NN:  the three smallest d2, equal d2 by ascending index; r = 1 / (d2 + 1e-8), w = r / ((r0 + r1) + r2),
           out = (p0 * w0 + p1 * w1) + p2 * w2
Single clouds ([N, 3]); the callers loop over the batch.
"""
import zlib

import numpy as np
import torch

from detinit import det_init_

F = np.float32


def d2(p, c):
    p, c = np.asarray(p, F), np.asarray(c, F)
    dx, dy, dz = p[..., 0] - c[..., 0], p[..., 1] - c[..., 1], p[..., 2] - c[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def fps(xyz, npoint, start):
    xyz = np.asarray(xyz, F)
    dist = np.full(xyz.shape[0], 1e10, F)
    out = np.empty(npoint, np.int64)
    cur = int(start)
    for k in range(npoint):
        out[k] = cur
        dist = np.minimum(dist, d2(xyz, xyz[cur]))
        cur = int(np.argmax(dist))                       # (numpy: the first of equal maxima)
    return out


def ball_query(radius, nsample, xyz, new_xyz):
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    r2 = F(float(radius) ** 2)
    n = xyz.shape[0]
    out = np.empty((new_xyz.shape[0], nsample), np.int64)
    for s, q in enumerate(new_xyz):
        inside = np.flatnonzero(~(d2(xyz, q) > r2))[:nsample]
        first = inside[0] if inside.size else n
        out[s, :inside.size] = inside
        out[s, inside.size:] = first
    return out


def group_rows(xyz, new_xyz, points, idx, ld=None):
    xyz, new_xyz = np.asarray(xyz, F), np.asarray(new_xyz, F)
    s, ns = idx.shape
    d = 0 if points is None else points.shape[1]
    ld = 3 + d if ld is None else ld
    rows = np.zeros((s, ns, ld), F)
    rows[:, :, :3] = xyz[idx] - new_xyz[:, None, :]
    if points is not None:
        rows[:, :, 3:3 + d] = np.asarray(points, F)[idx]
    return rows.reshape(s * ns, ld)


def group_max(rows, nsample):
    return rows.reshape(-1, nsample, rows.shape[1]).max(axis=1)


def three_nn(xyz1, xyz2):
    """-> idx [N, 3] int64, weight [N, 3] float32, d2 of the three [N, 3]."""
    xyz1, xyz2 = np.asarray(xyz1, F), np.asarray(xyz2, F)
    if xyz2.shape[0] == 1:
        n = xyz1.shape[0]
        return np.zeros((n, 3), np.int64), np.tile(np.array([1, 0, 0], F), (n, 1)), np.zeros((n, 3), F)
    dist = d2(xyz1[:, None, :], xyz2[None, :, :])
    idx = np.argsort(dist, axis=1, kind="stable")[:, :3]
    dd = np.take_along_axis(dist, idx, 1)
    r = F(1.0) / (dd + F(1e-8))
    norm = (r[:, 0] + r[:, 1]) + r[:, 2]
    return idx.astype(np.int64), r / norm[:, None], dd


def interpolate(points2, idx, weight):
    p = np.asarray(points2, F)
    if p.shape[0] == 1:
        return np.repeat(p, idx.shape[0], axis=0)
    return (p[idx[:, 0]] * weight[:, 0:1] + p[idx[:, 1]] * weight[:, 1:2]) + p[idx[:, 2]] * weight[:, 2:3]


# ------------------------------------------------------------------------------------------------ parameters
def init_pnpp_(model: torch.nn.Module, seed: int) -> torch.nn.Module:
    """``det_init_`` for the parameters, then name-keyed non-trivial BatchNorm affine parameters and running statistics:
    gamma in [0.75, 1.25), beta in [-0.1, 0.1), running_mean in [-0.1, 0.1), running_var in [0.5, 1.5)."""
    det_init_(model, seed=seed)
    with torch.no_grad():
        for name, m in sorted(model.named_modules()):
            if not isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                continue
            g = torch.Generator().manual_seed((seed * 1000003 + zlib.crc32(("bn:" + name).encode())) % (2 ** 31))
            u = torch.rand(4, m.num_features, generator=g, dtype=torch.float32)
            m.weight.copy_(0.75 + 0.5 * u[0])
            m.bias.copy_(0.2 * u[1] - 0.1)
            m.running_mean.copy_(0.2 * u[2] - 0.1)
            m.running_var.copy_(0.5 + u[3])
            m.num_batches_tracked.fill_(7)
    return model


def folded_layers(stage):
    """[(W' float32 [out, in], b' float32 [out])] of a stage's ``mlp_convs`` / ``mlp_bns``: the BatchNorm running statistics
    folded in float64, rounded once."""
    out = []
    for conv, bn in zip(stage.mlp_convs, stage.mlp_bns):
        s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
        w = conv.weight.detach().reshape(conv.weight.shape[0], -1).double() * s[:, None]
        b = (conv.bias.double() - bn.running_mean.double()) * s + bn.bias.double()
        out.append((w.detach().float().numpy(), b.detach().float().numpy()))
    return out


def chain(rows, layers):
    for w, b in layers:
        rows = np.maximum(rows[:, :w.shape[1]] @ w.T + b, F(0))
    return rows


def encoder_points(enc, xyz, start1, start2):
    """The point side of PointNetPlusPlus.forward (pointnetpp.py:152-163) for one cloud [N, 3] on the restatement: a dict of
    every level's indices and features (l0_points in the cloud's own order)."""
    xyz = np.asarray(xyz, F)
    o = {}
    sa1, sa2, sa3, fp3, fp2, fp1 = (folded_layers(getattr(enc, k)) for k in ("sa1", "sa2", "sa3", "fp3", "fp2", "fp1"))
    o["sa1_fps"] = fps(xyz, enc.sa1.npoint, start1)
    l1_xyz = xyz[o["sa1_fps"]]
    o["sa1_idx"] = ball_query(enc.sa1.radius, enc.sa1.nsample, xyz, l1_xyz)
    o["sa1_points"] = group_max(chain(group_rows(xyz, l1_xyz, xyz, o["sa1_idx"]), sa1), enc.sa1.nsample)
    o["sa2_fps"] = fps(l1_xyz, enc.sa2.npoint, start2)
    l2_xyz = l1_xyz[o["sa2_fps"]]
    o["sa2_idx"] = ball_query(enc.sa2.radius, enc.sa2.nsample, l1_xyz, l2_xyz)
    o["sa2_points"] = group_max(chain(group_rows(l1_xyz, l2_xyz, o["sa1_points"], o["sa2_idx"]), sa2), enc.sa2.nsample)
    o["l3_points"] = chain(np.concatenate([l2_xyz, o["sa2_points"]], 1), sa3).max(axis=0, keepdims=True)
    o["l2_points"] = chain(np.concatenate([o["sa2_points"], np.repeat(o["l3_points"], l2_xyz.shape[0], 0)], 1), fp3)
    o["fp2_idx"], w, _ = three_nn(l1_xyz, l2_xyz)
    o["l1_points"] = chain(np.concatenate([o["sa1_points"], interpolate(o["l2_points"], o["fp2_idx"], w)], 1), fp2)
    o["fp1_idx"], w, _ = three_nn(xyz, l1_xyz)
    o["l0_points"] = chain(interpolate(o["l1_points"], o["fp1_idx"], w), fp1)
    return o


# ------------------------------------------------------------------------------------------------ fixture access
def model_cfg(unet_type: str, g):
    """The configuration tests/golden/make_golden_pnpp.py built its reference models with."""
    from tomosar2height_amd.config import berlin_config
    cfg = berlin_config()
    cfg.model.encoder = "pointnet_plus_plus"
    cfg.model.encoder_kwargs = dict(feature_dim=int(g["feature_dim"]), plane_resolution=int(g["resolution"]), unet_type=unet_type,
                                    unet_kwargs=dict(depth=3, merge_mode="concat", start_filts=32))
    cfg.model.decoder_pixel_kwargs.output_size = int(g["output_size"])
    return cfg


def ref64(g, name, key):
    """(ref64, tolerance): the float64 result rebuilt from the stored float32 one, and 4 x max|ref32 - ref64|."""
    dev = float(g[f"{name}_{key}_dev"])
    return g[f"{name}_{key}"].astype(np.float64) + g[f"{name}_{key}_q"].astype(np.float64) * dev, 4.0 * dev


def coincident(targets, sources):
    """Rows of ``targets`` [N, 3] whose float64 d2 by differences to the nearest of ``sources`` [S, 3] is below 1e-12."""
    d = targets.astype(np.float64)[:, None, :] - sources.astype(np.float64)[None, :, :]
    return (d * d).sum(-1).min(-1) < 1e-12


def check_three_nn(g, name, level, b, weight, rows, say=print):
    """The issue's 3-NN comparison for cloud ``b`` of a case at ``level`` ('fp1' / 'fp2'): ``weight`` [N, 3] and ``rows``
    [N, >= row_cols] within 4 x ref32_dev of the float64 reference on ALL rows and of the float32 reference on the
    non-coincident rows; the excluded rows are exactly ``{level}_coincident``.  Returns the mask."""
    mask = g[f"{name}_{level}_coincident"][b]
    cols = int(g["row_cols"])
    for key, got in ((f"{level}_w", weight), (f"{level}_rows", rows[:, :cols])):
        want64, tol = ref64(g, name, key)
        want32 = g[f"{name}_{key}"][b]
        e64 = np.abs(got.astype(np.float64) - want64[b]).max()
        e32 = np.abs(got.astype(np.float64) - want32.astype(np.float64))[~mask].max() if (~mask).any() else 0.0
        say(f"{name}[{b}] {key}: max err vs ref64 (all rows) {e64:.3g}, vs ref32 ({int((~mask).sum())} non-coincident rows) {e32:.3g}, "
            f"tolerance {tol:.3g}")
        assert e64 <= tol and e32 <= tol, (name, b, key, e64, e32, tol)
    return mask
