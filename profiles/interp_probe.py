"""What do the device interpolation baselines cost at the Berlin chunk's size, and where does the time go?  

    python profiles/interp_probe.py [--out FILE] [--points 3000000] [--repeats 20] [--warmup 3]

Raster: the Berlin test chunk's, 1660 x 1990 at 1 m.  Cloud: synthetic, a few million points -- a uniform scatter with circular
holes tens of metres wide, dense lines (facades) and 8 % exact duplicates of (x, y) -- at UTM-sized offsets.  HIP events around
``CloudIndex`` (bounds + index + the one table copy), ``nearest_dsm`` and ``idw_dsm`` on an existing index, separately.  Beside
them the reference's own method on this host, once: pandas group-by, ``cKDTree`` build, ``query`` for k = 1 and k = 8 with the
IDW arithmetic, and the copy of the cloud to the host that path needs first.  The two rasters are compared on the way
(nearest: share of equal pixels, the rest being rank-1 ties; IDW: largest gap in units of 2^-53 max|z| over pixels without a
rank-8 tie).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tomosar2height_amd import CloudIndex, idw_dsm, interpolate, nearest_dsm  # noqa: E402


def berlin_cloud(n, seed=23, W=1990.0, H=1660.0):
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * (W, H)
    for _ in range(60):                                           # holes of 15 .. 50 m radius
        c, r = rng.random(2) * (W, H), rng.uniform(15.0, 50.0)
        xy = xy[np.hypot(xy[:, 0] - c[0], xy[:, 1] - c[1]) > r]
    lines = []
    for _ in range(300):                                          # facades: 4 000 points on 40 .. 120 m, 5 cm across
        a, ang, length = rng.random(2) * (W - 150, H - 150), rng.uniform(0, np.pi / 2), rng.uniform(40.0, 120.0)
        t = rng.random(4000) * length
        lines.append(np.c_[a[0] + t * np.cos(ang), a[1] + t * np.sin(ang)] + rng.standard_normal((4000, 2)) * 0.05)
    xy = np.r_[xy, np.concatenate(lines), [[0.0, 0.0], [W, H]]]
    xy = np.clip(np.round(xy / 0.001) * 0.001, 0.0, (W, H))
    z = 35.0 + 10.0 * np.sin(xy[:, 0] / 90.0) + rng.standard_normal(len(xy)) * 3.0
    dup = rng.choice(len(xy), len(xy) * 8 // 100, replace=False)
    xy, z = np.r_[xy, xy[dup]], np.r_[z, z[dup] + rng.standard_normal(len(dup)) * 5.0]
    order = rng.permutation(len(xy))
    return np.c_[392000.0 + xy[order, 0], 5820000.0 + xy[order, 1], z[order]]


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return out, ms


def fmt(ms):
    return f"median {statistics.median(ms):.3f} ms, min {min(ms):.3f} ms, max {max(ms):.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=int, default=3_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the pandas / k-d tree timing on the host")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host_pts = berlin_cloud(args.points)
    N = len(host_pts)
    pts = torch.from_numpy(host_pts).to(dev)
    index, index_ms = timed(lambda: CloudIndex(pts), args.warmup, args.repeats)
    (near, origin), near_ms = timed(lambda: nearest_dsm(index), args.warmup, args.repeats)
    (idw, _), idw_ms = timed(lambda: idw_dsm(index), args.warmup, args.repeats)
    ny, nx = index.grid_shape()
    M, (gy, gx), h = index.n_unique, index.cells, index.cell_edge
    ws = interpolate._lib.ws_bytes("t2h_interp_index_workspace_bytes", N)
    lines = [
        f"interpolation probe: {N} points -> {M} distinct (x, y); raster {ny} x {nx} = {ny * nx} nodes at 1 m",
        f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}, HIP events",
        f"cell grid                         : {gy} x {gx} cells of {h:.4f} m, {M / (gx * gy):.2f} distinct points per cell",
        f"CloudIndex (bounds, index, copy)  : {fmt(index_ms)}  [{interpolate.LAUNCHES_PER_BOUNDS + interpolate.LAUNCHES_PER_INDEX}"
        f" launches, workspace {ws / 1e6:.1f} MB]",
        f"nearest_dsm on the index          : {fmt(near_ms)}  [1 launch]",
        f"idw_dsm (k = 8) on the index      : {fmt(idw_ms)}  [1 launch]",
        f"index bytes (model: 200 B / point): {200 * N / 1e6:.1f} MB -> {200 * N / statistics.median(index_ms) / 1e6:.1f} GB/s",
        f"raster floor (cloud + offsets + raster once): {(24 * M + 4 * gx * gy + 8 * ny * nx) / 1e6:.1f} MB",
    ]
    if not args.no_host:
        import pandas as pd
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        back = pts.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        df = pd.DataFrame(back, columns=["X", "Y", "Z"]).groupby(["X", "Y"], as_index=False).max()
        group_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        tree = cKDTree(df[["X", "Y"]].values)
        tree_ms = (time.perf_counter() - t0) * 1e3
        gy_, gx_ = np.mgrid[df["Y"].min():df["Y"].max():1.0, df["X"].min():df["X"].max():1.0]
        q = np.c_[gx_.ravel(), gy_.ravel()]
        t0 = time.perf_counter()
        d1, i1 = tree.query(q, workers=-1)
        host_near = df["Z"].values[i1].reshape(gx_.shape)
        q1_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        d8, i8 = tree.query(q, k=9)                               # (the ninth only to know where rank 8 ties)
        q9_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        dist, i8k = tree.query(q, k=8)
        w = np.zeros_like(dist)
        zero = dist == 0
        w[zero] = 1
        w[~zero] = 1 / dist[~zero] ** 2
        w /= w.sum(axis=1, keepdims=True)
        host_idw = (w * df["Z"].values[i8k]).sum(axis=1).reshape(gx_.shape)
        q8_ms = (time.perf_counter() - t0) * 1e3
        assert len(df) == M and host_near.shape == (ny, nx) and origin == (df["X"].min(), df["Y"].min())
        same = near.cpu().numpy() == host_near
        untied = (d8[:, 7] != d8[:, 8]).reshape(ny, nx)
        unit = 2.0 ** -53 * np.abs(df["Z"].values).max()
        gap = np.abs(idw.cpu().numpy() - host_idw)[untied].max() / unit
        lines += [
            f"host: copy of the cloud           : {copy_ms:.1f} ms",
            f"host: pandas group-by max         : {group_ms:.1f} ms",
            f"host: cKDTree build               : {tree_ms:.1f} ms",
            f"host: query k = 1 (workers = -1, {os.cpu_count()} CPUs visible) + gather: {q1_ms:.1f} ms",
            f"host: query k = 8 (one worker, as the script) + IDW arithmetic: {q8_ms:.1f} ms   (k = 9 for the tie mask: {q9_ms:.1f} ms)",
            f"host / device, nearest end to end : {(copy_ms + group_ms + tree_ms + q1_ms) / (statistics.median(index_ms) + statistics.median(near_ms)):.1f} x",
            f"host / device, IDW end to end     : {(copy_ms + group_ms + tree_ms + q8_ms) / (statistics.median(index_ms) + statistics.median(idw_ms)):.1f} x",
            f"nearest raster equal to the host's: {100 * same.mean():.4f} % of nodes (the rest: rank-1 ties resolved by (d2, X, Y))",
            f"IDW raster vs the host's          : largest gap {gap:.2f} x 2^-53 max|z| over the {100 * untied.mean():.2f} % of nodes "
            "without a rank-8 tie (bound 32)",
        ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
