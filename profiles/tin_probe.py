"""What does the device Delaunay-linear baseline cost at the Berlin chunk's size, and where does the time go?  

    python profiles/tin_probe.py [--out FILE, default profiles/r11_tin.txt] [--points 3000000] [--repeats 20] [--warmup 3] [--no-host]

Raster and cloud: those of profiles/interp_probe.py (1660 x 1990 nodes at 1 m; a few million points with holes, facades and
duplicates at UTM-sized offsets).  HIP events around the hull (on a fresh index each time: the index caches it), ``delaunay_dsm``
and ``grid_simplex`` on an existing index, separately, with the status counts of the search.  Beside them, for context only,
``scipy.interpolate.griddata(method='linear')`` on this host, once, on the shifted unique cloud, and the largest gap between the
two rasters in units of 2^-52 max|z| of the cloud (nodes whose triangles differ -- cocircular quadruples of this millimetre
grid -- included: the interpolant is continuous).  No time is asserted anywhere.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from interp_probe import berlin_cloud, fmt, timed  # noqa: E402
from tomosar2height_amd import CloudIndex, delaunay_dsm, grid_simplex, interpolate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_tin.txt"))
    ap.add_argument("--points", type=int, default=3_000_000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the griddata timing on the host")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host_pts = berlin_cloud(args.points)
    N = len(host_pts)
    pts = torch.from_numpy(host_pts).to(dev)
    index = CloudIndex(pts)

    def fresh_hull():
        index._hull = None
        return index.hull()

    hull, hull_ms = timed(fresh_hull, args.warmup, args.repeats)
    (dsm, origin, status), dsm_ms = timed(lambda: delaunay_dsm(index, return_status=True), args.warmup, args.repeats)
    (tri, bary), tri_ms = timed(lambda: grid_simplex(index), args.warmup, args.repeats)
    ny, nx = index.grid_shape()
    M, (gy, gx), h = index.n_unique, index.cells, index.cell_edge
    nan = torch.isnan(dsm).float().mean().item()
    inside = ny * nx * (1.0 - nan)
    lines = [
        f"Delaunay-linear probe: {N} points -> {M} distinct (x, y); raster {ny} x {nx} = {ny * nx} nodes at 1 m",
        f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}, HIP events",
        f"cell grid                         : {gy} x {gx} cells of {h:.4f} m, {M / (gx * gy):.2f} distinct points per cell",
        f"hull (4 launches + status copy)   : {fmt(hull_ms)}",
        f"HULL SURVIVORS                    : {index.hull_survivors} of {M} points passed the polygon filter and are sorted and chained by "
        f"ONE workgroup ({100.0 * index.hull_survivors / M:.4f} %; this is the hull's serial tail); {hull.shape[0]} hull vertices",
        f"delaunay_dsm on the index         : {fmt(dsm_ms)}  [{interpolate.LAUNCHES_PER_TIN_RASTER} launches + status copy]",
        f"grid_simplex on the index         : {fmt(tri_ms)}",
        f"nodes outside the hull            : {100 * nan:.2f} %",
        f"search status                     : {status}  ({status['pivots'] / inside:.3f} verification and "
        f"{status['walk_pivots'] / inside:.2f} walk pivots per inside node)",
        f"raster floor (cloud + offsets + raster once): {(24 * M + 4 * gx * gy + 8 * ny * nx) / 1e6:.1f} MB",
    ]
    if not args.no_host:
        from scipy.interpolate import griddata
        u = index.unique.cpu().numpy()
        xs, ys = u[:, 0] - origin[0], u[:, 1] - origin[1]
        grid_y, grid_x = np.mgrid[ys.min():ys.max():1.0, xs.min():xs.max():1.0]
        t0 = time.perf_counter()
        host = griddata((xs, ys), u[:, 2], (grid_x, grid_y), method="linear")
        host_ms = (time.perf_counter() - t0) * 1e3
        got = dsm.cpu().numpy()
        both = ~np.isnan(host) & ~np.isnan(got)
        gap = np.abs(got - host)[both].max() / (2.0 ** -52 * np.abs(u[:, 2]).max())
        lines += [
            f"host: griddata(method='linear') on the shifted unique cloud: {host_ms:.1f} ms "
            f"({host_ms / (statistics.median(hull_ms) + statistics.median(dsm_ms)):.0f} x hull + delaunay_dsm)",
            f"NaN masks differ on               : {int((np.isnan(host) != np.isnan(got)).sum())} nodes",
            f"raster vs the host's              : largest gap {gap:.2f} x 2^-52 max|z| of the cloud, all nodes finite in both",
        ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
