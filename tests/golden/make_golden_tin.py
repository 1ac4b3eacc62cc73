"""Writes tests/golden/tin_baseline.npz: the Delaunay-linear baseline of the reference's scripts/interpolate_bilinear.py, run on
coordinates shifted to the cloud's (xmin, ymin) (build container only; needs scipy and pandas, the tests need numpy alone).

    python tests/golden/make_golden_tin.py

The script's own steps -- pandas group-by maximum, ``np.mgrid``, ``scipy.interpolate.griddata(method='linear')`` -- are applied
to ``X - xmin``, ``Y - ymin``; ``scipy.spatial.Delaunay(...).find_simplex`` gives the triangle of every node.  On the raw UTM
coordinates Qhull drops a large share of the points as ``coplanar`` (its lifted paraboloid's z of 3.4e13 swallows them) and the
script interpolates over a triangulation of the rest: that count is recorded per case for the documents, and is why the
device form is defined on shifted coordinates (DESIGN.md sections 4.8 and 7).

Coordinates are ``offset + d`` with d a multiple of 2^-16 below 256, offsets (389 000, 5 819 000): the shift is exact, and
every orientation test on shifted coordinates is exact in float64 (24-bit numbers, 51-bit determinants).

Asserted here and recorded per case: (a) Qhull drops no point on shifted coordinates; (b) general position, in exact integer
arithmetic: for every interior Delaunay edge the in-circle determinant of the two opposite vertices is nonzero; (c) the share
of AMBIGUOUS nodes -- finite in the reference, smallest |lambda| there below 2^-30 -- is at most 0.5 % of the finite nodes.
``units_bound``: the next power of two at or above four times the largest distance between the restatement (tests/tin_ref.py,
evaluated on find_simplex's triangles) and griddata, in units of 2^-52 * max|z| of a node's three vertices.
"""
import math
import os
import sys

import numpy as np
import pandas as pd
from scipy.interpolate import griddata
from scipy.spatial import Delaunay

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import tin_ref  # noqa: E402

X0, Y0 = 389000.0, 5819000.0
Q = 65536.0
AMBIGUOUS = 2.0 ** -30
EXCLUSION_CAP = 0.005


def cloud(seed, M, W, H, clustered=False, extra=()):
    """M points on W x H m (multiples of 2^-16), `extra` appended, then 10 % duplicated (X, Y) with another height."""
    r = np.random.default_rng(seed)
    xy = r.random((M, 2)) * (W, H)
    if clustered:
        xy[:M // 2] = r.random((M // 2, 2)) ** 3 * (W, H)
    xy = np.floor(xy * Q) / Q
    on_axis = (xy < 0.0625).any(1)                               # cubed coordinates pile up on the axes: rows of collinear hull points
    xy[on_axis] = np.floor(r.random((int(on_axis.sum()), 2)) * (W, H) * Q) / Q
    if len(extra):
        xy = np.r_[xy, np.asarray(extra, np.float64)]
    z = np.round((r.random(len(xy)) * 60 + 30) * 1024) / 1024
    src = r.integers(0, len(xy), len(xy) // 10)
    xy = np.r_[xy, xy[src]]
    z = np.r_[z, np.round((r.random(len(src)) * 60 + 30) * 1024) / 1024]
    order = r.permutation(len(xy))
    assert xy.max() < 256
    return np.c_[X0 + xy[order, 0], Y0 + xy[order, 1], z[order]]


CASES = {
    "tiny": (lambda: cloud(20250101, 60, 12, 10), 1.0),
    "mid": (lambda: cloud(20250102, 2000, 48, 40), 1.0),
    "fine": (lambda: cloud(20250103, 2000, 48, 40), 0.5),
    "clustered": (lambda: cloud(20250104, 4000, 64, 64, clustered=True), 1.0),
    "strip": (lambda: cloud(20250105, 300, 40, 3), 0.5),
    # (0, 0) pins the origin and is itself node (0, 0), a hull vertex; (7, 5) and (11.5, 3) are interior nodes at 0.5
    "on_node": (lambda: cloud(20250106, 500, 24, 20, extra=[(0.0, 0.0), (7.0, 5.0), (11.5, 3.0)]), 0.5),
}


def incircle_exact(a, b, c, d):
    """Exact in-circle determinant of four integer points (Python integers)."""
    m = [(p[0] - d[0], p[1] - d[1]) for p in (a, b, c)]
    m = [(x, y, x * x + y * y) for x, y in m]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
            m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def general_position(dt, P):
    ints = [(int(round(x * Q)), int(round(y * Q))) for x, y in P]
    assert np.array_equal(np.array(ints, np.float64) / Q, P)
    edges = 0
    for s, (verts, nbrs) in enumerate(zip(dt.simplices, dt.neighbors)):
        for k in range(3):
            n = nbrs[k]
            if n < s:                                            # -1: a hull edge; each interior edge once
                continue
            opposite = [v for v in dt.simplices[n] if v not in verts]
            assert len(opposite) == 1
            if incircle_exact(*(ints[v] for v in verts), ints[opposite[0]]) == 0:
                return False, edges
            edges += 1
    return True, edges


def main():
    out = {"cases": np.array(list(CASES))}
    worst = 0.0
    for name, (make, res) in CASES.items():
        pts = make()
        df = pd.DataFrame(pts, columns=["X", "Y", "Z"])
        top = df.groupby(["X", "Y"], as_index=False).max()
        ref_unique = top[["X", "Y", "Z"]].values
        unique = tin_ref.unique_cloud(pts)
        assert unique.tobytes() == np.ascontiguousarray(ref_unique).tobytes() and len(unique) < len(pts)
        xmin, ymin = top["X"].min(), top["Y"].min()
        xs, ys, zs = top["X"].values - xmin, top["Y"].values - ymin, top["Z"].values
        P, origin = tin_ref.shifted(unique)
        assert origin == (xmin, ymin) and np.array_equal(P, np.c_[xs, ys]) and np.array_equal(P + origin, unique[:, :2])
        grid_y, grid_x = np.mgrid[ys.min():ys.max():res, xs.min():xs.max():res]
        qx, qy = tin_ref.nodes(unique, res)
        assert np.array_equal(grid_x[0], qx) and np.array_equal(grid_y[:, 0], qy)
        dsm = griddata((xs, ys), zs, (grid_x, grid_y), method="linear")
        dt = Delaunay(np.c_[xs, ys])
        q = np.c_[grid_x.ravel(), grid_y.ravel()]
        simplex = dt.find_simplex(q)
        inside = simplex >= 0
        assert np.array_equal(np.isnan(dsm).ravel(), ~inside)
        tri = np.full((len(q), 3), -1, np.int32)
        tri[inside] = np.sort(dt.simplices[simplex[inside]], axis=1)
        T = dt.transform[simplex[inside]]
        b = np.einsum("nij,nj->ni", T[:, :2], q[inside] - T[:, 2])
        lam = np.c_[b, 1 - b.sum(1)]
        ambiguous = np.zeros(len(q), bool)
        ambiguous[inside] = np.abs(lam).min(1) < AMBIGUOUS
        tri, ambiguous = tri.reshape(dsm.shape + (3,)), ambiguous.reshape(dsm.shape)

        coplanar = len(dt.coplanar)                                                 # (a)
        assert coplanar == 0, (name, coplanar)
        general, edges = general_position(dt, P)                                    # (b)
        assert general, name
        share = ambiguous.sum() / inside.sum()                                      # (c)
        assert share <= EXCLUSION_CAP, (name, share)
        coplanar_raw = len(Delaunay(unique[:, :2]).coplanar)                        # (d)

        mine = tin_ref.linear(unique, tri, res)
        assert np.array_equal(np.isnan(mine), np.isnan(dsm))
        u = tin_ref.units(mine, dsm, unique, tri)
        gap = float(np.nanmax(np.where(ambiguous, np.nan, u)))
        worst = max(worst, gap)
        if len(unique) <= 64:
            brute, count = tin_ref.brute_force(unique, res)
            clear = ~ambiguous
            assert np.array_equal(brute[clear], tri[clear]) and (count[clear & inside.reshape(count.shape)] == 1).all()
            assert (count[~inside.reshape(count.shape)] == 0).all()
        on_point = int(((np.abs(lam - 1.0) < 1e-12).any(1)).sum())
        print(f"{name}: N = {len(pts)}, M = {len(unique)}, raster {dsm.shape} at {res}, NaN {np.isnan(dsm).mean():.1%}, "
              f"ambiguous {int(ambiguous.sum())}, nodes on a point {on_point}, interior edges {edges}, coplanar raw {coplanar_raw}, "
              f"restatement vs griddata {gap:.2f} units (p99 {np.nanpercentile(u, 99):.2f})")
        out.update({f"{name}_points": pts, f"{name}_resolution": np.float64(res), f"{name}_dsm": dsm, f"{name}_tri": tri,
                    f"{name}_ambiguous": ambiguous, f"{name}_coplanar": np.int64(coplanar),
                    f"{name}_coplanar_raw": np.int64(coplanar_raw), f"{name}_general_position": np.bool_(general),
                    f"{name}_ambiguous_share": np.float64(share), f"{name}_units": np.float64(gap)})
    bound = 2.0 ** math.ceil(math.log2(4.0 * worst))
    out["units_bound"] = np.float64(bound)
    print(f"largest distance {worst:.2f} units -> units_bound {bound}")
    path = os.path.join(HERE, "tin_baseline.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
