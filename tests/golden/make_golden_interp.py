"""Writes tests/golden/interp_baselines.npz from the reference's own scripts/interpolate_nearest.py and
scripts/interpolate_idw.py (build container only).

    python tests/golden/make_golden_interp.py

The two scripts are run where they lie (``runpy``).  laspy and rasterio are not installed: ``laspy.read`` is a stand-in that
returns an in-memory cloud, ``rasterio.open(...).write`` and ``rasterio.transform.from_origin`` capture what the script
writes.  pandas and scipy are the real ones.  Stored per case: the input points, the two rasters, their origins, the row of
the input each row of the script's group-by result came from, and the distances the script's k-d tree reports for k = 8 (the
tree is the script's own object, queried once more).  The shares of pixels whose k-th and (k + 1)-th neighbours tie -- left out
of the comparison with the reference, since the tree may return either -- are asserted here as tests/test_interp_cpu.py states
them, and the measured gap between the restatement and the reference is printed.
"""
import os
import runpy
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402
import interp_ref  # noqa: E402

X0, Y0 = 392000.0, 5820000.0                                 # UTM-sized offsets: float32 could not hold these coordinates
TIE_SHARE = {"main": 0.01, "coarse": 0.50, "sparse": 0.01}


def cloud(seed, quantum):
    """~3 200 points on 70.3 x 45.7 m: a uniform scatter with a circular hole of radius ~10 m, a dense line of ~600 points,
    both corners occupied, 10 % exact duplicates of (x, y) with another z; coordinates are multiples of ``quantum``."""
    rng = np.random.default_rng(seed)
    W, H = 70.3, 45.7
    xy = rng.random((2600, 2)) * (W, H)
    xy = xy[np.hypot(xy[:, 0] - 42.0, xy[:, 1] - 24.0) > 10.0]
    t = rng.random(600)
    line = np.c_[8.0 + 25.0 * t, 6.0 + 9.0 * t] + rng.standard_normal((600, 2)) * 0.05
    xy = np.r_[xy, line, [[0.0, 0.0], [W, H]]]
    xy = np.round(xy / quantum) * quantum
    xy = np.clip(xy, 0.0, (np.round(W / quantum) * quantum, np.round(H / quantum) * quantum))
    z = 30.0 + 8.0 * np.sin(xy[:, 0] / 9.0) + 5.0 * np.cos(xy[:, 1] / 7.0) + rng.standard_normal(len(xy)) * 2.0
    dup = rng.choice(len(xy), len(xy) // 10, replace=False)
    xy = np.r_[xy, xy[dup]]
    z = np.r_[z, z[dup] + rng.standard_normal(len(dup)) * 6.0]
    order = rng.permutation(len(xy))
    return np.c_[X0 + xy[order, 0], Y0 + xy[order, 1], z[order]]


def sparse_cloud(seed):
    rng = np.random.default_rng(seed)
    xy = np.r_[rng.random((38, 2)) * (30.0, 20.0), [[0.0, 0.0], [30.0, 20.0]]]
    xy = np.round(xy / 0.01) * 0.01
    return np.c_[X0 + xy[:, 0], Y0 + xy[:, 1], 10.0 + rng.standard_normal(40) * 3.0]


class Captured:
    def __init__(self):
        self.points, self.raster, self.origin = None, None, None

    def install(self):
        laspy = types.ModuleType("laspy")
        laspy.read = lambda path: types.SimpleNamespace(x=self.points[:, 0].copy(), y=self.points[:, 1].copy(),
                                                        z=self.points[:, 2].copy())
        cap = self

        class Dst:
            def __enter__(self):
                return self

            def __exit__(self, *exc):
                return False

            def write(self, arr, band):
                cap.raster = np.array(arr)

        rio = types.ModuleType("rasterio")
        rio.open = lambda *a, **kw: Dst()
        rio.transform = types.ModuleType("rasterio.transform")

        def from_origin(west, north, xsize, ysize):
            cap.origin = np.array([west, north], np.float64)
            return (west, north, xsize, ysize)

        rio.transform.from_origin = from_origin
        sys.modules.update({"laspy": laspy, "rasterio": rio, "rasterio.transform": rio.transform})


def run(script, cap, points):
    cap.points, cap.raster, cap.origin = points, None, None
    cwd = os.getcwd()
    os.chdir("/tmp")
    try:
        glob = runpy.run_path(os.path.join(ref_import.REFERENCE_ROOT, "scripts", script))
    finally:
        os.chdir(cwd)
    assert cap.raster is not None and cap.raster.dtype == np.float64
    return glob, cap.raster, cap.origin


def main():
    assert ref_import.reference_available()
    cap = Captured()
    cap.install()
    cases = {"main": cloud(20241101, 0.01), "coarse": cloud(20241102, 0.25), "sparse": sparse_cloud(20241103)}
    out = {"cases": np.array(list(cases))}
    for name, pts in cases.items():
        g_near, near, o_near = run("interpolate_nearest.py", cap, pts)
        g_idw, idw, o_idw = run("interpolate_idw.py", cap, pts)
        ref_unique = g_near["max_z_df"][["X", "Y", "Z"]].values
        unique = interp_ref.unique_cloud(pts)
        assert unique.tobytes() == np.ascontiguousarray(ref_unique).tobytes(), "groupby order is X, then Y"
        assert np.array_equal(o_near, o_idw) and near.shape == idw.shape
        # the row of the input every group-by row came from
        key = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(pts))}
        keep = np.array([key[r.tobytes()] for r in unique], np.int32)
        dist, _ = g_near["tree"].query(np.c_[g_near["grid_x"].ravel(), g_near["grid_y"].ravel()], k=8)
        dist = dist.reshape(near.shape + (8,))
        ny, nx = near.shape
        print(f"{name}: N = {len(pts)}, M = {len(unique)}, raster {ny} x {nx}, origin {tuple(o_near)}")

        d2, idx, tie8 = interp_ref.knn(unique, 1.0, 8)
        assert d2.shape == dist.shape and np.array_equal(np.sqrt(d2), dist), "k-d tree distances are sqrt(dx*dx + dy*dy)"
        zero = int((d2[..., 0] == 0).sum())
        r_near, tie1 = interp_ref.nearest(unique)
        r_idw, _ = interp_ref.idw(unique)
        share1, share8 = tie1.mean(), tie8.mean()
        rank1 = (d2[..., 0] == d2[..., 1]).mean()
        assert share1 <= TIE_SHARE[name] and share8 <= TIE_SHARE[name], (name, share1, share8)
        assert near[~tie1].tobytes() == r_near[~tie1].tobytes()
        unit = 2.0 ** -53 * np.abs(unique[:, 2]).max()
        gap = np.abs(idw - r_idw)[~tie8].max() / unit
        assert gap <= 32.0, gap
        print(f"  zero-distance nodes {zero}; pixels left out: {100 * share1:.2f} % at k = 1, {100 * share8:.2f} % at k = 8 "
              f"(ranks 1 and 2 tie on {100 * rank1:.2f} %); IDW gap {gap:.2f} x 2^-53 max|z| (bound 32)")
        out.update({f"{name}_points": pts, f"{name}_keep": keep, f"{name}_nearest": near, f"{name}_idw": idw,
                    f"{name}_origin": o_near, f"{name}_dist": dist})
    path = os.path.join(HERE, "interp_baselines.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
