"""Writes tests/golden/cloud_instances.npz from the reference's own scripts/evaluator_instance.py (build container only).

    python tests/golden/make_golden_cloud_instances.py

The script is imported where it lies, as in make_golden_instances.py: the same stand-in ``skimage.measure.label`` (scipy's
labelling with a full 3 x 3 structure), ``read_tif`` and ``read_npz`` replaced by look-ups into in-memory arrays, and the
stubbed ``rasterio.open`` a context manager whose object carries ``.transform``.

``.transform`` is a STAND-IN for ``affine.Affine`` (not installed): ``Transform`` below keeps the six coefficients, inverts
with the expressions of ``affine.Affine.__invert__`` and multiplies a pair as ``(vx*sa + vy*sb + sc, vx*sd + vy*se + sf)``,
which is what ``Affine.__mul__`` computes on a pair of arrays.

The reference's own ``evaluate_cloud_valid_only()`` and ``evaluate_cloud_all()`` run; they only print, so their three numbers
are recorded by wrapping ``ref.rmse``, ``ref.mean_absolute_error`` and ``ref.median_absolute_error``.  The per-building point
heights come from a direct call of ``associate_points_with_buildings``.  The reference crops ``dtm[:-1]`` and ``mask[1:-1]``
while taking the transform from the uncropped file: it is fed rasters of R + 1 and R + 2 rows, and the fixture stores the
cropped planes with that transform.  Only inputs and the reference's outputs are stored.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402


class Transform:
    """Stand-in for affine.Affine: x = a col + b row + c, y = d col + e row + f."""

    def __init__(self, a, b, c, d, e, f):
        self.coeffs = tuple(float(v) for v in (a, b, c, d, e, f))

    def __invert__(self):
        sa, sb, sc, sd, se, sf = self.coeffs
        idet = 1.0 / (sa * se - sb * sd)
        ra = se * idet
        rb = -sb * idet
        rd = -sd * idet
        re = sa * idet
        return Transform(ra, rb, -sc * ra - sf * rb, rd, re, -sc * rd - sf * re)

    def __mul__(self, other):
        sa, sb, sc, sd, se, sf = self.coeffs
        vx, vy = other
        return (vx * sa + vy * sb + sc, vx * sd + vy * se + sf)


def make_case(rng, R, C, transform, n_points):
    """Planes of R (+ 1, + 2) rows and a cloud in world coordinates quantised to 1 mm."""
    from make_golden_instances import sk_label
    mask_full = np.zeros((R + 2, C), np.uint8)
    for _ in range(46):
        y, x, h, w = rng.integers(1, R - 3), rng.integers(0, C - 4), rng.integers(2, 14), rng.integers(2, 14)
        mask_full[y:y + h, x:x + w] = 1
    mask_full[rng.random((R + 2, C)) < 0.006] = 1                # salt: buildings of one pixel, most of them without a point
    mask_full[0] = mask_full[-1] = 0
    mask = mask_full[1:-1]
    dtm_full = (30 + 0.02 * np.arange(C)[None, :] + rng.standard_normal((R + 1, C)) * 0.3).astype(np.float32)
    ndsm = (np.abs(rng.standard_normal((R, C))) * 2 + 11 * mask).astype(np.float32)
    labels = sk_label(mask)
    K = int(labels.max())
    # pixel coordinates: most points on the raster, a share of them on buildings, some outside on all four sides
    col = rng.random(n_points) * C
    row = rng.random(n_points) * R
    by, bx = np.nonzero(mask)
    on = rng.random(n_points) < 0.45
    pick = rng.integers(0, by.size, n_points)
    col[on], row[on] = bx[pick[on]] + rng.random(on.sum()), by[pick[on]] + rng.random(on.sum())
    out = rng.random(n_points) < 0.04
    side = rng.integers(0, 4, n_points)
    col[out & (side == 0)] = -rng.random((out & (side == 0)).sum()) * 9
    col[out & (side == 1)] = C + rng.random((out & (side == 1)).sum()) * 9
    row[out & (side == 2)] = -rng.random((out & (side == 2)).sum()) * 9
    row[out & (side == 3)] = R + rng.random((out & (side == 3)).sum()) * 9
    edge = rng.random(n_points) < 0.02                             # exactly on pixel edges (before the quantisation)
    col[edge], row[edge] = np.floor(col[edge]), np.floor(row[edge])
    x, y = transform * (col, row)
    li = labels[np.clip(np.floor(row).astype(int), 0, R - 1), np.clip(np.floor(col).astype(int), 0, C - 1)]
    z = 30 + 0.02 * col + np.where(li > 0, 11.0, 0.0) + rng.standard_normal(n_points) * 1.5
    pts = np.round(np.stack([x, y, z], 1) * 1000.0) / 1000.0     # 1 mm, as LAS stores it
    return mask_full, mask, dtm_full, ndsm, pts, K


def thin_one_building(pts, mask, transform):
    """Removes all but one point of the first building that holds at least three: the fixture has a one-point segment."""
    from make_golden_instances import sk_label
    labels = sk_label(mask)
    R, C = mask.shape
    fx, fy = (~transform) * (pts[:, 0], pts[:, 1])
    li = labels[np.clip(np.floor(fy).astype(int), 0, R - 1), np.clip(np.floor(fx).astype(int), 0, C - 1)]
    sizes = np.bincount(li, minlength=labels.max() + 1)
    k = int(np.nonzero(sizes[1:] >= 3)[0][0]) + 1
    drop = np.nonzero(li == k)[0][1:]
    return np.delete(pts, drop, axis=0), k


def main():
    from make_golden_instances import sk_label               # (scipy: only the generator needs it, not the stand-in class)
    ref_import.import_reference()
    sk = types.ModuleType("skimage")
    sk.measure = types.ModuleType("skimage.measure")
    sk.measure.label = sk_label
    sys.modules["skimage"], sys.modules["skimage.measure"] = sk, sk.measure
    spec = importlib.util.spec_from_file_location(
        "evaluator_instance", os.path.join(ref_import.REFERENCE_ROOT, "scripts", "evaluator_instance.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    files, state, recorded = {}, {}, {}

    def lookup(path):
        return files[os.path.basename(path)]

    class Source:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        transform = property(lambda self: state["transform"])

    ref.read_tif = lookup
    ref.read_npz = lookup
    ref.rasterio.open = lambda path: Source()

    def record(name, fn):
        def wrapped(y_true, y_pred):
            recorded["dtypes"] = (np.asarray(y_true).dtype, np.asarray(y_pred).dtype)
            recorded[name] = out = fn(y_true, y_pred)
            return out
        return wrapped

    ref.rmse = record("RMSE-B", ref.rmse)
    ref.mean_absolute_error = record("MAE-B", ref.mean_absolute_error)
    ref.median_absolute_error = record("MedAE-B", ref.median_absolute_error)

    import cloud_inst_ref                                    # tests/cloud_inst_ref.py: the gap printed below
    rng = np.random.default_rng(20241019)
    R, C = 96, 160
    cases = {
        "north_up": Transform(1.0, 0.0, 392000.0, 0.0, -1.0, 5820000.0 + R),
        "rotated": Transform(0.5, 0.03125 + 1e-3, 392000.25, 0.0205, -0.5, 5820000.5 + R / 2),
    }
    out = {"cases": np.array(list(cases))}
    for name, transform in cases.items():
        mask_full, mask, dtm_full, ndsm, pts, K = make_case(rng, R, C, transform, 12000)
        pts, single = thin_one_building(pts, mask, transform)
        files.update({"input_point_cloud.npz": pts, "munich_chunk5_dem.tif": dtm_full, "munich_chunk5_mask.tif": mask_full,
                      "ndsm_chunk5.tif": ndsm})
        state["transform"] = transform
        labels = sk_label(mask).astype(np.int32)
        heights = ref.associate_points_with_buildings(pts, mask, labels, transform)
        assert list(heights) == list(range(1, K + 1))
        counts = np.array([heights[k].size for k in range(1, K + 1)], np.int32)
        pred_median = np.array([np.median(heights[k]) if heights[k].size else np.nan for k in range(1, K + 1)], np.float64)
        dtm_median = ref.compute_median_height_per_building(dtm_full[:-1], mask, labels)
        ndsm_median = ref.compute_median_height_per_building(ndsm, mask, labels)
        assert dtm_median.dtype == np.float32 and ndsm_median.dtype == np.float32 and not np.isnan(ndsm_median).any()
        # the per-point label, from the reference's own index expressions (lines 156-158)
        rx, ry = (~transform) * (pts[:, 0], pts[:, 1])
        rx = np.clip(np.floor(rx).astype(int), 0, C - 1)
        ry = np.clip(np.floor(ry).astype(int), 0, R - 1)
        point_label = labels[ry, rx].astype(np.int32)
        for k in range(1, K + 1):                            # same multiset per building as the function's own lists
            assert np.array_equal(np.sort(heights[k]), np.sort(pts[point_label == k, 2]))
        fx, fy = (np.floor(v) for v in (~transform) * (pts[:, 0], pts[:, 1]))
        outside = [int((fx < 0).sum()), int((fx >= C).sum()), int((fy < 0).sum()), int((fy >= R).sum())]
        assert min(outside) > 10, outside
        assert (counts == 0).sum() >= 3 and counts[single - 1] == 1
        three = {}
        for mode, fn in (("valid_only", ref.evaluate_cloud_valid_only), ("all", ref.evaluate_cloud_all)):
            recorded.clear()
            stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
            try:
                fn()
            finally:
                sys.stdout.close()
                sys.stdout = stdout
            three[mode] = np.array([float(recorded[k]) for k in ("RMSE-B", "MAE-B", "MedAE-B")])
            dtypes = recorded["dtypes"]
        print(f"{name}: {K} components, {pts.shape[0]} points, {int(counts.sum())} on buildings, segment sizes {counts.min()} .. "
              f"{counts.max()}, {int((counts == 0).sum())} without a point, building {single} has one; points outside "
              f"(left, right, top, bottom) {outside}; sklearn sees y_true {dtypes[0]}, y_pred {dtypes[1]}")
        transform6 = np.array(transform.coeffs)
        for mode in ("valid_only", "all"):
            got, rec = cloud_inst_ref.evaluate(pts, mask, dtm_full[:-1], ndsm, transform6, mode)
            assert rec["point_label"].tobytes() == point_label.tobytes() and rec["counts"].tobytes() == counts.tobytes()
            assert cloud_inst_ref.same_floats(rec["pred_median"], pred_median)
            gap = max(abs(got[k] - v) / v for k, v in zip(("RMSE-B", "MAE-B", "MedAE-B"), three[mode]))
            print(f"  {mode}: reference RMSE-B / MAE-B / MedAE-B", *(f"{v:.12f}" for v in three[mode]),
                  f"; restatement vs reference: largest relative gap {gap:.3e} (bound 4 K 2^-53 = {4 * K * 2.0 ** -53:.3e})")
        out.update({f"{name}_transform": transform6, f"{name}_points": pts, f"{name}_mask": mask,
                    f"{name}_dtm": np.ascontiguousarray(dtm_full[:-1]), f"{name}_ndsm": ndsm, f"{name}_labels": labels,
                    f"{name}_point_label": point_label, f"{name}_counts": counts, f"{name}_pred_median": pred_median,
                    f"{name}_dtm_median": dtm_median, f"{name}_ndsm_median": ndsm_median,
                    f"{name}_height": pred_median - dtm_median, f"{name}_three_valid_only": three["valid_only"],
                    f"{name}_three_all": three["all"], f"{name}_inverse": np.array((~transform).coeffs)})
    path = os.path.join(HERE, "cloud_instances.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
