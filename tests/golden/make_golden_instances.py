"""Writes tests/golden/building_instances.npz from the reference's own scripts/evaluator_instance.py (build container only).

    python tests/golden/make_golden_instances.py

The script is imported where it lies and its ``read_tif`` is replaced by a look-up into in-memory arrays (rasterio is a stub).
skimage is not installed: before the import a stand-in ``skimage.measure.label(img, connectivity=2)`` is installed, defined as
``scipy.ndimage.label(img != 0, structure=np.ones((3, 3)))[0]`` -- for a binary mask the same partition by definition, with
the same raster-order numbering, and the three metrics do not depend on the numbering anyway.  The metric functions are
sklearn's, as in the reference.  Only inputs and the reference's outputs are stored.
"""
import importlib.util
import os
import sys
import types

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import  # noqa: E402

STRUCT = {1: ndimage.generate_binary_structure(2, 1), 2: np.ones((3, 3), bool)}


def sk_label(img, connectivity=2):
    return ndimage.label(np.asarray(img) != 0, structure=STRUCT[connectivity])[0]


def structural_masks():
    """Planes of 70 x 101 pixels = 3 x 4 tiles of 32 x 32 with ragged last tiles, one mechanism of the tile merge each."""
    R, C = 70, 101
    out = {}
    m = np.zeros((R, C), np.uint8)
    m[31, 31] = m[32, 32] = 1                                # touch only diagonally across a four-tile corner
    m[31, 64] = m[32, 63] = 1                                # ... and on the other diagonal
    out["corner_diagonals"] = m
    m = np.zeros((R, C), np.uint8)
    m[31, 3:98] = 1                                          # a tile's last row
    m[64, 3:98] = 1                                          # a tile's first row
    out["seam_lines"] = m
    m = np.zeros((R, C), np.uint8)
    m[5:51, 10] = m[5:51, 80] = 1                            # arms in tile columns 0 and 2, joined in tile row 1
    m[50, 10:81] = 1
    out["u_shape"] = m
    m = np.zeros((R, C), np.uint8)
    m[0::2, :] = 1
    for r in range(1, R - 1, 2):
        m[r, C - 1 if (r // 2) % 2 == 0 else 0] = 1
    out["serpentine"] = m
    m = np.zeros((R, C), np.uint8)                           # a spiral, one pixel wide, one pixel apart: walk ahead while the
    y, x, dy, dx = 0, 0, 0, 1                                # cell after the next is free, else turn right
    m[0, 0] = 1
    inside = lambda yy, xx: 0 <= yy < R and 0 <= xx < C
    moved = True
    while moved:
        moved = False
        for _ in range(2):
            if inside(y + dy, x + dx) and not m[y + dy, x + dx] and not (inside(y + 2 * dy, x + 2 * dx) and m[y + 2 * dy, x + 2 * dx]):
                y, x, moved = y + dy, x + dx, True
                m[y, x] = 1
                break
            dy, dx = dx, -dy
    out["spiral"] = m
    out["full"] = np.ones((R, C), np.uint8)
    out["empty"] = np.zeros((R, C), np.uint8)
    for name, (h, w) in {"checker_8x8": (8, 8), "checker_67x131": (67, 131)}.items():
        yy, xx = np.mgrid[:h, :w]
        out[name] = ((yy + xx) % 2 == 0).astype(np.uint8)
    rng = np.random.default_rng(5)
    out["one_pixel"] = np.ones((1, 1), np.uint8)
    out["row_1x200"] = (rng.random((1, 200)) < 0.6).astype(np.uint8)
    out["col_200x1"] = (rng.random((200, 1)) < 0.6).astype(np.uint8)
    return out


def main():
    ref_import.import_reference()
    sk = types.ModuleType("skimage")
    sk.measure = types.ModuleType("skimage.measure")
    sk.measure.label = sk_label
    sys.modules["skimage"], sys.modules["skimage.measure"] = sk, sk.measure
    spec = importlib.util.spec_from_file_location(
        "evaluator_instance", os.path.join(ref_import.REFERENCE_ROOT, "scripts", "evaluator_instance.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rasters = {}
    ref.read_tif = rasters.__getitem__

    def reference(pred, gt, mask):
        rasters.update(pred=pred, gt=gt, mask=mask)
        three = np.array([float(v) for v in ref.evaluate_buildingwise_errors("pred", "gt", "mask")])
        labels = sk_label(mask, connectivity=2)
        pm = ref.compute_median_height_per_building(pred, mask, labels)
        gm = ref.compute_median_height_per_building(gt, mask, labels)
        return three, labels.astype(np.int32), pm, gm

    rng = np.random.default_rng(20241018)
    R, C = 96, 160
    mask = np.zeros((R, C), np.uint8)
    for _ in range(40):
        y, x, h, w = rng.integers(0, R - 4), rng.integers(0, C - 4), rng.integers(2, 16), rng.integers(2, 16)
        mask[y:y + h, x:x + w] = 1
    mask[rng.random((R, C)) < 0.01] = 1
    gt = (rng.standard_normal((R, C)) * 2 + 12 * mask + 3).astype(np.float32)
    pred = (gt + rng.standard_normal((R, C)) * 1.5 + 0.4).astype(np.float32)
    three, labels, pm, gm = reference(pred, gt, mask)
    sizes = np.bincount(labels.ravel())[1:]
    print(f"{labels.max()} components, sizes {sizes.min()} .. {sizes.max()}, {int((sizes % 2 == 0).sum())} of even size")
    print("reference RMSE-B / MAE-B / MedAE-B:", *(f"{v:.8f}" for v in three))
    out = dict(mask=mask, gt=gt, pred=pred, three=three, labels=labels, pred_median=pm, gt_median=gm)

    import inst_ref                                          # tests/inst_ref.py: the measured gap the GPU test's docstring records
    m64 = inst_ref.metrics(pm, gm)
    gap = max(abs(m64[k] - v) for k, v in zip(("RMSE-B", "MAE-B", "MedAE-B"), three))
    bound = 2.0 ** -20 * max(np.abs(pm).max(), np.abs(gm).max())
    print(f"float32 (sklearn) vs float64 aggregates: gap {gap:.3e}, bound 2^-20 max|median| = {bound:.3e}")

    # float64 prediction: the reference sees it as the GeoTIFF round trip leaves it, in float32
    pred64 = pred.astype(np.float64) + rng.standard_normal((R, C)) * 1e-6
    three64, _, pm64, _ = reference(pred64.astype(np.float32), gt, mask)
    out.update(pred64=pred64, three64=three64, pred64_median=pm64)

    # a window: the reference on the three rasters cropped to it
    t_row, l_col, H, W = 11, 23, 70, 101
    win = (slice(t_row, t_row + H), slice(l_col, l_col + W))
    three_w, labels_w, pm_w, gm_w = reference(np.ascontiguousarray(pred[win]), np.ascontiguousarray(gt[win]),
                                              np.ascontiguousarray(mask[win]))
    out.update(window=np.array([t_row, l_col, H, W]), three_window=three_w, labels_window=labels_w, pred_median_window=pm_w,
               gt_median_window=gm_w)

    names = []
    for name, m in structural_masks().items():
        names.append(name)
        out[f"s_{name}"] = m
        for conn in (1, 2):
            out[f"s_{name}_labels{conn}"] = sk_label(m, conn).astype(np.int32)
    out["structural"] = np.array(names)
    path = os.path.join(HERE, "building_instances.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
