"""Writes tests/golden/dsm_evaluator.npz from the reference's own DSMEvaluator.eval and dilate_mask (build container only).

    python tests/golden/make_golden_evaluator.py

The reference's constructor reads GeoTIFFs through rasterio, which is not installed: the instance is made with
``object.__new__`` and its attributes are set from in-memory arrays, with a translation-and-scale stand-in for the two affine
objects ``eval`` multiplies with.  Only inputs and the reference's outputs are stored.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

STAT_KEYS = ("max", "min", "MAE", "RMSE", "abs_median", "median", "n_pixel", "NMAD")


class ScaleShift:
    """``Affine(a, 0, c, 0, e, f) * (x, y)`` for the axis-aligned case: (a x + c, e y + f)."""

    def __init__(self, a, c, e, f):
        self.a, self.c, self.e, self.f = a, c, e, f

    def __mul__(self, xy):
        return np.array([self.a * xy[0] + self.c, self.e * xy[1] + self.f])

    def inverse(self):
        return ScaleShift(1.0 / self.a, -self.c / self.a, 1.0 / self.e, -self.f / self.e)


class Reader:
    pass


def main():
    ref_import.import_reference()
    warnings.simplefilter("ignore", DeprecationWarning)
    import evaluator as ref_evaluator                      # the reference's evaluator.py
    from utils.dilate_mask import dilate_mask as ref_dilate

    rng = np.random.default_rng(20240607)
    R, C, H, W, t_row, l_col = 90, 150, 67, 131, 5, 7
    left, top, px, py = 1000.0, 2000.0, 0.5, 0.5
    gt = (rng.standard_normal((R, C)) * 8 + 30).astype(np.float32)
    gt[40, 60] = np.nan
    target = gt[t_row:t_row + H, l_col:l_col + W].astype(np.float64) + rng.standard_normal((H, W)) * 1.5
    target[40 - t_row, 60 - l_col] = 31.0                  # a finite target over the ground truth's NaN
    for y, x in ((0, 0), (3, 130), (66, 5), (30, 30), (50, 100)):
        target[y, x] = np.nan
    gt_mask = rng.random((R, C)) < 0.9
    building = (rng.random((R, C)) < 0.02).astype(np.uint8)
    type_plane = rng.choice(np.array([0, 1, 2], np.uint8), size=(R, C), p=(0.9, 0.06, 0.04))
    custom = rng.random((R, C)) < 0.3
    empty = np.zeros((R, C), bool)

    ev = object.__new__(ref_evaluator.DSMEvaluator)
    ev.gt_dsm, ev.gt_mask = gt, gt_mask
    ev._gt_dsm_reader = Reader()
    ev._gt_dsm_reader.T_inv = ScaleShift(px, left, -py, top).inverse()
    ev.other_mask = {}                                     # evaluator.py:30-51 on arrays instead of paths
    ev.other_mask["building"] = ref_dilate(building.astype(bool), iterations=2)
    ev.other_mask["terrain"] = ~ev.other_mask["building"]
    ev.other_mask["non_building"] = type_plane == 0
    ev.other_mask["residential"] = ref_dilate(type_plane == 1, iterations=2)
    ev.other_mask["non_residential"] = ref_dilate(type_plane == 2, iterations=2)
    ev.other_mask["building_combined"] = ref_dilate(type_plane > 0, iterations=2)
    ev.other_mask["water"] = custom.astype(bool)
    ev.other_mask["nothing"] = empty.astype(bool)
    top_left = (left + l_col * px + 0.1, top - t_row * py - 0.1)
    stats, diff = ev.eval(target, ScaleShift(px, top_left[0], -py, top_left[1]))

    names = list(stats)
    table = np.full((len(names), len(STAT_KEYS)), np.nan)
    is_none = np.zeros(table.shape, bool)
    for i, name in enumerate(names):
        for j, key in enumerate(STAT_KEYS):
            v = stats[name][key]
            is_none[i, j] = v is None
            if v is not None:
                table[i, j] = float(v)
    corners = np.zeros((H, W), bool)                       # set pixels in all four corners and on every edge
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 40), (H - 1, 77), (20, 0), (45, W - 1), (33, 64), (34, 66)):
        corners[y, x] = True
    line = np.zeros((1, 64), bool)
    line[0, [0, 9, 10, 40, 63]] = True
    out = dict(gt=gt, target=target, gt_mask=gt_mask, building=building, type=type_plane, water=custom, nothing=empty,
               geo=np.array([left, top, px, py]), top_left=np.array(top_left), window=np.array([t_row, l_col]),
               names=np.array(names), stat_keys=np.array(STAT_KEYS), table=table, is_none=is_none, diff=diff,
               corners=corners, line=line)
    for k in (1, 2, 3):
        out[f"building_dilated{k}"] = ref_dilate(building.astype(bool), iterations=k)
        out[f"corners_dilated{k}"] = ref_dilate(corners, iterations=k)
        out[f"line_dilated{k}"] = ref_dilate(line, iterations=k)
    path = os.path.join(HERE, "dsm_evaluator.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", names)


if __name__ == "__main__":
    main()
