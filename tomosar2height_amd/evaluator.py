"""DSM evaluation on the device (reference: evaluator.py:14-99, utils/dilate_mask.py; kernels: csrc/dsm_eval.hip).

``DSMGenerator.generate_dsm()`` leaves a float64 mosaic in HBM; ``DSMEvaluator.eval`` takes that tensor as it is and returns
the reference's statistics table (``max, min, MAE, RMSE, abs_median, median, n_pixel, NMAD`` per class, all ``None`` for an
empty class) plus the residual plane, with exact medians and one small device-to-host copy at the end.  The reference reads
its rasters from GeoTIFF paths; here they are device tensors and the ground truth's georeference is given the way
``DSMGenerator`` takes its own: left / top bound and pixel size, i.e. ``Affine(px, 0, left, 0, -py, top)``.  The reference's
``print_statistics`` accepts the returned ``stats`` unchanged.

The entry points of include/t2h_eval.h are bound here: ``_lib.declare("t2h_eval.h", SIGNATURES)``.
"""
import ctypes
import math

import torch

from . import _lib

_vp, _i, _i64, _sz, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); mirrors include/t2h_eval.h one to one
SIGNATURES = {
    "t2h_eval_predicate": (_i, [_vp, _i, _i, _d, _vp, _i64, _vp]),
    "t2h_eval_dilate": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "t2h_eval_class_bits": (_i, [_vp, _i, _vp, _i, _vp, _i64, _vp]),
    "t2h_eval_residual": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "t2h_eval_stats_workspace_bytes": (_sz, [_i64, _i]),
    "t2h_eval_stats": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _sz, _vp]),
}

MAX_CLASSES = 16
TABLE_COLS = 8
NONZERO, EQ, GT = 0, 1, 2
_KIND = {torch.bool: 0, torch.uint8: 0, torch.int16: 1, torch.int32: 2, torch.int64: 3, torch.float32: 4, torch.float64: 5}
STAT_KEYS = ("max", "min", "MAE", "RMSE", "abs_median", "median", "n_pixel", "NMAD")
# device launches of one eval(): residual, histogram clear, sums + their reduction, 2 rounds x 8 x (digit pass + scan), the
# two median kernels
LAUNCHES_PER_EVAL = 1 + 1 + 2 + 2 * (8 * 2 + 1)

_lib.declare("t2h_eval.h", SIGNATURES)
load = _lib.load


def _plane(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor, got {type(t).__name__}")
    _lib.require_device(t, what=what)
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty [rows, cols] plane, got {tuple(t.shape)}")
    return t


def _predicate(t, op, value, what):
    """uint8 0 / 1 plane of ``pred(t)`` (t2h_eval_predicate)."""
    kind = _KIND.get(t.dtype)
    if kind is None:
        raise TypeError(f"{what}: unsupported dtype {t.dtype}")
    out = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
    _lib.call("t2h_eval_predicate", _lib.ptr(t), kind, op, float(value), _lib.ptr(out), t.numel(), _lib.stream(),
              nbytes=t.numel() * (t.element_size() + 1))
    return out


def _dilate(m8, iterations):
    if int(iterations) != iterations or iterations < 1:
        raise ValueError(f"dilate_mask: iterations = {iterations}; scipy's 'repeat until stable' (< 1) is not built")
    out = torch.empty_like(m8)
    _lib.call("t2h_eval_dilate", _lib.ptr(m8), _lib.ptr(out), m8.shape[0], m8.shape[1], int(iterations), _lib.stream(),
              nbytes=2 * m8.numel())
    return out


def dilate_mask(mask: torch.Tensor, iterations: int = 1) -> torch.Tensor:
    """utils/dilate_mask.py: ``scipy.ndimage.binary_dilation(mask, iterations=iterations)`` with scipy's defaults (cross
    structuring element, border value 0) on a device bool plane; returns a device bool plane."""
    _plane(mask, "dilate_mask")
    m8 = mask.view(torch.uint8) if mask.dtype == torch.bool else _predicate(mask, NONZERO, 0, "dilate_mask")
    return _dilate(m8, iterations).view(torch.bool)


class DSMEvaluator:
    def __init__(self, gt_dsm, bounds, pixel_size=(1.0, 1.0), gt_mask=None, other_masks=None):
        """``gt_dsm`` [R, C] float32 / float64, ``bounds`` = (left, top) of the ground-truth raster, ``pixel_size`` =
        (px, py); ``gt_mask`` bool / uint8 [R, C] (default: all true); ``other_masks``: dict of [R, C] planes with the
        reference's keys -- ``'building'`` (dilated twice, adds ``'terrain'``), ``'type'`` (values 0 / 1 / 2: adds
        ``non_building, residential, non_residential, building_combined``), any other key used as a bool mask."""
        self.gt_dsm = _plane(gt_dsm, "DSMEvaluator gt_dsm")
        if gt_dsm.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"DSMEvaluator: gt_dsm must be float32 or float64, got {gt_dsm.dtype}")
        self.left, self.top = float(bounds[0]), float(bounds[1])
        self.pixel_size = (float(pixel_size[0]), float(pixel_size[1]))
        shape = tuple(gt_dsm.shape)

        def plane(t, what):
            if tuple(_plane(t, what).shape) != shape:
                raise ValueError(f"{what}: shape {tuple(t.shape)} is not the ground truth's {shape}")
            return t

        other_masks = dict(other_masks) if other_masks else {}
        names = ["overall"]
        if "building" in other_masks:
            names += ["building", "terrain"]
        if "type" in other_masks:
            names += ["non_building", "residential", "non_residential", "building_combined"]
        for key in other_masks:
            if key not in ("building", "type") and key not in names:     # (a key that repeats a derived name replaces it)
                names.append(key)
        if len(names) > MAX_CLASSES:
            raise ValueError(f"DSMEvaluator: {len(names)} classes including 'overall'; one uint16 of class bits per pixel "
                             f"holds at most {MAX_CLASSES}")
        self.class_names = names
        self.has_binary_building = "building" in other_masks
        self.has_ternary_building = "type" in other_masks

        gm = None
        if gt_mask is not None:
            gm = plane(gt_mask, "DSMEvaluator gt_mask")
            gm = gm.view(torch.uint8) if gm.dtype in (torch.bool, torch.uint8) else _predicate(gm, NONZERO, 0, "gt_mask")
        self.class_bits = torch.empty(shape, dtype=torch.int16, device=gt_dsm.device)      # uint16 bit patterns
        n = gt_dsm.numel()

        def set_bit(name, m8, invert=0):
            _lib.call("t2h_eval_class_bits", _lib.ptr(m8) if m8 is not None else None, invert,
                      _lib.ptr(gm) if gm is not None else None, names.index(name), _lib.ptr(self.class_bits), n,
                      _lib.stream(), nbytes=n * 6)

        set_bit("overall", None)                                          # stores the word: first
        masks = {}
        if "building" in other_masks:                                     # evaluator.py:30-34
            b = plane(other_masks["building"], "other_masks['building']")
            masks["building"] = _dilate(b.view(torch.uint8) if b.dtype == torch.bool else _predicate(b, NONZERO, 0, "building"), 2)
        if "type" in other_masks:                                         # evaluator.py:36-47
            t = plane(other_masks["type"], "other_masks['type']")
            masks["non_building"] = _predicate(t, EQ, 0, "type")
            masks["residential"] = _dilate(_predicate(t, EQ, 1, "type"), 2)
            masks["non_residential"] = _dilate(_predicate(t, EQ, 2, "type"), 2)
            masks["building_combined"] = _dilate(_predicate(t, GT, 0, "type"), 2)
        for key, m in other_masks.items():                                # evaluator.py:49-51
            if key not in ("building", "type"):
                m = plane(m, f"other_masks[{key!r}]")
                masks[key] = m.view(torch.uint8) if m.dtype == torch.bool else _predicate(m, NONZERO, 0, key)
        for name in names[1:]:
            if name == "terrain" and "terrain" not in masks:
                set_bit(name, masks["building"], invert=1)
            else:
                set_bit(name, masks[name])

    def window(self, top_left):
        """``(l_col, t_row)`` of a raster whose top-left corner is the world point ``top_left`` (evaluator.py:55-56)."""
        x, y = top_left
        return (int(math.floor((x - self.left) / self.pixel_size[0])), int(math.floor((self.top - y) / self.pixel_size[1])))

    def eval(self, target_dsm, top_left=None):
        """``(stats, diff)``: ``stats[class][key]`` as in the reference, ``diff`` the float64 [H, W] device plane of
        ``target - gt`` inside ``gt_mask`` (NaN outside).  ``top_left`` = world (x, y) of the target's top-left corner
        (default: the ground truth's own)."""
        t = _plane(target_dsm, "DSMEvaluator.eval target_dsm")
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"DSMEvaluator.eval: target_dsm must be float32 or float64, got {t.dtype}")
        if t.device != self.gt_dsm.device:
            raise ValueError(f"DSMEvaluator.eval: target on {t.device}, ground truth on {self.gt_dsm.device}")
        l_col, t_row = self.window(top_left) if top_left is not None else (0, 0)
        H, W = t.shape
        R, C = self.gt_dsm.shape
        if t_row < 0 or l_col < 0 or t_row + H > R or l_col + W > C:
            # the reference's slices (evaluator.py:58-59) would wrap around or come out short here
            raise ValueError(f"target rows [{t_row}, {t_row + H}) x cols [{l_col}, {l_col + W}) is not inside the "
                             f"{(R, C)} ground truth")
        dev, n, ncls = t.device, H * W, len(self.class_names)
        diff = torch.empty((H, W), dtype=torch.float64, device=dev)
        cw = torch.empty((H, W), dtype=torch.int16, device=dev)
        table = torch.empty((ncls, TABLE_COLS), dtype=torch.float64, device=dev)
        st = _lib.stream()
        _lib.call("t2h_eval_residual", _lib.ptr(t), int(t.dtype == torch.float64), H, W, _lib.ptr(self.gt_dsm),
                  int(self.gt_dsm.dtype == torch.float64), _lib.ptr(self.class_bits), R, C, t_row, l_col, _lib.ptr(diff),
                  _lib.ptr(cw), st, nbytes=n * (t.element_size() + self.gt_dsm.element_size() + 2 + 8 + 2))
        need = _lib.ws_bytes("t2h_eval_stats_workspace_bytes", n, ncls)
        ws = _lib.workspace(need, dev)
        _lib.call("t2h_eval_stats", _lib.ptr(diff), _lib.ptr(cw), n, ncls, _lib.ptr(table), _lib.ptr(ws), need, st,
                  nbytes=17 * 10 * n)
        host = table.cpu()                                                # the one device-to-host copy (and wait) of the call
        counts = host.view(torch.int64)[:, 0].tolist()
        rows = host.tolist()
        stats = {}
        for name, cnt, row in zip(self.class_names, counts, rows):
            if cnt == 0:
                stats[name] = dict.fromkeys(STAT_KEYS)
                continue
            _, mn, mx, sum_abs, sum_sq, med, abs_med, mad = row
            stats[name] = {"max": mx, "min": mn, "MAE": sum_abs / cnt, "RMSE": math.sqrt(sum_sq / cnt), "abs_median": abs_med,
                           "median": med, "n_pixel": int(cnt), "NMAD": 1.4826 * mad}
        return stats, diff
