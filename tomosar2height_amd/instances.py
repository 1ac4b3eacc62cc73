"""Building-wise DSM metrics on the device (reference: scripts/evaluator_instance.py:15-57; kernels: csrc/dsm_instances.hip).

``label_components`` is ``skimage.measure.label(mask, connectivity=2)`` for a binary mask (skimage separates regions of
different nonzero values; a footprint mask has one, so here every nonzero pixel is foreground).  ``BuildingEvaluator.eval``
takes the tensor ``DSMGenerator.generate_dsm()`` returns and gives the reference's RMSE-B / MAE-B / MedAE-B: the median height
of every building in the prediction and in the ground truth, then the error over the buildings.  The point-cloud variants of
the same script (evaluator_instance.py:139-291) are ``cloud_instances.py``; ``segment_medians`` takes any plane of values with a
plane of labels, and gives them their DTM and nDSM medians.

The entry points of include/t2h_inst.h are bound here: ``_lib.declare("t2h_inst.h", SIGNATURES)``.
"""
import ctypes
import math

import torch

from . import _lib
from .evaluator import NONZERO, _plane, _predicate

_vp, _i, _i64, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t

# name -> (restype, argtypes); mirrors include/t2h_inst.h one to one
SIGNATURES = {
    "t2h_inst_label_workspace_bytes": (_sz, [_i, _i]),
    "t2h_inst_label": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "t2h_inst_medians_workspace_bytes": (_sz, [_i64, _i]),
    "t2h_inst_medians": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "t2h_inst_metrics": (_i, [_vp, _vp, _i, _vp, _vp]),
}

TILE = 32               # T2H_INST_TILE
TINY_MAX = 64           # T2H_INST_TINY_MAX: one wave per segment up to here
SMALL_MAX = 2048        # T2H_INST_SMALL_MAX: one workgroup per segment up to here, radix select above
TABLE_COLS = 8
# device launches: tile pass, border merge, flatten, scan, rank, relabel
LAUNCHES_PER_LABEL = 6
# two clears, counts, three for the offsets, compaction, the two on-chip classes, 4 x (digit pass + scan) where a segment can
# be large
LAUNCHES_PER_MEDIANS = 2 + 1 + 3 + 1 + 2 + 4 * 2
LAUNCHES_PER_EVAL = LAUNCHES_PER_MEDIANS + 1

_lib.declare("t2h_inst.h", SIGNATURES)
load = _lib.load


def _mask8(mask, what):
    _plane(mask, what)
    return mask.view(torch.uint8) if mask.dtype in (torch.bool, torch.uint8) else _predicate(mask, NONZERO, 0, what)


def _label(m8, t_row, l_col, R, C, connectivity):
    """Labels of the [R, C] window at (t_row, l_col) of a contiguous uint8 plane, and the device int32 that holds K."""
    if connectivity not in (1, 2):
        raise ValueError(f"label_components: connectivity = {connectivity!r}; 1 (4 neighbours) or 2 (8 neighbours)")
    ld = m8.shape[1]
    labels = torch.empty((R, C), dtype=torch.int32, device=m8.device)
    k_dev = torch.empty(1, dtype=torch.int32, device=m8.device)
    need = _lib.ws_bytes("t2h_inst_label_workspace_bytes", R, C)
    if need == 0:
        raise ValueError(f"label_components: a {R} x {C} plane has more than 2^31 - 1 pixels")
    ws = _lib.workspace(need, m8.device)
    _lib.call("t2h_inst_label", _lib.ptr(m8) + t_row * ld + l_col, ld, R, C, int(connectivity), _lib.ptr(labels), _lib.ptr(k_dev),
              _lib.ptr(ws), need, _lib.stream(), nbytes=R * C * (1 + 6 * 4))
    return labels, k_dev


def label_components(mask: torch.Tensor, connectivity: int = 2):
    """``(labels, K)``: int32 [R, C] device plane with 0 for background and 1..K in raster order of each component's first
    pixel (skimage's and scipy's numbering), and K as a Python int (one 4-byte copy).  ``mask``: any dtype ``DSMEvaluator``
    takes for a mask; nonzero is foreground."""
    m8 = _mask8(mask, "label_components")
    labels, k_dev = _label(m8, 0, 0, m8.shape[0], m8.shape[1], connectivity)
    return labels, int(k_dev.item())


def segment_medians(values: torch.Tensor, labels: torch.Tensor, K: int, window=None):
    """``(counts int32 [K], medians float32 [K])`` on the device: ``np.median(values32[labels == k])`` for k = 1..K, where
    ``values32`` is ``values`` (float32, or float64 rounded to float32), or its window ``(t_row, l_col)`` of the labels' shape."""
    _plane(values, "segment_medians values")
    _plane(labels, "segment_medians labels")
    if values.dtype not in (torch.float32, torch.float64) or labels.dtype != torch.int32:
        raise TypeError(f"segment_medians: values float32 / float64 and labels int32, got {values.dtype} and {labels.dtype}")
    H, W = labels.shape
    t_row, l_col = window if window is not None else (0, 0)
    if t_row < 0 or l_col < 0 or t_row + H > values.shape[0] or l_col + W > values.shape[1]:
        raise ValueError(f"segment_medians: rows [{t_row}, {t_row + H}) x cols [{l_col}, {l_col + W}) is not inside the "
                         f"{tuple(values.shape)} plane of values")
    dev = values.device
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    medians = torch.empty(K, dtype=torch.float32, device=dev)
    if K == 0:
        return counts, medians
    n, ld = H * W, values.shape[1]
    need = _lib.ws_bytes("t2h_inst_medians_workspace_bytes", n, K)
    if need == 0:
        raise ValueError(f"segment_medians: {K} labels for {n} pixels (0 <= K <= pixels < 2^31)")
    ws = _lib.workspace(need, dev)
    _lib.call("t2h_inst_medians", _lib.ptr(values) + (t_row * ld + l_col) * values.element_size(),
              int(values.dtype == torch.float64), ld, H, W, _lib.ptr(labels), K, _lib.ptr(counts), _lib.ptr(medians),
              _lib.ptr(ws), need, _lib.stream(), nbytes=n * (2 * 4 + values.element_size() + 5 * 8) + 20 * K)
    return counts, medians


class BuildingEvaluator:
    def __init__(self, building_mask, gt_dsm, bounds, pixel_size=(1.0, 1.0), connectivity=2):
        """``building_mask`` [R, C] (nonzero = footprint), ``gt_dsm`` [R, C] float32 / float64, ``bounds`` = (left, top) of
        both rasters, ``pixel_size`` = (px, py): the georeference as ``DSMEvaluator`` takes it."""
        self.gt_dsm = _plane(gt_dsm, "BuildingEvaluator gt_dsm")
        if gt_dsm.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"BuildingEvaluator: gt_dsm must be float32 or float64, got {gt_dsm.dtype}")
        if tuple(_plane(building_mask, "BuildingEvaluator building_mask").shape) != tuple(gt_dsm.shape):
            raise ValueError(f"building_mask: shape {tuple(building_mask.shape)} is not the ground truth's {tuple(gt_dsm.shape)}")
        if building_mask.device != gt_dsm.device:
            raise ValueError(f"BuildingEvaluator: mask on {building_mask.device}, ground truth on {gt_dsm.device}")
        self.mask8 = _mask8(building_mask, "BuildingEvaluator building_mask")
        self.left, self.top = float(bounds[0]), float(bounds[1])
        self.pixel_size = (float(pixel_size[0]), float(pixel_size[1]))
        self.connectivity = connectivity
        self._windows = {}              # (t_row, l_col, H, W) -> (labels, K, counts, gt medians)

    def window(self, top_left):
        """``(l_col, t_row)`` of a raster whose top-left corner is the world point ``top_left`` (as ``DSMEvaluator.window``)."""
        x, y = top_left
        return (int(math.floor((x - self.left) / self.pixel_size[0])), int(math.floor((self.top - y) / self.pixel_size[1])))

    def buildings(self, t_row, l_col, H, W):
        """Labels, K, pixel counts and ground-truth medians of the mask cropped to a window: computed on first use (with the
        one 4-byte copy that reads K), then kept."""
        key = (t_row, l_col, H, W)
        hit = self._windows.get(key)
        if hit is None:
            labels, k_dev = _label(self.mask8, t_row, l_col, H, W, self.connectivity)
            K = int(k_dev.item())
            counts, gt_med = segment_medians(self.gt_dsm, labels, K, window=(t_row, l_col))
            hit = self._windows[key] = (labels, K, counts, gt_med)
        return hit

    def eval(self, target_dsm, top_left=None):
        """``(metrics, record)``: ``metrics`` = {"RMSE-B", "MAE-B", "MedAE-B", "max_abs", "n_buildings", "n_valid", "n_nan"}
        (the first four ``None`` when no building has two finite medians), ``record`` = {"labels", "counts", "pred_median",
        "gt_median"} on the device.  ``top_left`` = world (x, y) of the target's top-left corner (default: the ground
        truth's own); with a target smaller than the ground truth the result is the reference's on the three rasters cropped
        to that window."""
        t = _plane(target_dsm, "BuildingEvaluator.eval target_dsm")
        if t.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"BuildingEvaluator.eval: target_dsm must be float32 or float64, got {t.dtype}")
        if t.device != self.gt_dsm.device:
            raise ValueError(f"BuildingEvaluator.eval: target on {t.device}, ground truth on {self.gt_dsm.device}")
        l_col, t_row = self.window(top_left) if top_left is not None else (0, 0)
        H, W = t.shape
        R, C = self.gt_dsm.shape
        if t_row < 0 or l_col < 0 or t_row + H > R or l_col + W > C:
            raise ValueError(f"target rows [{t_row}, {t_row + H}) x cols [{l_col}, {l_col + W}) is not inside the "
                             f"{(R, C)} ground truth")
        labels, K, counts, gt_med = self.buildings(t_row, l_col, H, W)
        _, pred_med = segment_medians(t, labels, K)
        record = {"labels": labels, "counts": counts, "pred_median": pred_med, "gt_median": gt_med}
        metrics = {"RMSE-B": None, "MAE-B": None, "MedAE-B": None, "max_abs": None, "n_buildings": K, "n_valid": 0, "n_nan": 0}
        if K == 0:
            return metrics, record
        table = torch.empty(TABLE_COLS, dtype=torch.float64, device=t.device)
        _lib.call("t2h_inst_metrics", _lib.ptr(pred_med), _lib.ptr(gt_med), K, _lib.ptr(table), _lib.stream(), nbytes=8 * K * 17)
        n_valid, n_nan, sum_abs, sum_sq, med_abs, max_abs = table.cpu().tolist()[:6]   # the one copy (and wait) of the call
        metrics["n_valid"], metrics["n_nan"] = int(n_valid), int(n_nan)
        if n_valid > 0:
            metrics.update({"RMSE-B": math.sqrt(sum_sq / n_valid), "MAE-B": sum_abs / n_valid, "MedAE-B": med_abs,
                            "max_abs": max_abs})
        return metrics, record
