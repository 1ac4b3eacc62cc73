"""Building-wise metrics of the raw point cloud on the device (reference: scripts/evaluator_instance.py:139-291; kernels:
csrc/dsm_cloud.hip).

The reference's ``evaluate_cloud_all`` / ``evaluate_cloud_valid_only`` score the TomoSAR point cloud itself, building by
building: every point goes through the inverse raster transform to a pixel and takes that pixel's building label; the median z
of a building's points minus the building's median DTM height is compared with its median nDSM height.  A building without
points has a NaN height: ``"valid_only"`` drops it, ``"all"`` counts it as height 0 (``np.nan_to_num``).

``assign_points`` is ``associate_points_with_buildings`` (lines 155-164), ``point_medians`` the ``np.median`` of float64 z values
per building (lines 193-199, exact on 64-bit keys), ``CloudBuildingEvaluator.eval`` the rest.  Labels and the float32 medians of
the DTM and nDSM planes come from ``instances`` (csrc/dsm_instances.hip).

The entry points of include/t2h_cloud.h are bound here: ``_lib.declare("t2h_cloud.h", SIGNATURES)``.
"""
import ctypes
import math

import torch

from . import _lib
from . import instances
from .evaluator import _plane

_vp, _i, _i64, _sz, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double

# name -> (restype, argtypes); mirrors include/t2h_cloud.h one to one
SIGNATURES = {
    "t2h_cloud_assign": (_i, [_vp, _i64, _i64, _d, _d, _d, _d, _d, _d, _vp, _i, _i, _vp, _vp, _vp]),
    "t2h_cloud_medians_workspace_bytes": (_sz, [_i64, _i]),
    "t2h_cloud_medians": (_i, [_vp, _i64, _vp, _i64, _i, _vp, _vp, _vp, _sz, _vp]),
    "t2h_cloud_metrics": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
}

TINY_MAX = 64           # T2H_CLOUD_TINY_MAX: one wave per segment up to here
SMALL_MAX = 2048        # T2H_CLOUD_SMALL_MAX: one workgroup per segment up to here, radix select above
TABLE_COLS = 8
MODES = {"valid_only": 0, "all": 1}     # T2H_CLOUD_MODE_*
LAUNCHES_PER_ASSIGN = 2                 # the clear of n_bad, the kernel
# two clears, counts, three for the offsets, compaction, the two on-chip classes, 8 x (digit pass + scan) where a segment can
# be large
LAUNCHES_PER_MEDIANS = 2 + 1 + 3 + 1 + 2 + 8 * 2
LAUNCHES_PER_EVAL = LAUNCHES_PER_ASSIGN + LAUNCHES_PER_MEDIANS + 1

_lib.declare("t2h_cloud.h", SIGNATURES)
load = _lib.load


def inverse_coefficients(transform):
    """``(ra, rb, rc, rd, re, rf)`` of the inverse of the forward raster transform ``(a, b, c, d, e, f)`` (pixel -> world:
    ``x = a col + b row + c``, ``y = d col + e row + f``), in Python floats.  The expressions are a restatement of
    ``affine.Affine.__invert__`` (the class of rasterio's ``src.transform``; the package is not a dependency), operation for
    operation, so the coefficients are the reference's bit for bit."""
    coeffs = tuple(transform)[:6]
    if len(coeffs) != 6:
        raise ValueError(f"transform: expected the six coefficients (a, b, c, d, e, f), got {len(coeffs)}")
    a, b, c, d, e, f = (float(v) for v in coeffs)
    det = a * e - b * d
    if det == 0.0 or not math.isfinite(det):
        raise ValueError(f"transform {(a, b, c, d, e, f)} is singular (determinant {det}): it has no inverse")
    idet = 1.0 / det
    ra = e * idet
    rb = -b * idet
    rd = -d * idet
    re = a * idet
    rc = -c * ra - f * rb
    rf = -c * rd - f * re
    if not all(math.isfinite(v) for v in (ra, rb, rc, rd, re, rf)):
        raise ValueError(f"transform {(a, b, c, d, e, f)}: its inverse is not finite")
    return ra, rb, rc, rd, re, rf


def _cloud(points, what, min_cols):
    """A float64 [N, >= min_cols] device tensor whose columns are adjacent (any row stride: ``points[:, :3]`` of a wider list)."""
    if not isinstance(points, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor, got {type(points).__name__}")
    if not points.is_cuda:
        raise RuntimeError(f"{what}: expected a tensor on the MI355X (cuda device), got {points.device}. "
                           "tomosar2height_amd has no CPU path; the CPU restatement lives in tests/ only.")
    if points.dtype != torch.float64:
        raise TypeError(f"{what}: points must be float64 (world coordinates do not fit float32), got {points.dtype}")
    if points.dim() != 2 or points.shape[1] < min_cols:
        raise ValueError(f"{what}: expected [N, >= {min_cols}] points, got {tuple(points.shape)}")
    N = points.shape[0]
    if N > 1 and (points.stride(1) != 1 or points.stride(0) < points.shape[1]):
        points = points.contiguous()
    elif N == 1 and points.stride(1) != 1:
        points = points.contiguous()
    return points


def _row_stride(points):
    return points.stride(0) if points.shape[0] > 1 else points.shape[1]


def _assign(points, labels, inverse):
    N = points.shape[0]
    R, C = labels.shape
    point_label = torch.empty(N, dtype=torch.int32, device=points.device)
    n_bad = torch.empty(1, dtype=torch.int32, device=points.device)
    _lib.call("t2h_cloud_assign", _lib.ptr(points) if N else None, N, max(_row_stride(points), 2), *inverse, _lib.ptr(labels), R, C,
              _lib.ptr(point_label) if N else None, _lib.ptr(n_bad), _lib.stream(), nbytes=N * (24 + 4 + 4))
    return point_label, n_bad


def assign_points(points: torch.Tensor, labels: torch.Tensor, transform):
    """``point_label`` int32 [N] on the device: the label of the pixel under every point, as the reference's
    ``associate_points_with_buildings`` finds it.  ``points`` [N, >= 3] float64 (x, y, ...), ``labels`` [R, C] int32 contiguous,
    ``transform`` the FORWARD six coefficients ``(a, b, c, d, e, f)`` as rasterio / affine give them.  A point outside the raster
    takes the nearest border pixel's label (the reference's clip).  A point whose x or y is not finite raises ``ValueError``
    (one 4-byte copy): the reference's ``astype(int)`` of a NaN is platform-defined."""
    inverse = inverse_coefficients(transform)
    points = _cloud(points, "assign_points", 2)
    _plane(labels, "assign_points labels")
    if labels.dtype != torch.int32:
        raise TypeError(f"assign_points: labels must be int32, got {labels.dtype}")
    if labels.device != points.device:
        raise ValueError(f"assign_points: points on {points.device}, labels on {labels.device}")
    point_label, n_bad = _assign(points, labels, inverse)
    bad = int(n_bad.item())
    if bad:
        raise ValueError(f"assign_points: {bad} of {points.shape[0]} points have a non-finite x or y")
    return point_label


def point_medians(z_or_points: torch.Tensor, point_label: torch.Tensor, K: int):
    """``(counts int32 [K], medians float64 [K])`` on the device: ``np.median(z[point_label == k])`` for k = 1..K, exact in
    float64; NaN (and count 0) for a building without points, NaN for one with a NaN z.  ``z_or_points``: float64 [N] (any
    stride) or [N, >= 3] points, whose column 2 is z."""
    if not isinstance(z_or_points, torch.Tensor) or z_or_points.dim() == 2:
        pts = _cloud(z_or_points, "point_medians", 3)
        N, stride, z_ptr = pts.shape[0], _row_stride(pts), _lib.ptr(pts) + 16
    else:
        pts = z_or_points
        if not pts.is_cuda:
            raise RuntimeError(f"point_medians: expected a tensor on the MI355X (cuda device), got {pts.device}. "
                               "tomosar2height_amd has no CPU path; the CPU restatement lives in tests/ only.")
        if pts.dtype != torch.float64 or pts.dim() != 1:
            raise TypeError(f"point_medians: z must be float64 [N], got {pts.dtype} {tuple(pts.shape)}")
        N = pts.shape[0]
        if N > 1 and pts.stride(0) < 1:
            pts = pts.contiguous()
        stride, z_ptr = (pts.stride(0) if N > 1 else 1), _lib.ptr(pts)
    if not isinstance(point_label, torch.Tensor) or point_label.dtype != torch.int32 or tuple(point_label.shape) != (N,):
        raise TypeError(f"point_medians: point_label must be int32 [{N}]")
    if point_label.device != pts.device:
        raise ValueError(f"point_medians: points on {pts.device}, point_label on {point_label.device}")
    point_label = point_label.contiguous()
    K = int(K)
    if K < 0:
        raise ValueError(f"point_medians: K = {K}")
    dev = pts.device
    counts = torch.empty(K, dtype=torch.int32, device=dev)
    medians = torch.empty(K, dtype=torch.float64, device=dev)
    if K == 0:
        return counts, medians
    need = _lib.ws_bytes("t2h_cloud_medians_workspace_bytes", N, K)
    if need == 0:
        raise ValueError(f"point_medians: {N} points (at most 2^31 - 1)")
    ws = _lib.workspace(need, dev)
    _lib.call("t2h_cloud_medians", z_ptr if N else None, stride, _lib.ptr(point_label) if N else None, N, K, _lib.ptr(counts),
              _lib.ptr(medians), _lib.ptr(ws), need, _lib.stream(), nbytes=N * (2 * 4 + 8 + 12 + 8 * 12) + 28 * K)
    return counts, medians


class CloudBuildingEvaluator:
    def __init__(self, building_mask, dtm, ndsm, transform, connectivity=2):
        """``building_mask`` [R, C] (nonzero = footprint), ``dtm`` and ``ndsm`` [R, C] float32 / float64 on the same grid,
        ``transform`` = the forward six coefficients of that grid (pixel -> world).  The reference crops its rasters by a row or
        two before it uses them and keeps the uncropped file's transform; pass the planes as they are used, with the transform
        they are used with."""
        self.inverse = inverse_coefficients(transform)
        self.transform = tuple(float(v) for v in tuple(transform)[:6])
        _plane(building_mask, "CloudBuildingEvaluator building_mask")
        for name, plane in (("dtm", dtm), ("ndsm", ndsm)):
            _plane(plane, f"CloudBuildingEvaluator {name}")
            if plane.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"CloudBuildingEvaluator: {name} must be float32 or float64, got {plane.dtype}")
            if tuple(plane.shape) != tuple(building_mask.shape):
                raise ValueError(f"{name}: shape {tuple(plane.shape)} is not the mask's {tuple(building_mask.shape)}")
            if plane.device != building_mask.device:
                raise ValueError(f"CloudBuildingEvaluator: mask on {building_mask.device}, {name} on {plane.device}")
        self.mask8 = instances._mask8(building_mask, "CloudBuildingEvaluator building_mask")
        self.dtm, self.ndsm = dtm, ndsm
        self.connectivity = connectivity
        self._buildings = None          # (labels, K, pixel counts, dtm medians, ndsm medians)

    def buildings(self):
        """Labels, K, pixel counts and the float32 medians of the DTM and the nDSM per building: computed on first use (with
        the one 4-byte copy that reads K), then kept."""
        if self._buildings is None:
            R, C = self.mask8.shape
            labels, k_dev = instances._label(self.mask8, 0, 0, R, C, self.connectivity)
            K = int(k_dev.item())
            pixels, dtm_med = instances.segment_medians(self.dtm, labels, K)
            _, ndsm_med = instances.segment_medians(self.ndsm, labels, K)
            self._buildings = (labels, K, pixels, dtm_med, ndsm_med)
        return self._buildings

    def eval(self, points, mode="all"):
        """``(metrics, record)``: ``metrics`` = {"RMSE-B", "MAE-B", "MedAE-B", "max_abs", "n_buildings", "n_valid", "n_nan",
        "n_covered"} (the first four ``None`` when ``n_valid == 0``); ``record`` = {"labels", "point_label", "counts",
        "pred_median", "dtm_median", "ndsm_median", "height"} on the device, ``height`` = pred - dtm before any NaN handling.
        ``mode="all"`` is the reference's ``evaluate_cloud_all`` (a building without points has height 0; a NaN nDSM median
        raises ``ValueError`` as sklearn does there), ``"valid_only"`` its ``evaluate_cloud_valid_only`` (such buildings are
        dropped and counted in ``n_nan``).  ``n_covered``: buildings with at least one point.  One copy (64 bytes) per call."""
        if mode not in MODES:
            raise ValueError(f"CloudBuildingEvaluator.eval: mode = {mode!r}; one of {sorted(MODES)}")
        points = _cloud(points, "CloudBuildingEvaluator.eval", 3)
        if points.device != self.mask8.device:
            raise ValueError(f"CloudBuildingEvaluator.eval: points on {points.device}, rasters on {self.mask8.device}")
        labels, K, _, dtm_med, ndsm_med = self.buildings()
        N = points.shape[0]
        point_label, n_bad = _assign(points, labels, self.inverse)
        counts, pred_med = point_medians(points, point_label, K)
        height = torch.empty(K, dtype=torch.float64, device=points.device)
        record = {"labels": labels, "point_label": point_label, "counts": counts, "pred_median": pred_med, "dtm_median": dtm_med,
                  "ndsm_median": ndsm_med, "height": height}
        metrics = {"RMSE-B": None, "MAE-B": None, "MedAE-B": None, "max_abs": None, "n_buildings": K, "n_valid": 0, "n_nan": 0,
                   "n_covered": 0}
        table = torch.empty(TABLE_COLS, dtype=torch.float64, device=points.device)
        some = K > 0
        _lib.call("t2h_cloud_metrics", _lib.ptr(pred_med) if some else None, _lib.ptr(dtm_med) if some else None,
                  _lib.ptr(ndsm_med) if some else None, _lib.ptr(counts) if some else None, K, MODES[mode], _lib.ptr(n_bad),
                  _lib.ptr(height) if some else None, _lib.ptr(table), _lib.stream(), nbytes=K * (8 + 4 + 4 + 4) * 17 + 8 * K)
        n_valid, n_nan, sum_abs, sum_sq, med_abs, max_abs, n_covered, bad = table.cpu().tolist()   # the one copy (and wait) of the call
        if bad:
            raise ValueError(f"CloudBuildingEvaluator.eval: {int(bad)} of {N} points have a non-finite x or y")
        if mode == "all" and n_nan:
            raise ValueError(f"CloudBuildingEvaluator.eval: {int(n_nan)} of {K} nDSM medians are NaN (mode 'all' keeps every "
                             "building, and the reference's sklearn metrics refuse a NaN); use mode='valid_only'")
        metrics.update({"n_valid": int(n_valid), "n_nan": int(n_nan), "n_covered": int(n_covered)})
        if n_valid > 0:
            metrics.update({"RMSE-B": math.sqrt(sum_sq / n_valid), "MAE-B": sum_abs / n_valid, "MedAE-B": med_abs,
                            "max_abs": max_abs})
        return metrics, record
