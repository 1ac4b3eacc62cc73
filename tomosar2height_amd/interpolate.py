"""Interpolation baselines on the device (reference: scripts/interpolate_nearest.py, scripts/interpolate_idw.py,
scripts/interpolate_bilinear.py; kernels: csrc/dsm_interp.hip, csrc/dsm_tin.hip).

The rows the network is compared against: keep the highest z of every exactly equal (x, y), then rasterise on a regular grid
by the nearest neighbour or by inverse-distance weighting over the k = 8 nearest.  ``CloudIndex`` does the de-duplication and
builds a cell index of the cloud; ``nearest_dsm`` / ``idw_dsm`` return a float64 plane that ``DSMEvaluator.eval`` and
``BuildingEvaluator.eval`` take as it is; ``grid_knn`` gives the neighbour lists themselves.  Row 0 of a raster is ``ymin``
(the scripts flip nothing), node (j, i) lies at ``(xmin + i * resolution, ymin + j * resolution)``, and the maximum is excluded:
``nx = ceil((xmax - xmin) / resolution)``.  Ties at equal distance are resolved by (d2, X, Y) ascending -- the k-d tree of the
reference has no documented order there.

``delaunay_dsm`` is the Delaunay-linear baseline: ``griddata(method='linear')`` of scripts/interpolate_bilinear.py over the
unique cloud SHIFTED to its (xmin, ymin), NaN outside the convex hull; ``grid_simplex`` gives every node's triangle and
barycentric coordinates.  No triangulation is built: a node's triangle is found by a local search over the cell index
(DESIGN.md section 4.8).  On raw world coordinates the script itself interpolates over a triangulation of a SUBSET of the cloud
(Qhull drops the points its lifted paraboloid cannot resolve); that is not reproduced, and is why ``linear_dsm`` -- the name
for the script's own output -- stays unbuilt.

The entry points of include/t2h_interp.h and include/t2h_tin.h are bound here, one ``_lib.declare`` per header
(``SIGNATURES``, ``TIN_SIGNATURES``).
"""
import ctypes
import math
import warnings

import torch

from . import _lib

_vp, _i, _i64, _sz, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_double

_GRID = [_vp, _vp, _i, _d, _d, _d, _i, _i, _d, _i, _i]           # unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx
# name -> (restype, argtypes); mirrors include/t2h_interp.h one to one
SIGNATURES = {
    "t2h_interp_max_cells": (_i64, [_i64]),
    "t2h_interp_bounds_workspace_bytes": (_sz, [_i64]),
    "t2h_interp_bounds": (_i, [_vp, _i64, _vp, _vp, _sz, _vp]),
    "t2h_interp_index_workspace_bytes": (_sz, [_i64]),
    "t2h_interp_index": (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "t2h_interp_knn": (_i, _GRID + [_i, _vp, _vp, _vp]),
    "t2h_interp_nearest": (_i, _GRID + [_vp, _vp]),
    "t2h_interp_idw": (_i, _GRID + [_i, _vp, _vp]),
}

# name -> (restype, argtypes); mirrors include/t2h_tin.h one to one
TIN_SIGNATURES = {
    "t2h_tin_hull_workspace_bytes": (_sz, [_i64]),
    "t2h_tin_hull": (_i, [_vp, _i, _d, _d, _vp, _vp, _vp, _sz, _vp]),       # unique, M, xmin, ymin, hull, status, ws, bytes, stream
    "t2h_tin_simplex": (_i, _GRID + [_vp, _i, _vp, _vp, _vp, _vp]),         # ..., hull, n_hull, tri, bary, status, stream
    "t2h_tin_linear": (_i, _GRID + [_vp, _i, _vp, _vp, _vp]),               # ..., hull, n_hull, out, status, stream
}

TILE = 16               # T2H_INTERP_TILE: nodes per tile edge, one workgroup per tile
CHUNK = 2048            # T2H_INTERP_CHUNK: points staged in LDS at a time
MAX_K = 8               # T2H_INTERP_MAX_K
CELL_POINTS = 4         # T2H_INTERP_CELL_POINTS: input points per cell the cell edge aims at
TABLE_COLS = 16         # T2H_INTERP_TABLE_COLS
# bounds: partial rows, final row + cell grid.  index: clear, counts, 3 for the offsets, fill, rank, flags, 3 for their scan,
# compaction, cell offsets of the unique cloud
LAUNCHES_PER_BOUNDS = 2
LAUNCHES_PER_INDEX = 1 + 1 + 3 + 1 + 1 + 1 + 3 + 1 + 1
LAUNCHES_PER_RASTER = 1
TIN_DIRECTIONS = 16     # T2H_TIN_DIRECTIONS
TIN_MAX_PIVOTS = 64     # T2H_TIN_MAX_PIVOTS
TIN_STATUS_COLS = 8     # T2H_TIN_STATUS_COLS
LAUNCHES_PER_HULL = 4                   # partial extremes, polygon, filter, sort + chain
LAUNCHES_PER_TIN_RASTER = 1 + 1         # the clear of the status, the search

_lib.declare("t2h_interp.h", SIGNATURES)
_lib.declare("t2h_tin.h", TIN_SIGNATURES)
load = _lib.load


class CloudIndex:
    """Bounds, z-max de-duplication and cell index of an [N, 3] cloud of (X, Y, Z).

    ``unique`` [M, 3] float64: one row per distinct (X, Y) with the largest Z, in cell-major order (inside a cell by X, then
    Y); ``origin`` = (xmin, ymin); ``bounds`` = (xmin, xmax, ymin, ymax); ``grid_shape(resolution)`` = (ny, nx).  Building it
    costs one 128-byte copy to the host (and the wait for it): the raster's shape depends on what it carries."""

    def __init__(self, points: torch.Tensor):
        if not isinstance(points, torch.Tensor):
            raise TypeError(f"CloudIndex: expected a torch tensor, got {type(points).__name__}")
        if points.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"CloudIndex: points must be float64 (or float32, widened exactly), got {points.dtype}")
        if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
            raise ValueError(f"CloudIndex: expected [N, 3] points with N >= 1, got {tuple(points.shape)}")
        if not points.is_cuda:
            _lib.require_device(points, what="CloudIndex")
        pts = points.to(torch.float64).contiguous()
        N, dev = pts.shape[0], pts.device
        cap = int(load().t2h_interp_max_cells(N))
        if cap == 0:
            raise ValueError(f"CloudIndex: {N} points (1 .. 2^31 - 1)")
        table = torch.empty(TABLE_COLS, dtype=torch.float64, device=dev)
        unique = torch.empty((N, 3), dtype=torch.float64, device=dev)
        cell_offsets = torch.empty(cap + 1, dtype=torch.int32, device=dev)
        st = _lib.stream()
        need = _lib.ws_bytes("t2h_interp_bounds_workspace_bytes", N)
        ws = _lib.workspace(need, dev)
        _lib.call("t2h_interp_bounds", _lib.ptr(pts), N, _lib.ptr(table), _lib.ptr(ws), need, st, nbytes=24 * N)
        need = _lib.ws_bytes("t2h_interp_index_workspace_bytes", N)
        ws = _lib.workspace(need, dev)
        _lib.call("t2h_interp_index", _lib.ptr(pts), N, _lib.ptr(table), _lib.ptr(unique), _lib.ptr(cell_offsets), _lib.ptr(ws),
                  need, st, nbytes=N * (2 * 24 + 4 * 24 + 24 + 5 * 4) + 5 * 4 * cap)
        xmin, xmax, ymin, ymax, bad, h, gx, gy, M = table.cpu().tolist()[:9]      # the one copy (and wait)
        if bad > 0:
            raise ValueError(f"CloudIndex: {int(bad)} of {N} points have a non-finite coordinate or height (the reference's "
                             "pandas group-by would skip NaN keys; that is not reproduced)")
        self.n_points, self.n_unique = N, int(M)
        self.bounds = (xmin, xmax, ymin, ymax)
        self.origin = (xmin, ymin)
        self.cell_edge, self.cells = h, (int(gy), int(gx))
        self.unique = unique[:self.n_unique]
        self.cell_offsets = cell_offsets
        self.device = dev

    def grid_shape(self, resolution: float = 1.0):
        """``(ny, nx)`` of the raster at ``resolution``: numpy's ``len(arange(min, max, resolution))`` per axis."""
        res = _resolution(resolution)
        xmin, xmax, ymin, ymax = self.bounds
        return (int(math.ceil((ymax - ymin) / res)), int(math.ceil((xmax - xmin) / res)))

    def hull(self):
        """``hull [n] int32``: the convex hull of ``unique`` as rows of it, counter-clockwise from the smallest (X, Y), points on
        an edge left out.  Computed once and kept (one 32-byte copy to the host, and the wait for it).  ``ValueError`` for a
        cloud with fewer than 3 distinct points or with all of them on one line."""
        hit = getattr(self, "_hull", None)
        if hit is None:
            M, dev = self.n_unique, self.device
            hull = torch.empty(M + 1, dtype=torch.int32, device=dev)
            status = torch.empty(TIN_STATUS_COLS, dtype=torch.int32, device=dev)
            need = _lib.ws_bytes("t2h_tin_hull_workspace_bytes", M)
            ws = _lib.workspace(need, dev)
            _lib.call("t2h_tin_hull", _lib.ptr(self.unique), M, self.origin[0], self.origin[1], _lib.ptr(hull), _lib.ptr(status),
                      _lib.ptr(ws), need, _lib.stream(), nbytes=2 * 24 * M)
            n, degenerate, survivors = status.cpu().tolist()[:3]                  # the one copy (and wait)
            self.hull_survivors = survivors
            hit = self._hull = (None if degenerate else hull[:n],)
        if hit[0] is None:
            raise ValueError(f"CloudIndex.hull: the {self.n_unique} distinct (x, y) of this cloud span no area (fewer than 3, or all "
                             "on one line): there is no triangle to interpolate over (Qhull refuses such input too)")
        return hit[0]

    def _grid_args(self, res, ny, nx):
        return (_lib.ptr(self.unique), _lib.ptr(self.cell_offsets), self.n_unique, self.origin[0], self.origin[1], self.cell_edge,
                self.cells[1], self.cells[0], res, ny, nx)


def _resolution(resolution):
    res = float(resolution)
    if not (res > 0.0 and math.isfinite(res)):
        raise ValueError(f"resolution = {resolution!r}; a positive finite pixel size")
    return res


def _index(points_or_index):
    return points_or_index if isinstance(points_or_index, CloudIndex) else CloudIndex(points_or_index)


def _check_k(index, k, what):
    if int(k) != k or not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k = {k!r} (1 .. {MAX_K})")
    if index.n_unique < k:
        raise ValueError(f"{what}: {index.n_unique} distinct (x, y) for k = {k} neighbours (the reference would index past "
                         "the end of the cloud there)")
    return int(k)


def _work(index, ny, nx):
    """Algorithmic bytes of one raster launch, for a KernelTimeline: the unique cloud once per tile ring is not known before
    the run; the floor is the cloud and the offsets once."""
    return 24 * index.n_unique + 4 * (index.cells[0] * index.cells[1] + 1)


def grid_knn(index: CloudIndex, resolution: float = 1.0, k: int = 8):
    """``(d2 [ny, nx, k] float64, idx [ny, nx, k] int32)``: squared distances and rows of ``index.unique`` of the k nearest
    neighbours of every raster node, in (d2, X, Y) order."""
    if not isinstance(index, CloudIndex):
        raise TypeError(f"grid_knn: expected a CloudIndex, got {type(index).__name__}")
    k = _check_k(index, k, "grid_knn")
    res = _resolution(resolution)
    ny, nx = index.grid_shape(res)
    d2 = torch.empty((ny, nx, k), dtype=torch.float64, device=index.device)
    idx = torch.empty((ny, nx, k), dtype=torch.int32, device=index.device)
    if ny * nx > 0:
        _lib.call("t2h_interp_knn", *index._grid_args(res, ny, nx), k, _lib.ptr(d2), _lib.ptr(idx), _lib.stream(),
                  nbytes=_work(index, ny, nx) + 12 * k * ny * nx)
    return d2, idx


def nearest_dsm(points_or_index, resolution: float = 1.0):
    """``(dsm [ny, nx] float64, (xmin, ymin))``: scripts/interpolate_nearest.py on the device."""
    index = _index(points_or_index)
    _check_k(index, 1, "nearest_dsm")
    res = _resolution(resolution)
    ny, nx = index.grid_shape(res)
    out = torch.empty((ny, nx), dtype=torch.float64, device=index.device)
    if ny * nx > 0:
        _lib.call("t2h_interp_nearest", *index._grid_args(res, ny, nx), _lib.ptr(out), _lib.stream(),
                  nbytes=_work(index, ny, nx) + 16 * ny * nx)
    return out, index.origin


def idw_dsm(points_or_index, resolution: float = 1.0, k: int = 8, power: float = 2):
    """``(dsm [ny, nx] float64, (xmin, ymin))``: scripts/interpolate_idw.py on the device.  A coincident point has weight 1
    beside the others' 1 / d^2, as there."""
    if power != 2:
        raise ValueError(f"idw_dsm: power = {power!r}; only the reference's power = 2 is built")
    index = _index(points_or_index)
    k = _check_k(index, k, "idw_dsm")
    res = _resolution(resolution)
    ny, nx = index.grid_shape(res)
    out = torch.empty((ny, nx), dtype=torch.float64, device=index.device)
    if ny * nx > 0:
        _lib.call("t2h_interp_idw", *index._grid_args(res, ny, nx), k, _lib.ptr(out), _lib.stream(),
                  nbytes=_work(index, ny, nx) + (8 + 8 * k) * ny * nx)
    return out, index.origin


def _tin_status(status, what, return_status):
    capped, unresolved, pivots, walk_pivots = status.cpu().tolist()[:4]           # one 32-byte copy (and wait)
    out = {"capped": capped, "unresolved": unresolved, "pivots": pivots, "walk_pivots": walk_pivots}
    if (capped or unresolved) and not return_status:
        warnings.warn(f"{what}: {capped} nodes stopped at {TIN_MAX_PIVOTS} pivots and {unresolved} nodes inside the hull found no "
                      "triangle; their values are not the Delaunay interpolant (pass return_status=True for the counts)",
                      RuntimeWarning, stacklevel=3)
    return out


def grid_simplex(index: CloudIndex, resolution: float = 1.0, return_status: bool = False):
    """``(tri [ny, nx, 3] int32, bary [ny, nx, 3] float64)``: for every raster node the Delaunay triangle of the shifted unique
    cloud that contains it, as rows of ``index.unique`` in ascending order, and its barycentric coordinates in that order;
    -1 / NaN outside the convex hull.  The counterpart of ``grid_knn``.  With ``return_status`` a third value: ``{"capped":
    nodes that stopped at 64 pivots, "unresolved": ..., "pivots": ..., "walk_pivots": ...}``; without it, nodes that were capped
    raise a ``RuntimeWarning``."""
    if not isinstance(index, CloudIndex):
        raise TypeError(f"grid_simplex: expected a CloudIndex, got {type(index).__name__}")
    res = _resolution(resolution)
    hull = index.hull()
    ny, nx = index.grid_shape(res)
    tri = torch.empty((ny, nx, 3), dtype=torch.int32, device=index.device)
    bary = torch.empty((ny, nx, 3), dtype=torch.float64, device=index.device)
    status = torch.zeros(TIN_STATUS_COLS, dtype=torch.int32, device=index.device)
    if ny * nx > 0:
        _lib.call("t2h_tin_simplex", *index._grid_args(res, ny, nx), _lib.ptr(hull), hull.shape[0], _lib.ptr(tri), _lib.ptr(bary),
                  _lib.ptr(status), _lib.stream(), nbytes=_work(index, ny, nx) + 36 * ny * nx)
    st = _tin_status(status, "grid_simplex", return_status)
    return (tri, bary, st) if return_status else (tri, bary)


def delaunay_dsm(points_or_index, resolution: float = 1.0, return_status: bool = False):
    """``(dsm [ny, nx] float64, (xmin, ymin))``: scripts/interpolate_bilinear.py on the device, over the unique cloud shifted to
    its (xmin, ymin) -- ``griddata(method='linear')`` there -- NaN outside the convex hull.  On raw world coordinates the
    script's Qhull drops points, which is not reproduced.  A cloud without area raises ``ValueError``.
    ``return_status`` as for ``grid_simplex``."""
    index = _index(points_or_index)
    res = _resolution(resolution)
    hull = index.hull()
    ny, nx = index.grid_shape(res)
    out = torch.empty((ny, nx), dtype=torch.float64, device=index.device)
    status = torch.zeros(TIN_STATUS_COLS, dtype=torch.int32, device=index.device)
    if ny * nx > 0:
        _lib.call("t2h_tin_linear", *index._grid_args(res, ny, nx), _lib.ptr(hull), hull.shape[0], _lib.ptr(out), _lib.ptr(status),
                  _lib.stream(), nbytes=_work(index, ny, nx) + 8 * ny * nx)
    st = _tin_status(status, "delaunay_dsm", return_status)
    return (out, index.origin, st) if return_status else (out, index.origin)


def linear_dsm(points_or_index, resolution: float = 1.0):
    """The output of scripts/interpolate_bilinear.py on raw world coordinates is not built; the baseline
    itself is ``delaunay_dsm``."""
    raise NotImplementedError("linear_dsm: the output of scripts/interpolate_bilinear.py on raw world coordinates, with the points "
                              "Qhull drops there, is not reproduced; use delaunay_dsm, the same griddata on the cloud shifted "
                              "to its origin (DESIGN.md section 7)")
