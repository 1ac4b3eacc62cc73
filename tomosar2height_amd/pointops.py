"""PointNet++ point operators on the MI355X (reference: tomosar2height/encoder/pointnetpp.py:220-320 and :90-97): farthest
point sampling, radius grouping, grouped rows, grouped max and 3-nearest-neighbour interpolation over csrc/pnpp.hip.

Argument order and result shapes are the reference's; tensors are point-major (``[B, N, C]``), as the reference's helpers take
them.  ``group_rows``, ``group_max`` / ``group_max_rows`` and ``three_nn_interpolate`` are autograd functions, differentiable in
their FEATURES (``points``, ``rows``, ``points2``); ``xyz`` is input data, so sampling, grouping, the 3-NN indices and the 3-NN
weights carry no gradient.  The adjoint of a gather is a sum over an inverted index
(``index_transpose``), in a fixed association and without a float atomic: two backward passes give the same bytes.  There is
no CPU path: a tensor that is not on the device raises.

Squared distances are taken by differences in fp32, ``(dx*dx + dy*dy) + dz*dz``; the reference's matmul form rounds
differently within a few ulps of 6 at unit coordinates, which can move a point that lies that close to a ball's boundary, or
reorder two neighbours that close to equidistant.  Ties are broken by the lowest index everywhere (FPS maxima, 3-NN distances);
the reference leaves them to ``torch.max`` / an unstable ``sort``.

The entry points of include/t2h_pnpp.h are bound here: ``_lib.declare("t2h_pnpp.h", SIGNATURES)``.
"""
import ctypes
import numbers

import torch

from . import _lib, switches

_vp, _i, _i64, _sz, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float

# name -> (restype, argtypes); mirrors include/t2h_pnpp.h one to one
SIGNATURES = {
    "t2h_fps_workspace_bytes": (_sz, [_i, _i, _i]),
    "t2h_fps": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _sz, _vp]),
    "t2h_ball_query": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _vp, _vp]),
    "t2h_group_rows": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "t2h_group_max": (_i, [_vp, _i, _i64, _i, _i, _vp, _vp]),
    "t2h_three_nn_interp": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "t2h_group_max_bwd": (_i, [_vp, _i, _i64, _i, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "t2h_index_transpose": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "t2h_rows_gather_bwd": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "t2h_bn_col_stats": (_i, [_vp, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "t2h_bn_apply_relu": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "t2h_bn_running_update": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _vp]),
    "t2h_bn_bwd_reduce": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "t2h_bn_bwd_apply": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp]),
}

FPS_ONE_WG_MAX = 2048       # T2H_FPS_ONE_WG_MAX
# T2H_FPS_SLICE: points per workgroup of the sliced FPS (one launch per centroid).  Unset: clouds of up to FPS_ONE_WG_MAX points
# take the one-workgroup form and larger ones slices of FPS_SLICE_DEFAULT; set (a multiple of 64), EVERY cloud takes the sliced
# form with that slice -- how a test runs it on a small cloud.  Both forms give the same bytes.
FPS_SLICE_DEFAULT = 1024
BN_SLAB = 256               # T2H_BN_SLAB: rows per slab of the BatchNorm column reductions

_lib.declare("t2h_pnpp.h", SIGNATURES)
load = _lib.load


def fps_slice(n: int) -> int:
    """Points per workgroup ``farthest_point_sample`` will use on an N-point cloud (0: the one-workgroup form)."""
    s = switches.get("T2H_FPS_SLICE")
    if s is not None:
        if s < 64 or s % 64:
            raise ValueError(f"T2H_FPS_SLICE={s}: a multiple of 64 is needed")
        return s
    return 0 if n <= FPS_ONE_WG_MAX else FPS_SLICE_DEFAULT


def fps_launches(n: int, npoint: int) -> int:
    return 1 if fps_slice(n) == 0 else npoint


def _cloud(t, what, cols=3):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor, got {type(t).__name__}")
    _lib.require_device(t, what=what)
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: float32 expected, got {t.dtype}")
    if t.dim() != 3 or (cols is not None and t.shape[2] != cols) or t.shape[1] < 1 or t.shape[0] < 1:
        raise ValueError(f"{what}: expected [B, N, {cols if cols is not None else 'C'}], got {tuple(t.shape)}")
    return t


def fps_start(start, b: int, n: int, device) -> torch.Tensor:
    """``start`` of ``farthest_point_sample`` as an int64 [B] device tensor: None draws ``torch.randint(0, N, (B,))`` on the
    device (pointnetpp.py:232), an int is used for every cloud, a tensor is taken as it is."""
    if start is None:
        return torch.randint(0, n, (b,), dtype=torch.long, device=device)
    if isinstance(start, numbers.Integral):
        return torch.full((b,), int(start), dtype=torch.long, device=device)
    if not isinstance(start, torch.Tensor):
        raise TypeError(f"fps start: expected None, an integer or an int64 [{b}] tensor, got {type(start).__name__}")
    if start.dtype != torch.long or tuple(start.shape) != (b,):
        raise ValueError(f"fps start: expected an int64 [{b}] tensor, got {start.dtype} {tuple(start.shape)}")
    _lib.require_device(start, what="fps start")
    return start


def farthest_point_sample(xyz: torch.Tensor, npoint: int, start=None) -> torch.Tensor:
    """pointnetpp.py:220-241: ``xyz`` [B, N, 3] -> centroid indices [B, npoint] int64.  ``start``: see ``fps_start``; on equal
    maxima the next centroid is the lowest index of the maximum."""
    _cloud(xyz, "farthest_point_sample")
    lib = load()
    b, n, _ = xyz.shape
    start = fps_start(start, b, n, xyz.device)
    out = torch.empty(b, npoint, dtype=torch.long, device=xyz.device)
    slice_ = fps_slice(n)
    nws = int(lib.t2h_fps_workspace_bytes(b, n, slice_))
    ws = _lib.workspace(nws, xyz.device)
    _lib.call("t2h_fps", _lib.ptr(xyz), b, n, npoint, _lib.ptr(start), slice_, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream(),
              nbytes=b * n * (12 + (8 * npoint if slice_ else 0)), flops=9 * b * n * npoint)
    return out


def index_points(points: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """pointnetpp.py:200-217 for ``idx`` [B, S]: rows of ``points`` [B, N, C] -> [B, S, C] (a torch gather: plumbing)."""
    return torch.gather(points, 1, idx.unsqueeze(-1).expand(-1, -1, points.shape[2]))


def query_ball_point(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor) -> torch.Tensor:
    """pointnetpp.py:244-264: per query the first ``nsample`` indices, in index order, within ``radius`` -> [B, S, nsample] int64,
    padded with the first.  The threshold is ``radius ** 2`` rounded to fp32."""
    _cloud(xyz, "query_ball_point xyz")
    _cloud(new_xyz, "query_ball_point new_xyz")
    b, n, _ = xyz.shape
    s = new_xyz.shape[1]
    idx = torch.empty(b, s, nsample, dtype=torch.long, device=xyz.device)
    _lib.call("t2h_ball_query", _lib.ptr(xyz), _lib.ptr(new_xyz), b, n, s, float(radius) ** 2, nsample, _lib.ptr(idx), _lib.stream(),
              nbytes=12 * b * (n + s) + 8 * b * s * nsample)
    return idx


def _group_rows(xyz, new_xyz, points, idx, ld):
    b, n, _ = xyz.shape
    _, s, ns = idx.shape
    d = 0 if points is None else points.shape[2]
    rows = torch.empty(b * s * ns, ld, dtype=torch.float32, device=xyz.device)
    _lib.call("t2h_group_rows", _lib.ptr(xyz), _lib.ptr(new_xyz), None if points is None else _lib.ptr(points), _lib.ptr(idx), b, n,
              s, ns, d, ld, _lib.ptr(rows), _lib.stream(), nbytes=b * s * ns * (8 + 4 * (3 + d) + 4 * ld))
    return rows


def index_transpose(idx: torch.Tensor, n: int):
    """The inverted index of ``idx`` [B, ...] int64 over ``n`` sources (t2h_index_transpose): ``offsets`` [B, n + 1] int32 and
    ``entries`` [B, E] int32, per cloud the stable argsort of the flattened ``idx``; an index outside [0, n) counts as n - 1."""
    _lib.require_device(idx, what="index_transpose")
    if idx.dtype != torch.long or idx.dim() < 2:
        raise ValueError(f"index_transpose: expected an int64 [B, ...] tensor, got {idx.dtype} {tuple(idx.shape)}")
    b = idx.shape[0]
    e = idx.numel() // b
    offsets = torch.empty(b, n + 1, dtype=torch.int32, device=idx.device)
    entries = torch.empty(b, e, dtype=torch.int32, device=idx.device)
    cursor = torch.empty(b, n, dtype=torch.int32, device=idx.device)          # scratch: [B, n] int32 (include/t2h_pnpp.h)
    _lib.call("t2h_index_transpose", _lib.ptr(idx), b, e, n, _lib.ptr(offsets), _lib.ptr(entries), _lib.ptr(cursor), _lib.stream(),
              nbytes=b * (3 * 8 * e + 4 * e + 12 * n))
    return offsets, entries


def rows_gather_bwd(g: torch.Tensor, col0: int, d: int, weight, fan: int, offsets, entries, n: int) -> torch.Tensor:
    """out [B, n, d] = per source the sum, over the positions that read it, of ``weight`` x columns ``col0 .. col0 + d`` of the
    rows ``g`` [B * E / fan, >= col0 + d] (t2h_rows_gather_bwd; ``g`` may be a column slice of wider rows)."""
    _lib.require_device(offsets, entries, weight, what="rows_gather_bwd")
    if g.dim() != 2 or g.dtype != torch.float32 or g.stride(1) != 1:
        raise ValueError("rows_gather_bwd: expected fp32 rows with unit column stride")
    b, e = entries.shape
    if g.shape[0] * fan != b * e or g.shape[1] < col0 + d:
        raise ValueError(f"rows_gather_bwd: {tuple(g.shape)} rows for {b} x {e} entries at fan {fan}, columns {col0} .. {col0 + d}")
    out = torch.empty(b, n, d, dtype=torch.float32, device=g.device)
    _lib.call("t2h_rows_gather_bwd", _lib.ptr(g), g.stride(0), col0, d, None if weight is None else _lib.ptr(weight), fan,
              _lib.ptr(offsets), _lib.ptr(entries), b, e, n, _lib.ptr(out), _lib.stream(),
              nbytes=b * e * (4 * d + 8) + 4 * b * n * d, flops=2 * b * e * d)
    return out


def _row_slice(g: torch.Tensor) -> torch.Tensor:
    """``g`` [..., d] as 2-D rows the kernels can read in place: a column slice of contiguous rows stays a view."""
    g2 = g.reshape(-1, g.shape[-1]) if g.dim() != 2 else g
    if g2.stride(1) != 1 or g2.stride(0) < g2.shape[1]:
        g2 = g2.contiguous()
    return g2


class _GroupRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, xyz, new_xyz, idx, ld):
        ctx.save_for_backward(idx)
        ctx.n, ctx.d = points.shape[1], points.shape[2]
        return _group_rows(xyz, new_xyz, points, idx, ld)

    @staticmethod
    def backward(ctx, grows):
        idx, = ctx.saved_tensors
        offsets, entries = index_transpose(idx, ctx.n)          # built here: only when ``points`` wants a gradient
        return rows_gather_bwd(_row_slice(grows), 3, ctx.d, None, 1, offsets, entries, ctx.n), None, None, None, None


def group_rows(xyz, new_xyz, points, idx, ld=None) -> torch.Tensor:
    """Rows [B * S * nsample, ld] = grouped xyz minus the centroid | grouped features | zeros (``ld`` >= 3 + D: the row length
    the layers' products want, a multiple of 4).  Differentiable in ``points``: the gradient is the sum, per point, of the rows
    that gathered it (columns 3 .. 3 + D), over the transpose of ``idx``, which is built in the backward pass."""
    d = 0 if points is None else points.shape[2]
    ld = 3 + d if ld is None else ld
    if points is None or not (torch.is_grad_enabled() and points.requires_grad):
        return _group_rows(xyz, new_xyz, points, idx, ld)
    return _GroupRows.apply(points, xyz, new_xyz, idx, ld)


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, start=None):
    """pointnetpp.py:267-300: -> new_xyz [B, npoint, 3], new_points [B, npoint, nsample, 3 + D] (with ``returnfps`` also the
    grouped xyz and the FPS indices, as the reference)."""
    _cloud(xyz, "sample_and_group xyz")
    if points is not None:
        _cloud(points, "sample_and_group points", cols=None)
    b = xyz.shape[0]
    fps_idx = farthest_point_sample(xyz, npoint, start)
    new_xyz = index_points(xyz, fps_idx).contiguous()
    idx = query_ball_point(radius, nsample, xyz, new_xyz)
    new_points = group_rows(xyz, new_xyz, points, idx).view(b, npoint, nsample, -1)
    if returnfps:
        grouped_xyz = torch.gather(xyz, 1, idx.view(b, -1, 1).expand(-1, -1, 3)).view(b, npoint, nsample, 3)
        return new_xyz, new_points, grouped_xyz, fps_idx
    return new_xyz, new_points


def _group_max_rows(rows, nsample, c):
    groups = rows.shape[0] // nsample
    out = torch.empty(groups, c, dtype=torch.float32, device=rows.device)
    _lib.call("t2h_group_max", _lib.ptr(rows), rows.stride(0), groups, nsample, c, _lib.ptr(out), _lib.stream(),
              nbytes=4 * c * (rows.shape[0] + groups))
    return out


def group_max_bwd(rows, out, gout, nsample: int, relu: bool = False, gld: int = None) -> torch.Tensor:
    """Gradient of the rows [groups * nsample, gld] of ``group_max_rows`` (t2h_group_max_bwd): ``gout`` goes to the lowest row
    of each group that holds the maximum ``out``, +0 elsewhere; ``relu``: +0 also in every column whose maximum is not positive
    (the mask of a ReLU applied to the rows before the max)."""
    _lib.require_device(rows, out, gout, what="group_max_bwd")
    groups, c = out.shape
    gld = c if gld is None else gld
    grows = torch.empty(groups * nsample, gld, dtype=torch.float32, device=rows.device)
    _lib.call("t2h_group_max_bwd", _lib.ptr(rows), rows.stride(0), groups, nsample, c, _lib.ptr(out), _lib.ptr(gout), int(bool(relu)),
              _lib.ptr(grows), gld, _lib.stream(), nbytes=4 * groups * (nsample * (c + gld) + 2 * c))
    return grows


class _GroupMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, nsample, c):
        out = _group_max_rows(rows, nsample, c)
        ctx.save_for_backward(rows, out)
        ctx.nsample = nsample
        return out

    @staticmethod
    def backward(ctx, gout):
        rows, out = ctx.saved_tensors
        return group_max_bwd(rows, out, gout.contiguous(), ctx.nsample, gld=rows.shape[1]), None, None


def group_max_rows(rows: torch.Tensor, nsample: int, c: int = None) -> torch.Tensor:
    """[groups * nsample, ld] rows -> [groups, c]: the max over each group's rows (columns 0 .. c).  Differentiable in ``rows``:
    the lowest row that holds the maximum takes the gradient."""
    _lib.require_device(rows, what="group_max")
    c = rows.shape[1] if c is None else c
    if torch.is_grad_enabled() and rows.requires_grad:
        return _GroupMax.apply(rows, nsample, c)
    return _group_max_rows(rows, nsample, c)


def group_max(new_points: torch.Tensor) -> torch.Tensor:
    """``torch.max(new_points, 2)[0]`` of pointnetpp.py:55 on point-major groups: [B, S, nsample, C] -> [B, S, C]."""
    if not isinstance(new_points, torch.Tensor) or new_points.dim() != 4:
        raise ValueError("group_max: expected [B, S, nsample, C]")
    _lib.require_device(new_points, what="group_max")
    b, s, ns, c = new_points.shape
    return group_max_rows(new_points.view(b * s * ns, c), ns).view(b, s, c)


def _three_nn_interpolate(xyz1, xyz2, points2):
    b, n, _ = xyz1.shape
    s, d = xyz2.shape[1], points2.shape[2]
    idx = torch.empty(b, n, 3, dtype=torch.long, device=xyz1.device)
    weight = torch.empty(b, n, 3, dtype=torch.float32, device=xyz1.device)
    out = torch.empty(b, n, d, dtype=torch.float32, device=xyz1.device)
    _lib.call("t2h_three_nn_interp", _lib.ptr(xyz1), _lib.ptr(xyz2), _lib.ptr(points2), b, n, s, d, _lib.ptr(idx), _lib.ptr(weight),
              _lib.ptr(out), _lib.stream(), nbytes=b * n * (12 + 36 + 16 * d) + b * s * 12, flops=b * n * (9 * s + 5 * d))
    return out, idx, weight


class _ThreeNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points2, xyz1, xyz2):
        out, idx, weight = _three_nn_interpolate(xyz1, xyz2, points2)
        ctx.mark_non_differentiable(idx, weight)
        ctx.save_for_backward(idx, weight)
        ctx.s = points2.shape[1]
        return out, idx, weight

    @staticmethod
    def backward(ctx, gout, _gidx, _gweight):
        idx, weight = ctx.saved_tensors
        offsets, entries = index_transpose(idx, ctx.s)
        return rows_gather_bwd(_row_slice(gout), 0, gout.shape[-1], weight, 3, offsets, entries, ctx.s), None, None


def three_nn_interpolate(xyz1: torch.Tensor, xyz2: torch.Tensor, points2: torch.Tensor):
    """pointnetpp.py:87-97: features ``points2`` [B, S, D] at ``xyz2`` [B, S, 3] interpolated to ``xyz1`` [B, N, 3] with
    inverse-square-distance weights over the three nearest sources -> (interpolated [B, N, D], idx [B, N, 3] int64, weight
    [B, N, 3]).  ``S == 1`` repeats the one source row (idx 0, weight 1, 0, 0).  Differentiable in ``points2`` (per source the
    weighted sum of the target rows that read it); ``idx`` and ``weight`` never require a gradient."""
    _cloud(xyz1, "three_nn_interpolate xyz1")
    _cloud(xyz2, "three_nn_interpolate xyz2")
    _cloud(points2, "three_nn_interpolate points2", cols=None)
    if points2.shape[:2] != xyz2.shape[:2] or xyz2.shape[0] != xyz1.shape[0]:
        raise ValueError("three_nn_interpolate: xyz2 and points2 must share [B, S]")
    if torch.is_grad_enabled() and points2.requires_grad:
        return _ThreeNN.apply(points2, xyz1, xyz2)
    return _three_nn_interpolate(xyz1, xyz2, points2)


# ------------------------------------------------------------------------------------------- BatchNorm batch statistics
def _bn_rows(t, c, what):
    """``t`` as fp32 device rows [M, >= c] with unit column stride (a column slice of wider rows stays a view)."""
    _lib.require_device(t, what=what)
    if t.dim() != 2 or t.dtype != torch.float32 or t.stride(1) != 1 or t.shape[1] < c or t.stride(0) < t.shape[1]:
        raise ValueError(f"{what}: expected fp32 rows [M, >= {c}] with unit column stride, got {t.dtype} {tuple(t.shape)}")
    return t


def _bn_rows_count(m: int, c: int):
    if m < 2:                                                  # torch's wording (torch.nn.functional._verify_batch_size)
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {torch.Size([m, c])}")


def _bn_partial(m, c, planes, device):
    return torch.empty(planes * (-(-m // BN_SLAB)) * c, dtype=torch.float32, device=device)


def bn_col_stats(z: torch.Tensor, c: int, eps: float):
    """(mean, var, rstd) [c] of the columns 0 .. c of the rows ``z`` [M, ld]: the biased batch variance by two passes and
    ``rstd = 1 / sqrt(var + eps)`` (t2h_bn_col_stats; fixed association, include/t2h_pnpp.h)."""
    _bn_rows(z, c, "bn_col_stats")
    m = z.shape[0]
    _bn_rows_count(m, c)
    mean, var, rstd = (torch.empty(c, dtype=torch.float32, device=z.device) for _ in range(3))
    partial = _bn_partial(m, c, 1, z.device)
    _lib.call("t2h_bn_col_stats", _lib.ptr(z), z.stride(0), m, c, float(eps), _lib.ptr(partial), _lib.ptr(mean), _lib.ptr(var),
              _lib.ptr(rstd), _lib.stream(), nbytes=8 * m * c, flops=4 * m * c)
    return mean, var, rstd


def bn_apply_relu(z: torch.Tensor, c: int, mean, rstd, gamma, beta, ldy: int = None) -> torch.Tensor:
    """y [M, ldy] = relu(z * s + t), s = gamma * rstd, t = beta - mean * s; columns c .. ldy are zero (t2h_bn_apply_relu)."""
    _bn_rows(z, c, "bn_apply_relu")
    _lib.require_device(mean, rstd, gamma, beta, what="bn_apply_relu")
    m = z.shape[0]
    _bn_rows_count(m, c)
    ldy = c if ldy is None else ldy
    y = torch.empty(m, ldy, dtype=torch.float32, device=z.device)
    _lib.call("t2h_bn_apply_relu", _lib.ptr(z), z.stride(0), m, c, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(beta),
              _lib.ptr(y), ldy, _lib.stream(), nbytes=4 * m * (c + ldy), flops=3 * m * c)
    return y


def bn_running_update(mean, var, m: int, momentum: float, running_mean, running_var):
    """The momentum recurrence of ``running_mean`` / ``running_var`` in place, with the unbiased variance
    (t2h_bn_running_update)."""
    _lib.require_device(mean, var, running_mean, running_var, what="bn_running_update")
    c = mean.numel()
    _bn_rows_count(m, c)
    if not (running_mean.is_contiguous() and running_var.is_contiguous() and running_mean.numel() == c == running_var.numel()
            and running_mean.dtype == running_var.dtype == torch.float32):
        raise ValueError("bn_running_update: contiguous fp32 running statistics of the statistics' length expected")
    _lib.call("t2h_bn_running_update", _lib.ptr(mean), _lib.ptr(var), m, c, float(momentum), _lib.ptr(running_mean),
              _lib.ptr(running_var), _lib.stream(), nbytes=24 * c)
    # written behind torch's back: whatever is keyed on their version counters (the eval() fold) is stale
    torch.autograd.graph.increment_version((running_mean, running_var))
    return running_mean, running_var


def bn_bwd_reduce(gy, y, z, c: int, mean, rstd, relu: bool):
    """(dbeta, dgamma) [c]: the column sums of g and g * xhat, g = ``gy`` masked by ``y > 0`` when ``relu`` (t2h_bn_bwd_reduce)."""
    _bn_rows(gy, c, "bn_bwd_reduce gy"), _bn_rows(z, c, "bn_bwd_reduce z")
    if relu:
        _bn_rows(y, c, "bn_bwd_reduce y")
    m = z.shape[0]
    _bn_rows_count(m, c)
    dbeta, dgamma = (torch.empty(c, dtype=torch.float32, device=z.device) for _ in range(2))
    partial = _bn_partial(m, c, 2, z.device)
    _lib.call("t2h_bn_bwd_reduce", _lib.ptr(gy), gy.stride(0), _lib.ptr(y) if relu else None, y.stride(0) if relu else 0, _lib.ptr(z),
              z.stride(0), m, c, _lib.ptr(mean), _lib.ptr(rstd), int(bool(relu)), _lib.ptr(partial), _lib.ptr(dbeta), _lib.ptr(dgamma),
              _lib.stream(), nbytes=4 * m * c * (3 if relu else 2), flops=5 * m * c)
    return dbeta, dgamma


def bn_bwd_apply(gy, y, z, c: int, mean, rstd, gamma, dbeta, dgamma, relu: bool, gld: int = None) -> torch.Tensor:
    """dz [M, gld] = gamma * rstd * (g - dbeta / M - xhat * dgamma / M); columns c .. gld are zero (t2h_bn_bwd_apply)."""
    _bn_rows(gy, c, "bn_bwd_apply gy"), _bn_rows(z, c, "bn_bwd_apply z")
    if relu:
        _bn_rows(y, c, "bn_bwd_apply y")
    m = z.shape[0]
    _bn_rows_count(m, c)
    gld = c if gld is None else gld
    dz = torch.empty(m, gld, dtype=torch.float32, device=z.device)
    _lib.call("t2h_bn_bwd_apply", _lib.ptr(gy), gy.stride(0), _lib.ptr(y) if relu else None, y.stride(0) if relu else 0, _lib.ptr(z),
              z.stride(0), m, c, _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(gamma), _lib.ptr(dbeta), _lib.ptr(dgamma), int(bool(relu)),
              _lib.ptr(dz), gld, _lib.stream(), nbytes=4 * m * (c * (3 if relu else 2) + gld), flops=6 * m * c)
    return dz
