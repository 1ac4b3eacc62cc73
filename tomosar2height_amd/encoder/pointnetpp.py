"""PointNetPlusPlus (reference: tomosar2height/encoder/pointnetpp.py:16-173) on the MI355X path: inference, gradients of
every parameter in ``eval()`` (fine-tuning with frozen BatchNorm statistics), and -- opt-in -- training with batch statistics.

Constructor arguments, ``state_dict`` keys and shapes are the reference's (``sa{1,2,3}`` / ``fp{3,2,1}`` with ``mlp_convs.{k}`` and
``mlp_bns.{k}``, BatchNorm buffers and ``num_batches_tracked`` included, ``unet.*``), so a reference checkpoint loads with
``strict=True``.  The index work -- farthest point sampling, radius grouping, grouped max, 3-nearest-neighbour propagation --
runs on csrc/pnpp.hip (``pointops``); every 1 x 1 ``Conv2d`` / ``Conv1d`` + BatchNorm + ReLU layer is a rows x weight product on
the fp32 MFMA kernels (``mlp.linear_fwd_`` with ``relu_out``) with the BatchNorm running statistics folded into weight and
bias; rasterisation and the ALTO / plain U-Net are the modules the default encoder uses.

``eval()`` by default: ``forward`` under ``train()`` raises unless the encoder was built with ``batch_statistics=True`` (config:
``model.encoder_kwargs``), the opt-in switch for BatchNorm batch statistics (DESIGN.md sections 4.9 and 8).  With it, a stage
under ``train()`` runs ``_ChainBatchStats``: raw-weight products, the batch statistics of every layer's rows, their backward and
the running-average updates on csrc/pnpp.hip (``t2h_bn_*``); the switch is a plain attribute (no ``state_dict`` entry) and has no
effect in ``eval()``.
In ``eval()`` with gradients enabled and an encoder parameter (or an incoming feature) that requires one, the stages build an
autograd graph: the layers run on the same products forward (``_Chain``: ``linear_dgrad_`` / ``linear_wgrad_`` backward, the
ReLU masks fused into the data gradients), the grouped max, the grouped rows and the 3-NN propagation have their adjoints in
csrc/pnpp.hip, and the gradients of ``conv.weight``, ``conv.bias``, ``bn.weight`` and ``bn.bias`` follow from the fold's chain
rule; the running statistics and ``xyz`` get none.  The forward is bit-identical in both modes.  Under ``torch.no_grad()``, or
with nothing requiring a gradient, the cached fold is used and nothing is saved.

The reference's inference is itself random: ``farthest_point_sample`` starts from ``torch.randint`` (pointnetpp.py:232), once
for ``sa1`` and once for ``sa2``.  ``fps_start = None`` (default) does the same on the device, in that order -- reproducible
under ``torch.manual_seed``, but not the reference's draws, which come from the host generator.  An ``int`` or an int64 ``[B]``
tensor fixes the start of both levels (clamped to the level's point count); a pair ``(sa1, sa2)`` of those fixes each.
"""
from typing import Dict

import torch
import torch.nn as nn

from .. import _lib, mlp, ops, pointops
from ..tile import TileIndex
from .alto import UNet as Alto
from .unet import UNet


def _pad4(k: int) -> int:
    return (k + 3) // 4 * 4


class _FoldedLayers(nn.Module):
    """``mlp_convs`` / ``mlp_bns`` of one stage and their folded form: W' = W * s, b' = (b - mean) * s + beta with
    s = gamma / sqrt(var + eps), computed in float64 and rounded once; the first layer's W' is padded with zero columns to the
    row length of its input (a multiple of 4: 16-byte rows for the product kernels; K = 131 and 259 have no kernel otherwise).
    Cached per version of every tensor involved (``_lib.Derived``)."""

    def _make_layers(self, conv, bn, in_channel, widths):
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last = in_channel
        for out in widths:
            self.mlp_convs.append(conv(last, out, 1))
            self.mlp_bns.append(bn(out))
            last = out
        self.__dict__["_fold"] = _lib.Derived()
        self.batch_statistics = False      # train(): BatchNorm batch statistics (``_ChainBatchStats``); a plain attribute, no state

    def _refuse_training(self, name):
        """``train()`` without the switch: the stage has no batch statistics to offer."""
        if self.training and not self.batch_statistics:
            raise NotImplementedError(f"{name} runs in eval() only: BatchNorm batch statistics are not built by default; "
                                      f"construct PointNetPlusPlus(batch_statistics=True) (config: model.encoder_kwargs), or set "
                                      f"``stage.batch_statistics = True``, to train with them")

    def wants_batch_stats(self) -> bool:
        return self.training and self.batch_statistics

    def folded(self, graph=False):
        """[(W', b')] of the layers.  By default without a graph, cached; ``graph``: the same float64 torch operations under
        autograd, uncached -- the same bytes, with the chain rule to ``conv.weight``, ``conv.bias``, ``bn.weight`` and ``bn.bias``
        (the running statistics are constants)."""
        pairs = list(zip(self.mlp_convs, self.mlp_bns))

        def fold():
            layers = []
            for conv, bn in pairs:
                _lib.require_device(conv.weight, what="PointNetPlusPlus layer")
                s = bn.weight.double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
                w = conv.weight.reshape(conv.weight.shape[0], -1).double() * s[:, None]
                b = (conv.bias.double() - bn.running_mean.detach().double()) * s + bn.bias.double()
                k = w.shape[1]
                layers.append((torch.nn.functional.pad(w.float(), (0, _pad4(k) - k)), b.float()))
            return layers

        if graph:
            return fold()
        sources = [t for conv, bn in pairs for t in (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)]
        return self.__dict__["_fold"].get("layers", sources, fold)          # (``Derived.get`` fills under ``no_grad``)

    def wants_graph(self, *features) -> bool:
        """True when this stage has to build an autograd graph: gradients are enabled and a parameter of its layers, or a
        feature tensor it is handed, requires one."""
        if not torch.is_grad_enabled():
            return False
        return any(t is not None and t.requires_grad for t in features) or any(
            p.requires_grad for m in (self.mlp_convs, self.mlp_bns) for p in m.parameters())

    def _chain(self, rows, nsample=0, graph=False):
        """relu(bn(conv(.))) of every layer over [M, K] rows; ``nsample`` > 0: followed by the max over each group of
        ``nsample`` consecutive rows.  ``graph``: as one autograd node (``_Chain``)."""
        if graph or self.wants_batch_stats():
            widths = [conv.weight.shape[0] for conv in self.mlp_convs]
            if any(w % 4 for w in widths):
                raise NotImplementedError(f"PointNetPlusPlus gradients need layer widths that are multiples of 4 (16-byte rows of "
                                          f"the data- and weight-gradient products), got {widths}; inference takes any width")
        if self.wants_batch_stats():
            return self._chain_batch_stats(rows, nsample)
        if graph:
            return _Chain.apply(rows, nsample, *[t for wb in self.folded(graph=True) for t in wb])
        with torch.no_grad():
            for w, b in self.folded():
                y = torch.empty(rows.shape[0], w.shape[0], dtype=torch.float32, device=rows.device)
                mlp.linear_fwd_(rows, w, b, y, relu_out=True)
                rows = y
            if nsample:
                rows = pointops.group_max_rows(rows, nsample)
        return rows


    def _chain_batch_stats(self, rows, nsample):
        """The training-mode chain: per layer the raw weight (reshaped to [C, K], zero-padded to ``_pad4(K)`` columns: torch
        operations under autograd, so ``dW`` reaches ``conv.weight`` through them), its bias, gamma and beta go into ONE node;
        the running statistics are updated in place inside it, gradients enabled or not."""
        args, bns = [], []
        for conv, bn in zip(self.mlp_convs, self.mlp_bns):
            _lib.require_device(conv.weight, what="PointNetPlusPlus layer")
            if bn.momentum is None or not bn.track_running_stats or not bn.affine:
                raise NotImplementedError("PointNetPlusPlus batch statistics: affine BatchNorm with running statistics and a fixed "
                                          "momentum (the reference's layers) only")
            w = conv.weight.reshape(conv.weight.shape[0], -1)
            k = w.shape[1]
            args += [torch.nn.functional.pad(w, (0, _pad4(k) - k)), conv.bias, bn.weight, bn.bias]
            bns.append(bn)
        return _ChainBatchStats.apply(rows, nsample, bns, *args)


class _ChainBatchStats(torch.autograd.Function):
    """The layers of a stage under ``train()`` with ``batch_statistics``: per layer z = x W^T + b (``linear_fwd_``, the raw
    weight, no fold), the batch statistics of z's columns (``t2h_bn_col_stats``), y = relu(z * s + t) (``t2h_bn_apply_relu``) and
    the momentum update of the layer's running statistics (``t2h_bn_running_update``, ``num_batches_tracked += 1``); then
    (``nsample`` > 0) the max over each group of rows.  One node.  Backward, per layer from the last: the gradient of y comes from
    ``t2h_group_max_bwd(relu=1)`` (set abstraction; the mask is then applied) or is the incoming one (the mask is applied by
    ``t2h_bn_bwd_reduce`` / ``t2h_bn_bwd_apply`` with ``relu=1``, as for every inner layer); ``bwd_reduce`` gives dbeta and dgamma,
    ``bwd_apply`` dz, ``linear_wgrad_`` dW and db, ``linear_dgrad_`` (no mask) the gradient of the layer's input."""

    @staticmethod
    def forward(ctx, rows, nsample, bns, *params):
        n = len(bns)
        xs, zs, ys, stats = [rows], [], [], []
        for k, bn in enumerate(bns):
            w, b, gamma, beta = params[4 * k:4 * k + 4]
            c = w.shape[0]
            z = torch.empty(xs[-1].shape[0], c, dtype=torch.float32, device=rows.device)
            mlp.linear_fwd_(xs[-1], w, b, z, relu_out=False)
            mean, var, rstd = pointops.bn_col_stats(z, c, bn.eps)
            y = pointops.bn_apply_relu(z, c, mean, rstd, gamma, beta)
            pointops.bn_running_update(mean, var, z.shape[0], bn.momentum, bn.running_mean, bn.running_var)
            bn.num_batches_tracked.add_(1)
            zs.append(z), ys.append(y), stats.extend((mean, rstd)), xs.append(y)
        out = pointops._group_max_rows(ys[-1], nsample, ys[-1].shape[1]) if nsample else ys[-1]
        ctx.nsample, ctx.layers = nsample, n
        ctx.save_for_backward(*xs[:n], *zs, *ys, *stats, *params[0::4], *params[2::4], *((out,) if nsample else ()))
        return out

    @staticmethod
    def backward(ctx, gout):
        n = ctx.layers
        sv = ctx.saved_tensors
        xs, zs, ys, stats, ws, gammas = sv[:n], sv[n:2 * n], sv[2 * n:3 * n], sv[3 * n:5 * n], sv[5 * n:6 * n], sv[6 * n:7 * n]
        g = gout.contiguous()
        relu = True
        if ctx.nsample:
            g, relu = pointops.group_max_bwd(ys[n - 1], sv[-1], g, ctx.nsample, relu=True), False
        grads = [None] * (4 * n)
        for k in range(n - 1, -1, -1):
            x, z, y, w, gamma, (mean, rstd) = xs[k], zs[k], ys[k], ws[k], gammas[k], stats[2 * k:2 * k + 2]
            c = w.shape[0]
            dbeta, dgamma = pointops.bn_bwd_reduce(g, y, z, c, mean, rstd, relu)
            dz = pointops.bn_bwd_apply(g, y, z, c, mean, rstd, gamma, dbeta, dgamma, relu)
            if ctx.needs_input_grad[3 + 4 * k] or ctx.needs_input_grad[4 + 4 * k]:
                dw, db = torch.empty_like(w), torch.empty(c, dtype=torch.float32, device=w.device)
                mlp.linear_wgrad_(dz, x, dw, db)
                grads[4 * k], grads[4 * k + 1] = dw, db
            grads[4 * k + 2], grads[4 * k + 3] = dgamma, dbeta
            if k > 0 or ctx.needs_input_grad[0]:
                g, relu = mlp.linear_dgrad_(dz, w, torch.empty_like(x), mask=None), True
        return (g if ctx.needs_input_grad[0] else None, None, None, *grads)


class _Chain(torch.autograd.Function):
    """The layers of a stage, y_k = relu(y_{k-1} W'_k^T + b'_k), and (``nsample`` > 0) the max over each group of rows, as one
    node.  Backward: the gradient of the last pre-activation comes from ``t2h_group_max_bwd(relu=1)`` (set abstraction: max
    and ReLU mask in one pass) or ``t2h_relu_mask`` (propagation); then per layer ``linear_wgrad_`` over the padded rows and
    ``linear_dgrad_`` with the layer's input as mask -- the ReLU mask of layer k - 1 is the ``x > 0`` mask of layer k's data
    gradient.  The first layer's input is data or another node's output: no mask, and no product unless it wants a gradient."""

    @staticmethod
    def forward(ctx, rows, nsample, *wb):
        acts = [rows]
        for w, b in zip(wb[0::2], wb[1::2]):
            y = torch.empty(rows.shape[0], w.shape[0], dtype=torch.float32, device=rows.device)
            mlp.linear_fwd_(acts[-1], w, b, y, relu_out=True)
            acts.append(y)
        out = pointops._group_max_rows(acts[-1], nsample, acts[-1].shape[1]) if nsample else acts[-1]
        ctx.nsample, ctx.layers = nsample, len(wb) // 2
        ctx.save_for_backward(*acts, *wb[0::2], *((out,) if nsample else ()))
        return out

    @staticmethod
    def backward(ctx, gout):
        n = ctx.layers
        saved = ctx.saved_tensors
        acts, ws = saved[:n + 1], saved[n + 1:2 * n + 1]
        gout = gout.contiguous()
        if ctx.nsample:
            g = pointops.group_max_bwd(acts[n], saved[-1], gout, ctx.nsample, relu=True)
        else:
            g = torch.empty_like(gout)
            _lib.call("t2h_relu_mask", _lib.ptr(gout), _lib.ptr(acts[n]), _lib.ptr(g), gout.numel(), _lib.stream(),
                      nbytes=12 * gout.numel())
        grads = [None] * (2 * n)
        for k in range(n - 1, -1, -1):
            x, w = acts[k], ws[k]
            if ctx.needs_input_grad[2 + 2 * k] or ctx.needs_input_grad[3 + 2 * k]:
                dw, db = torch.empty_like(w), torch.empty(w.shape[0], dtype=torch.float32, device=w.device)
                mlp.linear_wgrad_(g, x, dw, db)
                grads[2 * k], grads[2 * k + 1] = dw, db
            if k > 0 or ctx.needs_input_grad[0]:
                g = mlp.linear_dgrad_(g, w, torch.empty_like(x), mask=x if k > 0 else None)
        return (g if ctx.needs_input_grad[0] else None, None, *grads)


class PointNetSetAbstraction(_FoldedLayers):
    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all):
        super().__init__()
        self.npoint, self.radius, self.nsample, self.group_all = npoint, radius, nsample, group_all
        self._make_layers(nn.Conv2d, nn.BatchNorm2d, in_channel, mlp)

    def forward_rows(self, xyz, points, start=None, trace=None):
        """Point-major form of pointnetpp.py:31-57: ``xyz`` [B, N, 3], ``points`` [B, N, D] or None -> new_xyz [B, S, 3],
        new_points [B, S, D'].  ``trace``: a dict that receives ``fps_idx`` and the ball ``idx``."""
        self._refuse_training("PointNetSetAbstraction")
        pointops._cloud(xyz, "PointNetSetAbstraction xyz")
        b, n, _ = xyz.shape
        d = 0 if points is None else points.shape[2]
        ld = _pad4(3 + d)
        graph = self.wants_graph(points)
        with torch.no_grad():
            if self.group_all:                                             # pointnetpp.py:303-320: a view and a concatenation
                new_xyz = torch.zeros(b, 1, 3, dtype=torch.float32, device=xyz.device)
                nsample = n
            else:
                fps_idx = pointops.farthest_point_sample(xyz, self.npoint, start)
                new_xyz = pointops.index_points(xyz, fps_idx).contiguous()
                idx = pointops.query_ball_point(self.radius, self.nsample, xyz, new_xyz)
                nsample = self.nsample
                if trace is not None:
                    trace["fps_idx"], trace["idx"] = fps_idx, idx
        with torch.set_grad_enabled(graph):
            if self.group_all:                                             # (its backward: a column slice)
                parts = [xyz.reshape(b * n, 3)] + ([] if points is None else [points.reshape(b * n, d)])
                if ld > 3 + d:
                    parts.append(torch.zeros(b * n, ld - 3 - d, dtype=torch.float32, device=xyz.device))
                rows = torch.cat(parts, dim=1)
            else:
                rows = pointops.group_rows(xyz, new_xyz, points, idx, ld)
            new_points = self._chain(rows, nsample, graph)
        return new_xyz, new_points.view(b, -1, new_points.shape[1])

    def forward(self, xyz, points, start=None):
        """The reference's layout: ``xyz`` [B, 3, N], ``points`` [B, D, N] -> new_xyz [B, 3, S], new_points [B, D', S]."""
        new_xyz, new_points = self.forward_rows(xyz.permute(0, 2, 1).contiguous(),
                                                None if points is None else points.permute(0, 2, 1).contiguous(), start)
        return new_xyz.permute(0, 2, 1), new_points.permute(0, 2, 1)


class _RowConstant(torch.autograd.Function):
    """Identity whose gradient is exactly zero: the one source row of a propagation over ONE cloud (``fp3`` at B = 1, the batch a
    ``Trainer`` tile is).  The ``repeat`` branch copies it to every target, so in z = [points1 | row] W^T + b of the first layer
    it is a per-channel constant over all M rows, which the batch statistics remove (z - mean): the output does not depend on
    it, and its exact gradient -- and with it every gradient of ``sa3`` -- is 0.  The chain rule through the rounded kernels
    would hand back rounding noise in its place (sum_r dz W, with sum_r dz = 0 only in exact arithmetic); this returns the
    exact value, so ``sa3``'s parameters get zero gradients (not ``None``: weight decay still sees them).  With two or more
    clouds the row is a constant per cloud only and the ordinary adjoint runs."""

    @staticmethod
    def forward(ctx, points2):
        return points2.view_as(points2)

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


class PointNetFeaturePropagation(_FoldedLayers):
    def __init__(self, in_channel, mlp):
        super().__init__()
        self._make_layers(nn.Conv1d, nn.BatchNorm1d, in_channel, mlp)

    def forward_rows(self, xyz1, xyz2, points1, points2, trace=None):
        """Point-major form of pointnetpp.py:70-109: targets ``xyz1`` [B, N, 3] (features ``points1`` [B, N, D1] or None), sources
        ``xyz2`` [B, S, 3] with ``points2`` [B, S, D2] -> [B, N, D'].  ``trace`` receives the 3-NN ``idx`` and ``weight``."""
        self._refuse_training("PointNetFeaturePropagation")
        b, n, _ = xyz1.shape
        graph = self.wants_graph(points1, points2)
        with torch.set_grad_enabled(graph):
            if graph and self.wants_batch_stats() and b == 1 and xyz2.shape[1] == 1 and points2.requires_grad:
                points2 = _RowConstant.apply(points2)
            interp, idx, weight = pointops.three_nn_interpolate(xyz1, xyz2, points2)
            if trace is not None:
                trace["idx"], trace["weight"], trace["interpolated"] = idx, weight, interp
            rows = interp.view(b * n, -1)
            if points1 is not None:
                rows = torch.cat([points1.reshape(b * n, -1), rows], dim=1)
            out = self._chain(rows, 0, graph)
        return out.view(b, n, -1)

    def forward(self, xyz1, xyz2, points1, points2):
        """The reference's layout: [B, C, N] tensors in, [B, D', N] out."""
        pm = lambda t: None if t is None else t.permute(0, 2, 1).contiguous()
        return self.forward_rows(pm(xyz1), pm(xyz2), pm(points1), pm(points2)).permute(0, 2, 1)


class PointNetPlusPlus(nn.Module):
    def __init__(self, feature_dim=128, dim=3, hidden_dim=None, scatter_type=None, unet_type="alto", unet_kwargs=None,
                 plane_resolution=None, batch_statistics: bool = False):
        super().__init__()
        self.sa1 = PointNetSetAbstraction(npoint=512, radius=0.2, nsample=32, in_channel=dim + 3, mlp=[64, 64, 128], group_all=False)
        self.sa2 = PointNetSetAbstraction(npoint=128, radius=0.4, nsample=64, in_channel=128 + 3, mlp=[128, 128, 256], group_all=False)
        self.sa3 = PointNetSetAbstraction(npoint=None, radius=None, nsample=None, in_channel=256 + 3, mlp=[256, 512, 1024], group_all=True)
        self.fp3 = PointNetFeaturePropagation(in_channel=1280, mlp=[256, 256])
        self.fp2 = PointNetFeaturePropagation(in_channel=384, mlp=[256, 128])
        self.fp1 = PointNetFeaturePropagation(in_channel=128, mlp=[128, 128, feature_dim])
        self.unet_type = unet_type
        self.feature_dim = feature_dim
        if unet_type == "unet":
            self.unet = UNet(feature_dim, in_channels=feature_dim, **(unet_kwargs or {}))
        elif unet_type == "alto":
            self.unet = Alto(feature_dim, in_channels=feature_dim, **(unet_kwargs or {}))
        else:
            raise ValueError(f"Unknown unet_type: {unet_type}")
        self.reso_plane = plane_resolution
        self.channels_last = False
        self.fps_start = None          # see the module docstring
        self.batch_statistics = bool(batch_statistics)
        for stage in (self.sa1, self.sa2, self.sa3, self.fp3, self.fp2, self.fp1):
            stage.batch_statistics = self.batch_statistics

    def set_channels_last(self, flag: bool):
        """Keep the grid side in channels_last memory so planes need no NCHW<->NHWC copies."""
        self.channels_last = bool(flag)
        if hasattr(self.unet, "set_channels_last"):
            self.unet.set_channels_last(flag)

    def _starts(self):
        s = self.fps_start
        return tuple(s) if isinstance(s, (tuple, list)) else (s, s)

    def point_features(self, xyz: torch.Tensor, targets: torch.Tensor = None, trace: dict = None) -> torch.Tensor:
        """pointnetpp.py:152-163: ``xyz`` [B, N, dim] -> per-point features [B, N', feature_dim] at ``targets`` [B, N', 3]
        (default: the cloud itself, in its own order).  The last propagation is independent per target, so the encoder asks
        for the features in the cell-sorted order of its tile index.  ``trace``: a dict that receives every level's tensors."""
        tr = (lambda k: trace.setdefault(k, {})) if trace is not None else (lambda k: None)
        l0_xyz = xyz[:, :, :3].contiguous()
        s1, s2 = self._starts()
        l1_xyz, l1_points = self.sa1.forward_rows(l0_xyz, xyz, s1, tr("sa1"))       # (the order of the draws: sa1, then sa2)
        l2_xyz, l2_points = self.sa2.forward_rows(l1_xyz, l1_points, s2, tr("sa2"))
        l3_xyz, l3_points = self.sa3.forward_rows(l2_xyz, l2_points)
        l2_points = self.fp3.forward_rows(l2_xyz, l3_xyz, l2_points, l3_points, tr("fp3"))
        l1_points = self.fp2.forward_rows(l1_xyz, l2_xyz, l1_points, l2_points, tr("fp2"))
        l0_points = self.fp1.forward_rows(l0_xyz if targets is None else targets, l1_xyz, None, l1_points, tr("fp1"))
        if trace is not None:
            trace.update(l1_points=l1_points, l2_points=l2_points, l3_points=l3_points, l0_points=l0_points)
        return l0_points

    def forward(self, xyz: torch.Tensor, trace: dict = None) -> Dict[str, torch.Tensor]:
        """``xyz`` [B, N, dim] in [0, 1) -> ``{'xy': [B, feature_dim, R, R]}``."""
        if self.training and not self.batch_statistics:
            raise NotImplementedError("PointNetPlusPlus runs in eval() only by default: training needs BatchNorm batch statistics, "
                                      "which are opt-in -- PointNetPlusPlus(batch_statistics=True) (config: model.encoder_kwargs); "
                                      "gradients of every parameter are also available in eval() (frozen statistics)")
        pointops._cloud(xyz, "PointNetPlusPlus", cols=None)
        xyz = xyz.contiguous()
        b, n, dim = xyz.shape
        tile = TileIndex(xyz, self.reso_plane)
        targets = tile.pts.view(b, n, dim)[:, :, :3].contiguous()
        net = self.point_features(xyz, targets, trace).view(b * n, self.feature_dim)        # rows in the tile's sorted order
        if trace is not None:
            trace["tile"] = tile
        if self.unet_type == "alto":
            plane, net = ops.rasterise_mean_thru(tile, net, self.reso_plane, self.channels_last)     # pointnetpp.py:166
            out = {"xy": self.unet.forward_sorted(tile, plane, net)}                                 # pointnetpp.py:171
        else:
            plane = ops.rasterise_mean(tile, net, self.reso_plane, self.channels_last)
            out = {"xy": self.unet(plane)}
        if trace is not None:
            trace["plane"] = plane
        return out
