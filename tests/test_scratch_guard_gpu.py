"""-m gpu: every launch that takes scratch, run over poisoned, guarded workspaces (tests/scratch_guard.py).

One table, CASES.  A row names the package-level call (so the package's own ``ws_bytes`` / ``workspace`` pairing is what runs), the
shape, the fill of its raw workspaces and the sign each size query must have at that shape (checked on the CPU as well, by
test_scratch_guard_cpu.py, which also fails when a ``T2H_API size_t`` query of the sources has no row where it is positive).

Per row: (1) a clean run, compared with float64 where the row carries a ``check`` (the operator's own reference: the C oracle,
torch's float64 operator, tests/*_ref.py) -- rows without one are whole-path rows whose float64 comparison lives in the module
named in ``why``; (2) a recording run of the same calls on ANOTHER input of the same shape, then the run under the row's fill,
floating allocations NaN, integer allocations stale from the recording run: every output and gradient bit-identical to the
clean run, every guard band intact; (3) the size queries have the tabled sign.

Fill rule: "nan" only where reading the source shows the workspace holds floating data only; "stale" where it holds anything
used as an index, offset, count or loop bound -- the ``why`` column gives the line the choice rests on.  No row is in the
atomic mode: no package-level call of this table reaches ``t2h_sample_bwd_atomic`` (ops._sample_bwd takes the gather, the
per-cell partials or the transposed matrix).

``_sizing_cases``: the tile builds' workspaces and the split-weight buffers (both ``_lib.workspace``s, so banded) at the smallest
shapes where their size queries can be wrong, each against the reference the suite already uses for the operation; the batched
refresh of 25 split buffers has a test of its own at the end.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from detinit import det_init_, synth_cloud
from scratch_guard import _hit, guarded_scratch

pytestmark = pytest.mark.gpu
D = torch.float64


def _dev():
    return torch.device("cuda:0")


def _cl(t):
    return t.to(_dev()).contiguous(memory_format=torch.channels_last)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close(got, want, tol, what=""):
    want = want.detach().to(D).cpu()
    scale = want.abs().max().item() + 1e-30
    err = (got.detach().to(D).cpu() - want).abs().max().item()
    assert tuple(got.shape) == tuple(want.shape) and err <= tol * scale, (what, err / scale)


class Case:
    def __init__(self, id, call, run, fill, why, queries, check=None, setup=None, sites=(), nan_sites=(), loose=False):
        """``run(seed) -> {name: tensor}``; ``check(outputs, seed)`` the float64 comparison of the clean run; ``setup``: a dict of
        ``module.ATTR -> value`` switches set for the row; ``queries``: (size query, its arguments, ">0" | "==0")."""
        self.id, self.call, self.run, self.fill, self.why, self.queries = id, call, run, fill, why, queries
        self.check, self.setup, self.sites = check, setup or {}, sites      # sites: call sites whose workspaces the row must reach
        # nan_sites: call sites of float-only workspaces of a stale row (they get NaN); loose: the query arguments depend on the
        # data (component count, hull size), so the handed-out size is not compared with the tabled query
        self.nan_sites, self.loose = nan_sites, loose


# ------------------------------------------------------------------------------------------------ point <-> grid
def _point_grid(n, reso, c, batch=1, ragged=None):
    def tile_of(seed):
        from tomosar2height_amd.tile import TileIndex
        if ragged:
            return TileIndex([synth_cloud(k, seed=seed + i).to(_dev()) for i, k in enumerate(ragged)], reso), None
        cloud = synth_cloud(n, seed=seed, batch=batch)
        return TileIndex(cloud.to(_dev()), reso), cloud

    def run(seed):
        from tomosar2height_amd import ops
        t, _ = tile_of(seed)
        g = _gen(seed)
        rows = t.n_points
        f = torch.randn(rows, c, generator=g).to(_dev()).requires_grad_(True)
        plane = ops.rasterise_mean(t, f, reso)
        plane.backward(torch.randn(plane.shape, generator=g).to(_dev()))
        p = torch.randn(t.B, c, reso, reso, generator=g).to(_dev()).requires_grad_(True)
        out = ops.sample_plane(t, p)
        out.backward(torch.randn(rows, c, generator=g).to(_dev()))
        return {"plane": plane.detach(), "dfeat": f.grad, "sampled": out.detach(), "dplane": p.grad,
                "perm": t.perm, "cell": t.cell, "off0": t.off0}

    def check(o, seed):
        from oracle import c_oracle
        if ragged:
            return _check_ragged(o, seed)
        t, cloud = tile_of(seed)
        g = _gen(seed)
        feat = torch.randn(batch * n, c, generator=g)
        gplane = torch.randn(batch, c, reso, reso, generator=g)
        pl = torch.randn(batch, c, reso, reso, generator=g)
        gs = torch.randn(batch * n, c, generator=g)
        idx = c_oracle.coordinate2index(cloud.numpy(), reso)
        unsorted = t.unsort_rows(feat.to(_dev())).cpu().reshape(batch, n, c).numpy()      # run() fed SORTED rows
        np.testing.assert_allclose(o["plane"].cpu().numpy(), c_oracle.scatter_mean_fwd(unsorted, idx, reso), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(t.unsort_rows(o["dfeat"]).cpu().numpy().reshape(batch, n, c),
                                   c_oracle.scatter_mean_bwd(gplane.numpy(), idx, n), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(t.unsort_rows(o["sampled"]).cpu().numpy().reshape(batch, n, c),
                                   c_oracle.grid_sample_fwd(pl.numpy(), cloud.numpy()), rtol=1e-5, atol=1e-6)
        gs_un = t.unsort_rows(gs.to(_dev())).cpu().reshape(batch, n, c).numpy()
        want = c_oracle.grid_sample_bwd(gs_un, cloud.numpy(), reso, reso)
        np.testing.assert_allclose(o["dplane"].cpu().numpy(), want, rtol=1e-4, atol=1e-5 * (np.abs(want).max() + 1e-6))
    def _check_ragged(o, seed):
        """torch's own float64 operators per tile on the sorted rows (the form test_hip_deferred.py uses): index_add / count for
        the mean, F.grid_sample (bilinear, border, align_corners) and its autograd for the sample."""
        t, _ = tile_of(seed)
        g = _gen(seed)
        rows = t.n_points
        feat = torch.randn(rows, c, generator=g).to(_dev()).to(D)
        gplane = torch.randn(t.B, c, reso, reso, generator=g).to(_dev()).to(D)
        pl = torch.randn(t.B, c, reso, reso, generator=g).to(_dev()).to(D).requires_grad_(True)
        gs = torch.randn(rows, c, generator=g).to(_dev()).to(D)
        xy = t.pts[:, :2].to(D)
        b = torch.repeat_interleave(torch.arange(t.B, device=_dev()), torch.tensor(t.counts, device=_dev()))
        cell = (b * reso + (t.pts[:, 1] * reso).long()) * reso + (t.pts[:, 0] * reso).long()
        cnt = torch.zeros(t.B * reso * reso, dtype=D, device=_dev()).index_add_(0, cell, torch.ones(rows, dtype=D, device=_dev()))
        mean = torch.zeros(t.B * reso * reso, c, dtype=D, device=_dev()).index_add_(0, cell, feat) / cnt.clamp_min(1)[:, None]
        _close(o["plane"], mean.reshape(t.B, reso, reso, c).permute(0, 3, 1, 2), 1e-5, "plane")
        gp = gplane.permute(0, 2, 3, 1).reshape(-1, c)
        _close(o["dfeat"], gp[cell] / cnt[cell][:, None], 1e-6, "dfeat")
        outs = []
        for k in range(t.B):
            lo, hi = t.starts[k], t.starts[k + 1]
            vgrid = (2.0 * xy[lo:hi] - 1.0).reshape(1, hi - lo, 1, 2)
            outs.append(F.grid_sample(pl[k:k + 1], vgrid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, :, 0].t())
        out = torch.cat(outs, 0)
        out.backward(gs)
        _close(o["sampled"], out, 1e-5, "sampled")
        _close(o["dplane"], pl.grad, 1e-4, "dplane")
    return run, check


def _pg_case(id, n, reso, c, batch, seg, smp, adjoint, ragged=None):
    run, check = _point_grid(n, reso, c, batch, ragged)
    nb = reso.bit_length() - 1
    nq = -sum(ragged) if ragged else n
    b = len(ragged) if ragged else batch
    q = [("t2h_segmean_workspace_bytes", (b, nq, nb, 0, c), seg), ("t2h_sample_bwd_workspace_bytes", (b, nq, nb, 0, c), smp)]
    if ragged:
        q.append(("t2h_tile_ragged_workspace_bytes", (b, sum(ragged), max(ragged), nb), ">0"))
    else:
        q.append(("t2h_tile_workspace_bytes", (b, n, nb), ">0"))
    if adjoint:
        q.append(("t2h_sample_adjoint_offsets_len", (b, nb, 0), ">0"))
    return Case(id, "ops.rasterise_mean / ops.sample_plane, forward and backward", run, "stale",
                "the tile build's sort keys and histograms are TileIndex's own integer buffers (tile.py:58, :99); the coarse-walk "
                "partials (ops.py:222, :281) are floats but share the row's one fill", q, check,
                {"ops.SAMPLE_ADJOINT": adjoint}, nan_sites=("ops.py",))


# ------------------------------------------------------------------------------------------------ convolutions
def _conv3x3(b, h, w, cin, cout):
    def data(seed):
        g = _gen(seed)
        return (torch.randn(b, cin, h, w, generator=g), torch.randn(cout, cin, 3, 3, generator=g) * 0.1, torch.randn(cout, generator=g),
                torch.randn(b, cout, h, w, generator=g))

    def run(seed):
        from tomosar2height_amd import grid
        x, wt, bias, gy = data(seed)
        xd, wd, gyd = _cl(x), _cl(wt), _cl(gy)
        y = grid._empty_cl(b, cout, h, w, _dev())
        grid.conv3x3_fwd_(xd, wd, bias.to(_dev()), y, relu=True)
        dx = grid._empty_cl(b, cin, h, w, _dev())
        grid.conv3x3_dgrad_(gyd, wd, dx)
        dw = torch.empty(cout, cin, 3, 3, device=_dev()).contiguous(memory_format=torch.channels_last)
        db = torch.empty(cout, device=_dev())
        grid.conv3x3_wgrad_(gyd, xd, dw, db)
        return {"y": y, "dx": dx, "dw": dw, "db": db}

    def check(o, seed):
        x, wt, bias, gy = (t.double() for t in data(seed))
        x.requires_grad_(True), wt.requires_grad_(True), bias.requires_grad_(True)
        want = F.conv2d(x, wt, bias, padding=1)
        want.backward(gy)
        for k, ref in (("y", F.relu(want)), ("dx", x.grad), ("dw", wt.grad), ("db", bias.grad)):
            _close(o[k], ref, 2e-5, k)                  # test_hip_conv.py: 2e-5 of the max-norm, fp32 and split kernels alike
    return run, check


def _conv_case(b, h, w, cin, cout, precision, fwd, dgrad, wgrad, weights=None):
    run, check = _conv3x3(b, h, w, cin, cout)
    s = (b, h, w, cin, cout)
    pre = "t2h_conv3x3_" if precision == "fp32" else "t2h_conv3x3_bx3_"
    q = [(pre + "fwd_workspace_bytes", s, fwd), (pre + "dgrad_workspace_bytes", s, dgrad), (pre + "wgrad_workspace_bytes", s, wgrad)]
    if weights:
        q.append((weights, (cin, cout), ">0"))
    return Case(f"conv3x3-{precision}-{'x'.join(map(str, s))}", "grid.conv3x3_fwd_ / conv3x3_dgrad_ / conv3x3_wgrad_", run, "nan",
                "split-reduction slabs of float partial sums only (conv.hip:547-600, conv_bx3.hip:1137-1240); the split-weight "
                "buffer (grid.py:227) is a raw workspace of packed 16-bit planes, never an index", q, check,
                {"grid.CONV_PRECISION": precision, "grid.BX3_MIN_PIXELS": 0, "grid.BX3_WGRAD": True})


def _upconv(b, h, w, cin, cout):
    def mods(seed):
        torch.manual_seed(seed)
        conv = torch.nn.ConvTranspose2d(cin, cout, 2, stride=2)
        g = _gen(seed)
        return conv, torch.randn(b, cin, h, w, generator=g), torch.randn(b, cout, 2 * h, 2 * w, generator=g)

    def run(seed):
        from tomosar2height_amd import grid
        conv, x, gout = mods(seed)
        conv = conv.to(_dev()).to(memory_format=torch.channels_last)
        xg = _cl(x).requires_grad_(True)
        y = grid.upconv2x2(xg, conv)
        assert type(y.grad_fn).__name__ == "_UpConv2x2Backward"
        y.backward(_cl(gout))
        return {"y": y.detach(), "dx": xg.grad, "dw": conv.weight.grad, "db": conv.bias.grad}

    def check(o, seed):
        conv, x, gout = mods(seed)
        conv, x = conv.double(), x.double().requires_grad_(True)
        y = conv(x)
        y.backward(gout.double())
        for k, ref in (("y", y), ("dx", x.grad), ("dw", conv.weight.grad), ("db", conv.bias.grad)):
            _close(o[k], ref, 2e-5, k)
    return run, check


def _upconv_case(b, h, w, cin, cout, precision, dgrad, wgrad, weights=None):
    run, check = _upconv(b, h, w, cin, cout)
    s = (b, h, w, cin, cout)
    pre = "t2h_upconv2x2_" if precision == "fp32" else "t2h_upconv2x2_bx3_"
    q = [(pre + "dgrad_workspace_bytes", s, dgrad), (pre + "wgrad_workspace_bytes", s, wgrad)]
    if weights:
        q.append((weights, (cin, 4 * cout), ">0"))
    return Case(f"upconv2x2-{precision}-{'x'.join(map(str, s))}", "grid.upconv2x2 forward and backward", run, "nan",
                "float partial sums of the split reduction only (conv.hip:642-700, conv_bx3.hip:1366-1440)", q, check,
                {"grid.CONV_PRECISION": precision, "grid.BX3_MIN_PIXELS": 0, "grid.UPCONV_BX3": True})


def _module_conv(kind, b, h, w, cin, cout):
    """conv_bias_act on the small-Cin kernels (kind 'small'), conv1x1 on the GEMM kernels ('1x1'), head1x1 ('head')."""
    def mods(seed):
        torch.manual_seed(seed)
        conv = torch.nn.Conv2d(cin, cout, 3 if kind == "small" else 1, padding=1 if kind == "small" else 0)
        g = _gen(seed)
        return conv, torch.randn(b, cin, h, w, generator=g), torch.randn(b, cout, h, w, generator=g)

    def run(seed):
        from tomosar2height_amd import grid
        conv, x, gy = mods(seed)
        conv = conv.to(_dev())
        if kind == "small":
            conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
        xg = _cl(x).requires_grad_(True)
        if kind == "small":
            assert grid.conv3x3_small_supported(xg, conv)
            y = grid.conv_bias_act(xg, conv, relu=True)
        elif kind == "1x1":
            y = grid.conv1x1(xg, conv)
        else:
            y = grid.head1x1([xg], conv)
            assert type(y.grad_fn).__name__ == "_Head1x1Backward"
        y.backward(_cl(gy))
        return {"y": y.detach(), "dx": xg.grad, "dw": conv.weight.grad, "db": conv.bias.grad}

    def check(o, seed):
        conv, x, gy = mods(seed)
        conv, x = conv.double(), x.double().requires_grad_(True)
        y = torch.relu(conv(x)) if kind == "small" else conv(x)
        y.backward(gy.double())
        for k, ref in (("y", y), ("dx", x.grad), ("dw", conv.weight.grad), ("db", conv.bias.grad)):
            _close(o[k], ref, 2e-5, k)
    return run, check


def _bias_relu(b, h, w, c):
    def run(seed):
        from tomosar2height_amd import _lib, grid
        torch.manual_seed(seed)
        conv = torch.nn.Conv2d(c, c, 5, padding=2).to(_dev())
        g = _gen(seed)
        x = torch.randn(b, c, h, w, generator=g).to(_dev()).requires_grad_(True)
        with _lib.allow_library_fallback(True):
            y = grid.conv_bias_act(x, conv, relu=True)
            assert type(y.grad_fn).__name__ == "_ConvBiasActBackward"
            y.backward(torch.randn(b, c, h, w, generator=g).to(_dev()))
        return {"y": y.detach(), "dx": x.grad, "dw": conv.weight.grad, "db": conv.bias.grad}

    def check(o, seed):
        torch.manual_seed(seed)
        conv = torch.nn.Conv2d(c, c, 5, padding=2).double()
        g = _gen(seed)
        x = torch.randn(b, c, h, w, generator=g).double().requires_grad_(True)
        y = torch.relu(conv(x))
        y.backward(torch.randn(b, c, h, w, generator=g).double())
        for k, ref in (("y", y), ("dx", x.grad), ("dw", conv.weight.grad), ("db", conv.bias.grad)):
            _close(o[k], ref, 2e-5, k)                  # the tolerance of the convolutions (test_hip_conv.py)
    return run, check


# ------------------------------------------------------------------------------------------------ per-point products
def _linear(m, k, n, bx3=False):
    def data(seed):
        g = _gen(seed)
        return torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) * 0.1, torch.randn(n, generator=g), torch.randn(m, n, generator=g)

    def run(seed):
        from tomosar2height_amd import mlp
        x, w, bias, gy = (t.to(_dev()) for t in data(seed))
        out = {}
        if bx3:
            assert mlp._bx3_gemm_ok(m, k, n, x, gy)
            out["y"] = mlp.linear_fwd_(x, w, bias, torch.empty(m, n, device=_dev()), bx3=True)
        else:
            xr, wr, br = x.requires_grad_(True), w.requires_grad_(True), bias.requires_grad_(True)
            y = mlp.linear(xr, wr, br)
            y.backward(gy)
            out.update({"y": y.detach(), "dx": xr.grad, "db": br.grad})
        dw, db = torch.empty(n, k, device=_dev()), torch.empty(n, device=_dev())
        mlp.linear_wgrad_(gy, x.detach(), dw, db)
        out.update({"dw": dw, "db2": db})
        return out

    def check(o, seed):
        x, w, bias, gy = (t.double() for t in data(seed))
        _close(o["y"], x @ w.t() + bias, 2e-5, "y")
        _close(o["dw"], gy.t() @ x, 2e-5, "dw")
        _close(o["db2"], gy.sum(0), 2e-5, "db")
        if "dx" in o:
            _close(o["dx"], gy @ w, 2e-5, "dx")
    return run, check


def _trunk(n):
    def run(seed):
        from tomosar2height_amd import mlp
        from tomosar2height_amd.encoder.pointnet import LocalPoolPointnet
        from tomosar2height_amd.tile import TileIndex
        enc = LocalPoolPointnet(feature_dim=32, dim=3, hidden_dim=32, scatter_type="max", unet_type="alto",
                                unet_kwargs=dict(depth=2, merge_mode="concat", start_filts=8), plane_resolution=256)
        enc = det_init_(enc, seed=5).to(_dev())
        tile = TileIndex(synth_cloud(n, seed=seed).to(_dev()), 256)
        out = mlp.point_trunk(tile, tile.pts, enc.fc_pos, enc.blocks, enc.fc_c)
        out.backward(torch.randn(n, 32, generator=_gen(seed)).to(_dev()))
        grads = {k: p.grad for k, p in enc.named_parameters() if p.grad is not None}
        assert len(grads) == 2 + 5 * 5 + 2
        return {"out": out.detach(), **grads}

    def check(o, seed):
        import trunk_ref
        from tomosar2height_amd import mlp
        from tomosar2height_amd.encoder.pointnet import LocalPoolPointnet
        from tomosar2height_amd.tile import TileIndex
        enc = LocalPoolPointnet(feature_dim=32, dim=3, hidden_dim=32, scatter_type="max", unet_type="alto",
                                unet_kwargs=dict(depth=2, merge_mode="concat", start_filts=8), plane_resolution=256)
        enc = det_init_(enc, seed=5).to(_dev())
        names = ["fc_pos.weight", "fc_pos.bias"]
        for i in range(len(enc.blocks)):
            names += [f"blocks.{i}.{k}" for k in ("fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias", "shortcut.weight")]
        names += ["fc_c.weight", "fc_c.bias"]
        ps = dict(enc.named_parameters())
        params = [ps[k].detach() for k in names]
        blocks = [params[2 + 5 * i: 7 + 5 * i] for i in range(len(enc.blocks))]
        tile = TileIndex(synth_cloud(n, seed=seed).to(_dev()), 256)
        cc, nets, pooled_f, hrs, winners, cats = mlp._trunk_forward_fused(tile, tile.pts, params[0], params[1], blocks, params[-2],
                                                                          params[-1], want_x_full=True)
        g_out = torch.randn(n, 32, generator=_gen(seed)).to(_dev())
        want = trunk_ref.fused_backward_float64(tile, params, nets, hrs, winners, cats, g_out)
        for k, ref in zip(names, want):
            _close(o[k], ref, 1e-5, k)                  # test_hip_trunk.py: 1e-5 of the max-norm with the kernels' own masks
    return run, check


# ------------------------------------------------------------------------------------------------ deferred point update
def _deferred(compact):
    """test_compact_sums.py's configuration (its smallest that the Deferred state runs: R = 32, levels r = 16 then r = 32, 128
    channels, one clustered tile of 2100 points whose occupied-row count is no multiple of the 128-row tile)."""
    def run(seed, compact=compact):
        from test_compact_sums import _clustered
        from tomosar2height_amd import deferred
        from tomosar2height_amd.tile import TileIndex
        old, deferred.COMPACT_SUMS = deferred.COMPACT_SUMS, compact
        try:
            R, cb, chans = 32, 32, (128, 128)
            tile = TileIndex([_clustered(2100, 0).to(_dev())], R)            # (one cloud for both runs: the occupied rows size buffers)
            g = _gen(seed)
            base = torch.randn(tile.n_points, cb, generator=g).to(_dev()).requires_grad_()
            fcs, qs = [], []
            for r, c, cprev in ((R // 2, chans[0], cb), (R, chans[1], chans[0])):
                fc_b, fc_c = torch.nn.Linear(2 * c, c), torch.nn.Linear(cprev, c)
                for m in (fc_b, fc_c):
                    with torch.no_grad():
                        m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[1] ** 0.5)
                        m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                    m.to(_dev())
                fcs.append((fc_b, fc_c))
                qs.append(torch.randn(tile.B * r * r, 2 * c, generator=g).to(_dev()).requires_grad_())
            state = deferred.Deferred(tile, [1, 0], list(chans), base)
            assert (state.compact_lv == 0) == compact
            if compact:
                assert int(state.rows[2 * tile.B * R * R].item()) % 128 != 0
            rasters = [state.advance(q, r, fc_b, fc_c) for q, r, (fc_b, fc_c) in zip(qs, (R // 2, R), fcs)]
            sum((ra * torch.randn(ra.shape, generator=g).to(_dev())).sum() for ra in rasters).backward()
            out = {"raster0": rasters[0].detach(), "raster1": rasters[1].detach(), "dq0": qs[0].grad, "dq1": qs[1].grad, "dbase": base.grad}
            for i, pair in enumerate(fcs):
                for j, m in enumerate(pair):
                    out[f"dw{i}{j}"], out[f"db{i}{j}"] = m.weight.grad, m.bias.grad
            return out
        finally:
            deferred.COMPACT_SUMS = old

    def check(o, seed):
        other = run(seed, compact=not compact)          # test_compact_sums.py's criterion: the two forms agree bit for bit
        for k in ("raster0", "raster1", "dq0", "dq1", "dbase", "db00", "db01", "db10", "db11"):
            assert torch.equal(o[k], other[k]), k
    return run, check


# ------------------------------------------------------------------------------------------------ GroupNorm
def _groupnorm(b, c, h, w, groups):
    def run(seed):
        from tomosar2height_amd.encoder import hourglass as hg
        x = torch.randn(b, c, h, w, generator=_gen(seed))
        return {"stats": hg.group_norm_stats(_cl(x), groups, 1e-5)}

    def check(o, seed):
        import hg_ref
        x = torch.randn(b, c, h, w, generator=_gen(seed))
        one = torch.ones(c, dtype=D)
        _, mean64, rstd64 = hg_ref.group_norm(x.double(), groups, one, 0 * one, 1e-5, stats=True)
        _, t_mean, t_rstd = torch.native_group_norm(x, None, None, b, c, h * w, groups, 1e-5)
        got = o["stats"].cpu().double()
        for mine, theirs, ref in ((got[..., 0], t_mean, mean64), (got[..., 1], t_rstd, rstd64)):
            ref = ref.reshape(b, groups)                # test_hourglass_gpu.py: four times torch's own float32 error
            bar = 4 * ((theirs.double().reshape(b, groups) - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
            assert ((mine - ref).abs() / ref.abs().clamp_min(1e-30)).max().item() <= max(bar, 1e-6)
    return run, check


# ------------------------------------------------------------------------------------------------ integer workspaces (stale)
def _fps(n, npoint):
    def run(seed):
        from tomosar2height_amd import pointops
        pts = torch.rand(1, n, 3, generator=_gen(seed)).to(_dev())
        return {"idx": pointops.farthest_point_sample(pts, npoint, torch.zeros(1, dtype=torch.long, device=_dev()))}

    def check(o, seed):
        import pnpp_ref
        pts = torch.rand(1, n, 3, generator=_gen(seed))
        assert np.array_equal(o["idx"].cpu().numpy()[0], np.asarray(pnpp_ref.fps(pts[0].numpy(), npoint, 0)))
    return run, check


def _raster_inputs(seed, hw):
    rng = np.random.default_rng(seed)
    gt = (rng.random((hw, hw)) * 30).astype(np.float32)
    target = gt + rng.normal(size=(hw, hw)).astype(np.float32)
    mask = np.zeros((hw, hw), bool)
    for _ in range(12):
        r, c = rng.integers(0, hw - 9, 2)
        mask[r:r + rng.integers(2, 9), c:c + rng.integers(2, 9)] = True
    return target, gt, mask


def _evaluator(hw):
    def run(seed):
        from tomosar2height_amd import DSMEvaluator
        target, gt, mask = _raster_inputs(seed, hw)
        ev = DSMEvaluator(torch.from_numpy(gt).to(_dev()), bounds=(0.0, 0.0), pixel_size=(1.0, 1.0),
                          other_masks={"building": torch.from_numpy(mask).to(_dev())})
        stats, diff = ev.eval(torch.from_numpy(target).to(_dev()), top_left=(0.5, -0.5))
        def leaves(v):
            if isinstance(v, dict):
                return [x for k in sorted(v) for x in leaves(v[k])]
            return [float(x) for x in np.ravel(v.cpu().numpy() if isinstance(v, torch.Tensor) else v)]
        flat = torch.tensor(leaves(stats), dtype=D)
        return {"diff": diff, "stats": flat}

    def check(o, seed):
        import eval_ref
        target, gt, mask = _raster_inputs(seed, hw)
        _, want_diff = eval_ref.evaluate(target, gt, None, {"building": mask}, 0, 0)
        eval_ref.assert_diff(o["diff"].cpu().numpy(), want_diff)
    return run, check


def _instances(hw):
    def run(seed):
        from tomosar2height_amd import label_components, segment_medians
        target, mask = _raster_inputs(seed, hw)[0], _raster_inputs(0, hw)[2]      # one mask: K sizes the buffers
        labels, k = label_components(torch.from_numpy(mask).to(_dev()), 2)
        counts, med = segment_medians(torch.from_numpy(target).to(_dev()), labels, k)
        return {"labels": labels, "counts": counts, "medians": med}

    def check(o, seed):
        import inst_ref
        target, _, mask = _raster_inputs(seed, hw)
        labels = o["labels"].cpu().numpy()
        k = int(labels.max())
        want_counts, want = inst_ref.segment_medians(target, labels, k)
        assert o["counts"].cpu().numpy().tobytes() == want_counts.tobytes()
        assert inst_ref.same_floats(o["medians"].cpu().numpy(), want)
    return run, check


def _cloud_medians(n, k):
    def data(seed):
        rng = np.random.default_rng(seed)
        return rng.random((n, 3)) * 50, rng.integers(0, k + 1, n).astype(np.int32)

    def run(seed):
        from tomosar2height_amd import point_medians
        pts, lab = data(seed)
        counts, med = point_medians(torch.from_numpy(pts).to(_dev()), torch.from_numpy(lab).to(_dev()), k)
        return {"counts": counts, "medians": med}

    def check(o, seed):
        import cloud_inst_ref
        pts, lab = data(seed)
        want_counts, want = cloud_inst_ref.point_medians(pts[:, 2], lab, k)
        assert o["counts"].cpu().numpy().tobytes() == want_counts.tobytes()
        assert o["medians"].cpu().numpy().tobytes() == np.asarray(want).tobytes()
    return run, check


def _interp(n, tin):
    def data(seed):
        rng = np.random.default_rng(seed)
        return np.concatenate([rng.random((n, 2)) * 40, rng.random((n, 1)) * 20], 1)

    def run(seed):
        from tomosar2height_amd import CloudIndex, delaunay_dsm, idw_dsm, nearest_dsm
        index = CloudIndex(torch.from_numpy(data(seed)).to(_dev()))
        out = {"unique": index.unique, "nearest": nearest_dsm(index, 1.0)[0], "idw": idw_dsm(index, 1.0, k=8)[0]}
        if tin:
            out["tin"] = delaunay_dsm(index, 1.0)[0]
        return out

    def check(o, seed):
        import interp_ref
        u = interp_ref.unique_cloud(data(seed))
        assert o["nearest"].cpu().numpy().tobytes() == interp_ref.nearest(u, 1.0)[0].tobytes()
        assert np.abs(o["idw"].cpu().numpy() - interp_ref.idw(u, 1.0, 8)[0]).max() <= interp_ref.idw_bound(u[:, 2])
    return run, check


def _crop(p):
    def run(seed):
        from tomosar2height_amd.producer import TileProducer
        rng = np.random.default_rng(seed)
        chunk = np.concatenate([rng.random((p, 2)) * 1024 + [1000.0, 5000.0], rng.random((p, 1)) * 60], 1)
        tile = TileProducer(torch.from_numpy(chunk).to(_dev())).crop((1200.0, 5300.0), with_index=True)
        return {k: v for k, v in tile.items() if isinstance(v, torch.Tensor)}

    def check(o, seed):
        from oracle import producer_ref
        from test_tile_producer import Z_SPAN, _ulp_close
        rng = np.random.default_rng(seed)
        chunk = np.concatenate([rng.random((p, 2)) * 1024 + [1000.0, 5000.0], rng.random((p, 1)) * 60], 1)
        idx, pts, _ = producer_ref.produce_tile(chunk, (1200.0, 5300.0), z_span=Z_SPAN)
        assert np.array_equal(o["index"].cpu().numpy(), idx)
        _ulp_close(o["inputs"][0].cpu().numpy(), pts)
    return run, check


# ------------------------------------------------------------------------------------------------ the whole network
def _model(train):
    def run(seed):
        from tomosar2height_amd import TomoSAR2Height
        from tomosar2height_amd.config import berlin_config
        from tomosar2height_amd.trainer import Trainer
        cfg = berlin_config()
        cfg.model.encoder_kwargs.unet_kwargs.depth = 4
        model = det_init_(TomoSAR2Height(cfg), seed=21).to(_dev())
        model.set_channels_last(True)
        tiles = [{"inputs": synth_cloud(49152, seed=seed + i).to(_dev()),
                  "dsm": (torch.rand(1, 512, 512, generator=_gen(seed + i)) * 30).to(_dev())} for i in range(2)]
        if not train:
            model.eval()
            with torch.no_grad():
                return {"heights": model(input_cloud=tiles[0]["inputs"])[0]}
        tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.0), device=_dev(), optimize_every=100, use_cloud=True)
        tr.coalesce_tiles = 1
        for t in tiles:
            tr.train_step(t)
        tr.flush_gradients()
        torch.cuda.synchronize()
        return {"bucket": tr.bucket.flat, "loss": torch.tensor(float(tr.accumulated_loss), dtype=D)}

    def check(o, seed):
        """The CPU torch oracle with the same weights (as __graft_entry__.smoke and test_hip_model.py do): heights to 1e-4 of
        their scale, the window's summed L1 loss to 1e-4.  (Gradients against the oracle: test_hip_model.py, at the 1e-2 / 3e-3
        that mask flips allow; here they are compared bit for bit with the clean step.)"""
        from oracle import torch_ref
        from tomosar2height_amd.config import berlin_config
        cfg = berlin_config()
        cfg.model.encoder_kwargs.unet_kwargs.depth = 4
        ref = det_init_(torch_ref.TomoSAR2Height(cfg), seed=21)
        loss = 0.0
        with torch.no_grad():
            for i in range(2 if train else 1):
                pa, _ = ref(input_cloud=synth_cloud(49152, seed=seed + i))
                if not train:
                    rel = ((o["heights"].cpu() - pa).abs().max() / pa.abs().max()).item()
                    assert rel <= 1e-4, rel
                dsm = torch.rand(1, 512, 512, generator=_gen(seed + i)) * 30
                loss += F.l1_loss(pa.squeeze(), dsm.squeeze()).item()
        if train:
            assert abs(o["loss"].item() - loss) <= 1e-4 * abs(loss), (o["loss"].item(), loss)
    return run, check


# ------------------------------------------------------------------------------------------------ tile builds (tile.py)
def _index_ref(cloud, reso):
    """The index restatement of test_hip_ops.py::test_tile_index_bit_exact (the C oracle's cell of each point, Morton code, a
    STABLE sort per tile, CSR offsets), as the four arrays the build writes -- so that they compare byte for byte."""
    from oracle import c_oracle
    from test_hip_ops import _morton
    b, n, _ = cloud.shape
    idx = c_oracle.coordinate2index(cloud.numpy(), reso)[:, 0]
    m0 = reso * reso
    code = _morton(idx % reso, idx // reso).astype(np.int64) + np.arange(b)[:, None] * m0
    perm = np.stack([np.argsort(code[k], kind="stable") for k in range(b)])
    counts = np.bincount(code.reshape(-1), minlength=b * m0)
    return {"pts": np.concatenate([cloud.numpy()[k][perm[k]] for k in range(b)]),
            "perm": perm.reshape(-1).astype(np.int32), "cell": np.take_along_axis(code, perm, 1).reshape(-1).astype(np.int32),
            "off0": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)}


def _tile_case(b, n, reso):
    def run(seed):
        from tomosar2height_amd.tile import TileIndex
        t = TileIndex(synth_cloud(n, seed=seed, batch=b).to(_dev()), reso)
        assert t.out_of_domain() == 0
        return {"pts": t.pts, "perm": t.perm, "cell": t.cell, "off0": t.off0}

    def check(o, seed):
        want = _index_ref(synth_cloud(n, seed=seed, batch=b), reso)
        for k, ref in want.items():
            got = o[k].cpu().numpy()
            assert got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes(), k
    return Case(f"tile-build-b{b}-n{n}-r{reso}", "TileIndex(cloud, R) (t2h_tile_build)", run, "stale",
                "sort keys, histograms and scans (tile_index.hip); an integer site of the harness under every fill",
                [("t2h_tile_workspace_bytes", (b, n, reso.bit_length() - 1), ">0")], check, sites=("/tile.py:",))


def _ragged_tile_case(counts, reso):
    def clouds(seed):
        return [synth_cloud(k, seed=seed + 31 * i).to(_dev()) for i, k in enumerate(counts)]

    def run(seed):
        from tomosar2height_amd.tile import TileIndex
        t = TileIndex(clouds(seed), reso)
        assert t.ragged and t.n_points == sum(counts) and t.out_of_domain() == 0
        return {"pts": t.pts, "perm": t.perm, "cell": t.cell, "off0": t.off0}

    def check(o, seed):
        """test_hip_ragged.py::test_ragged_tile_index_equals_the_single_tile_indices: tile by tile the single-tile index."""
        from tomosar2height_amd.tile import TileIndex
        m0, row = reso * reso, 0
        assert o["pts"].shape == (sum(counts), 4) and o["off0"].numel() == len(counts) * m0 + 1
        for b, (c, n) in enumerate(zip(clouds(seed), counts)):
            one = TileIndex(c, reso)
            assert torch.equal(o["pts"][row:row + n, :3], one.pts)
            assert torch.equal(o["pts"][row:row + n, 3].view(torch.int32), torch.full((n,), b, dtype=torch.int32, device=_dev()))
            assert torch.equal(o["perm"][row:row + n], one.perm)
            assert torch.equal(o["cell"][row:row + n], one.cell + b * m0)
            assert torch.equal(o["off0"][b * m0:(b + 1) * m0 + 1], one.off0 + row)
            row += n
    return Case(f"tile-build-ragged-{'+'.join(map(str, counts))}-r{reso}", "TileIndex([clouds], R) (t2h_tile_build_ragged)", run,
                "stale", "as the uniform build; sized by (B, total, max count)",
                [("t2h_tile_ragged_workspace_bytes", (len(counts), sum(counts), max(counts), reso.bit_length() - 1), ">0")], check,
                sites=("/tile.py:",))


# ------------------------------------------------------------------------------------------------ split-weight buffers (grid.py)
_SPLIT_SITE = ("/grid.py:", "(_get)")                    # SplitWeightCache._get
_SPLIT_QUERY = {("conv", "f16x2"): "t2h_conv3x3_f16x2_weights_bytes", ("conv", "bf16x3"): "t2h_conv3x3_bx3_weights_bytes",
                ("gemm", "f16x2"): "t2h_gemm_f16x2_weights_bytes", ("gemm", "bf16x3"): "t2h_gemm_bx3_weights_bytes"}
_SPLIT_WHY = ("packed 16-bit planes and a trailer of scale and exponent, never an index: may start from 0xFF; every byte of the "
              "buffer is compared as well (the single prepare writes all of it, conv_bx3.hip:1447-1487)")


def _split_conv_case(cin, cout, precision):
    """Both 3x3 kinds at the smallest plane the split kernels take (4 x 32): ``get(w, False)`` under the forward, ``get(w, True)``
    under the data gradient; float64 F.conv2d at test_hip_conv.py's 2e-5 of the max-norm."""
    b, h, w = 1, 4, 32

    def data(seed):
        g = _gen(seed)
        return (torch.randn(b, cin, h, w, generator=g), torch.randn(cout, cin, 3, 3, generator=g) * 0.1, torch.randn(cout, generator=g),
                torch.randn(b, cout, h, w, generator=g))

    def run(seed):
        from tomosar2height_amd import grid
        x, wt, bias, gy = data(seed)
        assert grid.bx3_applicable(b, h, w, cin, cout)
        wd = _cl(wt)
        y = grid.conv3x3_fwd_(_cl(x), wd, bias.to(_dev()), grid._empty_cl(b, cout, h, w, _dev()))
        dx = grid.conv3x3_dgrad_(_cl(gy), wd, grid._empty_cl(b, cin, h, w, _dev()))
        return {"y": y, "dx": dx, "wf": grid.split_weights.get(wd, False).clone(), "wf_t": grid.split_weights.get(wd, True).clone()}

    def check(o, seed):
        x, wt, bias, gy = (t.double() for t in data(seed))
        x.requires_grad_(True)
        want = F.conv2d(x, wt, bias, padding=1)
        want.backward(gy)
        _close(o["y"], want, 2e-5, "y")
        _close(o["dx"], x.grad, 2e-5, "dx")
    return Case(f"split-conv3x3-{precision}-cin{cin}-cout{cout}", "SplitWeightCache.get, both orientations, under conv3x3_fwd_ / "
                "conv3x3_dgrad_", run, "nan", _SPLIT_WHY, [(_SPLIT_QUERY["conv", precision], (cin, cout), ">0")], check,
                {"grid.CONV_PRECISION": precision, "grid.BX3_MIN_PIXELS": 0}, sites=(_SPLIT_SITE,))


def _split_gemm_case(k, n, precision, pad=0):
    """Both matrix kinds at the fewest rows the split product takes (128): ``get_gemm(w [N,K], False)`` under y = x w^T + bias and
    ``get_gemm(w [K,N], True)`` under y = x w; ``pad``: each weight is a column slice of a matrix ``pad`` columns wider (ldw > row
    length).  float64 at test_hip_gemm.py's 2e-5 of the max-norm (test_gemm_bx3_rows_vs_float64)."""
    m = 128

    def data(seed):
        g = _gen(seed)
        return (torch.randn(m, k, generator=g), torch.randn(n, k + pad, generator=g) / k ** 0.5, torch.randn(k, n + pad, generator=g) / k ** 0.5,
                torch.randn(n, generator=g))

    def run(seed):
        from tomosar2height_amd import _lib, grid, mlp
        assert _lib.ws_bytes("t2h_gemm_bx3_supported", m, k, n)
        x, wide_nk, wide_kn, bias = (t.to(_dev()) for t in data(seed))
        w_nk, w_kn = wide_nk[:, pad // 2:pad // 2 + k], wide_kn[:, pad // 2:pad // 2 + n]
        assert (w_nk.stride(0) > k) == (pad > 0) and (w_kn.stride(0) > n) == (pad > 0)
        y_nk = mlp._gemm_bx3(x, w_nk, False, bias, None, torch.empty(m, n, device=_dev()), False, False, "split-gemm-nk")
        y_kn = mlp._gemm_bx3(x, w_kn, True, None, None, torch.empty(m, n, device=_dev()), False, False, "split-gemm-kn")
        return {"y_nk": y_nk, "y_kn": y_kn, "wf_nk": grid.split_weights.get_gemm(w_nk, False).clone(),
                "wf_kn": grid.split_weights.get_gemm(w_kn, True).clone()}

    def check(o, seed):
        x, wide_nk, wide_kn, bias = (t.double() for t in data(seed))
        _close(o["y_nk"], x @ wide_nk[:, pad // 2:pad // 2 + k].t() + bias, 2e-5, "y_nk")
        _close(o["y_kn"], x @ wide_kn[:, pad // 2:pad // 2 + n], 2e-5, "y_kn")
    return Case(f"split-gemm-{precision}-k{k}-n{n}" + (f"-ldw+{pad}" if pad else ""), "SplitWeightCache.get_gemm, [N,K] and [K,N], "
                "under t2h_gemm_bx3 (mlp._gemm_bx3)", run, "nan", _SPLIT_WHY, [(_SPLIT_QUERY["gemm", precision], (k, n), ">0")],
                check, {"grid.CONV_PRECISION": precision}, sites=(_SPLIT_SITE, "mlp.py:94"))


def _split_up_case(cin, cout, precision):
    """Both transposed-convolution kinds at the smallest plane the split kernels take (4 x 32 = 128 pixels): ``get_up(w, True)`` under
    the forward, ``get_up(w, False)`` under the data gradient; float64 conv_transpose2d at test_hip_conv.py's 2e-5."""
    b, h, w = 1, 4, 32

    def data(seed):
        g = _gen(seed)
        return (torch.randn(b, cin, h, w, generator=g), torch.randn(cin, cout, 2, 2, generator=g) * 0.1, torch.randn(cout, generator=g),
                torch.randn(b, cout, 2 * h, 2 * w, generator=g))

    def run(seed):
        from tomosar2height_amd import _lib, grid
        x, wt, bias, gy = data(seed)
        assert _lib.ws_bytes("t2h_upconv2x2_bx3_supported", b, h, w, cin, cout)
        wd = _cl(wt)                                                     # [Cin][2][2][Cout] in memory
        y = grid.upconv2x2_fwd_(_cl(x), wd, bias.to(_dev()), None, grid._empty_cl(b, cout, 2 * h, 2 * w, _dev()), True)
        dx = grid.upconv2x2_dgrad_(_cl(gy), cout, wd, grid._empty_cl(b, cin, h, w, _dev()), True)
        return {"y": y, "dx": dx, "wf_kn": grid.split_weights.get_up(wd, True).clone(), "wf_nk": grid.split_weights.get_up(wd, False).clone()}

    def check(o, seed):
        x, wt, bias, gy = (t.double() for t in data(seed))
        x.requires_grad_(True)
        want = F.conv_transpose2d(x, wt, bias, stride=2)
        want.backward(gy)
        _close(o["y"], want, 2e-5, "y")
        _close(o["dx"], x.grad, 2e-5, "dx")
    return Case(f"split-upconv2x2-{precision}-cin{cin}-cout{cout}", "SplitWeightCache.get_up, [K,N] and [N,K], under upconv2x2_fwd_ / "
                "upconv2x2_dgrad_", run, "nan", _SPLIT_WHY, [(_SPLIT_QUERY["gemm", precision], (cin, 4 * cout), ">0")], check,
                {"grid.CONV_PRECISION": precision}, sites=(_SPLIT_SITE,))


def _sizing_cases():
    """The smallest shapes at which a size query or a trailer offset can be wrong (tile builds, split-weight buffers)."""
    cases = [_tile_case(1, 1, 2), _tile_case(1, 5, 2),
             _tile_case(2, 2049, 64),                      # one element past a 2048 block
             _tile_case(1, 300, 1024),                     # 2^20 cells for 300 points: the histogram part dominates
             _tile_case(3, 257, 16),
             _ragged_tile_case((1, 2049, 7), 16),          # max count far from both ends
             _ragged_tile_case((3, 4097), 256),            # max ~ total
             _ragged_tile_case((1, 1, 1, 1), 2),           # B cells >= points
             _ragged_tile_case((600,), 1024)]
    for precision in ("f16x2", "bf16x3"):
        # t2h_conv3x3_bx3_supported: Cin, Cout multiples of 32 from 32; t2h_gemm_bx3_supported: K a multiple of 64 from 64, N of 32
        # from 32 (its smallest pair already has K != N); t2h_upconv2x2_bx3_supported: Cin, Cout multiples of 64 from 64
        cases += [_split_conv_case(32, 32, precision), _split_conv_case(32, 64, precision),
                  _split_gemm_case(64, 32, precision), _split_gemm_case(64, 32, precision, pad=32),
                  _split_up_case(64, 64, precision), _split_up_case(64, 128, precision)]
    return cases


def _cases():
    cases = [
        # coarse plan on, S = 8 (rows_per_tile >= 16 cells, C % 4 == 0); C = 12 keeps it; C = 6 and reso 16 switch it off
        _pg_case("point-grid-300-r4-c8", 300, 4, 8, 1, ">0", ">0", False),
        _pg_case("point-grid-300-r4-c12", 300, 4, 12, 1, ">0", ">0", False),
        _pg_case("point-grid-300-r4-c6", 300, 4, 6, 1, "==0", "==0", False),
        _pg_case("point-grid-300-r16-c8", 300, 16, 8, 1, "==0", "==0", False),
        _pg_case("point-grid-300-r4-c8-b2", 300, 4, 8, 2, ">0", ">0", False),
        _pg_case("point-grid-ragged-290+10-r4-c8", 0, 4, 8, 1, "==0", ">0", False, ragged=(290, 10)),
        # n <= 4 B r^2: the transposed sampling matrix (tile.sample_adjoint's offsets / entries)
        _pg_case("point-grid-60-r4-c8-adjoint", 60, 4, 8, 1, "==0", "==0", True),
        _pg_case("point-grid-300-r16-c8-adjoint", 300, 16, 8, 1, "==0", "==0", True),
        # 3x3 convolutions: smallest channel counts (16), B = 1 / 3, non-square; first shapes with a split reduction
        _conv_case(1, 8, 8, 16, 16, "fp32", "==0", "==0", ">0"),
        _conv_case(3, 4, 8, 16, 16, "fp32", "==0", "==0", ">0"),
        _conv_case(1, 8, 8, 512, 256, "fp32", ">0", ">0", ">0"),
        _conv_case(1, 32, 32, 32, 32, "bf16x3", "==0", "==0", ">0", "t2h_conv3x3_bx3_weights_bytes"),
        _conv_case(1, 32, 32, 32, 32, "f16x2", "==0", "==0", ">0", "t2h_conv3x3_f16x2_weights_bytes"),
        _conv_case(3, 8, 32, 64, 256, "f16x2", ">0", ">0", ">0", "t2h_conv3x3_f16x2_weights_bytes"),
        _conv_case(3, 8, 32, 64, 256, "bf16x3", ">0", ">0", ">0", "t2h_conv3x3_bx3_weights_bytes"),
        _upconv_case(1, 8, 8, 16, 16, "fp32", "==0", ">0"),
        _upconv_case(3, 4, 8, 16, 16, "fp32", "==0", ">0"),
        _upconv_case(2, 16, 16, 128, 64, "fp32", ">0", ">0"),
        _upconv_case(2, 16, 16, 128, 64, "f16x2", ">0", "==0", "t2h_gemm_f16x2_weights_bytes"),
        _upconv_case(3, 8, 32, 64, 256, "bf16x3", ">0", ">0", "t2h_gemm_bx3_weights_bytes"),
    ]
    for b, h, w in ((1, 8, 8), (3, 5, 7)):
        run, check = _module_conv("small", b, h, w, 3, 32)
        cases.append(Case(f"smallcin-{b}x{h}x{w}", "grid.conv_bias_act (Conv2d(3, 32, 3))", run, "nan",
                          "per-workgroup float partials of dw / db (conv_small.hip:190)",
                          [("t2h_conv3x3_smallcin_wgrad_workspace_bytes", (3, 32), ">0")], check))
        run, check = _module_conv("1x1", b, h, w, 16, 16)
        cases.append(Case(f"conv1x1-{b}x{h}x{w}", "grid.conv1x1 (the weight gradient of grid.py:544)", run, "nan",
                          "split-K float partials (gemm.hip:749)", [("t2h_linear_wgrad_workspace_bytes", (b * h * w, 16, 16), ">0")], check))
        run, check = _module_conv("head", b, h, w, 32, 1)
        cases.append(Case(f"head1x1-{b}x{h}x{w}", "grid.head1x1 (grid.py:718)", run, "nan",
                          "two-stage float sums of dw / db (grid_fused.hip:431)",
                          [("t2h_head1x1_bwd_workspace_bytes", (b * h * w, 32), ">0")], check))
    for m in (1, 127, 129):                              # one row, one below and one above a multiple of the 128-row tile
        run, check = _linear(m, 16, 16)
        cases.append(Case(f"linear-{m}x16x16", "mlp.linear forward / backward, mlp.linear_wgrad_", run, "nan",
                          "split-K float partials (gemm.hip:749)", [("t2h_linear_wgrad_workspace_bytes", (m, 16, 16), ">0")], check))
        cases.append(Case(f"trunk-{m}", "mlp.point_trunk forward and backward (the chain's shared workspace, mlp.py:693)", _trunk(m)[0],
                          "stale", "float slabs of the block gradients (trunk.hip:1444) next to TileIndex's integer buffers",
                          [("t2h_trunk_block_bwd_workspace_bytes", (m,), ">0")], _trunk(m)[1], nan_sites=("mlp.py:166",)))
    run, check = _linear(4096, 128, 128, bx3=True)
    cases.append(Case("gemm-bx3-4096x128x128", "mlp.linear_fwd_(bx3=True)", run, "nan", "split-K float slabs (conv_bx3.hip:1262)",
                      [("t2h_gemm_bx3_workspace_bytes", (4096, 128, 128), ">0"), ("t2h_gemm_f16x2_weights_bytes", (128, 128), ">0")],
                      check, {"grid.CONV_PRECISION": "f16x2"}, sites=("mlp.py:94",)))
    run, check = _linear(4096, 64, 512, bx3=True)         # one 64-wide chunk into a wide matrix (the persistent form): no split
    cases.append(Case("gemm-bx3-4096x64x512", "mlp.linear_fwd_(bx3=True)", run, "nan", "no slabs at one chunk (conv_bx3.hip:1262)",
                      [("t2h_gemm_bx3_workspace_bytes", (4096, 64, 512), "==0")], check, {"grid.CONV_PRECISION": "f16x2"},
                      sites=("mlp.py:94",)))
    run, check = _linear(4096, 64, 1024)
    cases.append(Case("gemm-bx3-wgrad-4096x64x1024", "mlp.linear_wgrad_ on the split kernels", run, "nan",
                      "float slabs (conv_bx3.hip:1301)", [("t2h_gemm_bx3_wgrad_workspace_bytes", (4096, 64, 1024), ">0")], check,
                      {"grid.CONV_PRECISION": "f16x2", "mlp._GEMM_BX3_WGRAD": True}))
    for compact in (True, False):
        run, check = _deferred(compact)
        cases.append(Case(f"deferred-r32-2100-compact{int(compact)}", "deferred.Deferred.advance x 2 and its backward (t2h_segsum_fwd / "
                          "_bwd_multi, t2h_sample_bwd_from_sums, t2h_mean_bias_bwd; deferred.py:56, :271, :498)", run, "stale",
                          "the occupied-row lists are integer tensors (deferred.py:93); the workspaces of deferred.py and mlp.py hold "
                          "float partials only", [("t2h_mean_bias_bwd_workspace_bytes", (1024, 128), ">0")], check,
                          sites=("deferred.py:56", "deferred.py:271"), nan_sites=("deferred.py", "mlp.py:94", "mlp.py:166"), loose=True))
    # GroupNorm: h w c just above 65 536 (two-stage partials), at it (the one-byte form), groups of 5 channels
    for b, c, h, w, groups, two_stage in ((1, 256, 16, 17, 4, True), (1, 256, 16, 16, 4, False), (2, 20, 33, 31, 4, False),
                                          (1, 20, 82, 80, 4, True)):       # five channels a group over two 65 536-element chunks
        run, check = _groupnorm(b, c, h, w, groups)
        cases.append(Case(f"groupnorm-{b}x{c}x{h}x{w}-g{groups}", "hourglass.group_norm_stats", run, "nan",
                          "float partial sums per (chunk, group) (hourglass.hip:273)",
                          [("t2h_hg_groupnorm_workspace_bytes", (b, h, w, c, groups), ">0")], check))
    run, check = _fps(3000, 64)
    cases.append(Case("fps-3000", "pointops.farthest_point_sample", run, "stale", "distances and arg-max indices (pnpp.hip:298)",
                      [("t2h_fps_workspace_bytes", (1, 3000, 1024), ">0")], check))
    run, check = _evaluator(64)
    cases.append(Case("evaluator-64x64", "DSMEvaluator.eval", run, "stale", "sort keys and class histograms (dsm_eval.hip:421)",
                      [("t2h_eval_stats_workspace_bytes", (4096, 2), ">0")], check, sites=("evaluator.py",), loose=True))
    run, check = _instances(64)
    cases.append(Case("instances-64x64", "label_components / segment_medians", run, "stale",
                      "union-find parents, label maps, sort keys (dsm_instances.hip:260, :300)",
                      [("t2h_inst_label_workspace_bytes", (64, 64), ">0"), ("t2h_inst_medians_workspace_bytes", (4096, 5), ">0")], check,
                      sites=("instances.py:61", "instances.py:97"), loose=True))
    run, check = _cloud_medians(3000, 5)
    cases.append(Case("cloud-medians-3000", "point_medians", run, "stale", "segment offsets and sort keys (dsm_cloud.hip:143)",
                      [("t2h_cloud_medians_workspace_bytes", (3000, 5), ">0")], check))
    run, check = _interp(3000, True)
    cases.append(Case("interp-tin-3000", "CloudIndex / nearest_dsm / idw_dsm / delaunay_dsm", run, "stale",
                      "cell histograms, the sorted index, hull stacks (dsm_interp.hip:438, :459, dsm_tin.hip:402); the triangulation "
                      "against tests/tin_ref.py: test_tin_gpu.py",
                      [("t2h_interp_bounds_workspace_bytes", (3000,), ">0"), ("t2h_interp_index_workspace_bytes", (3000,), ">0"),
                       ("t2h_tin_hull_workspace_bytes", (3000,), ">0")], check,
                      sites=("interpolate.py:100", "interpolate.py:103", "interpolate.py:134"), loose=True))
    cases.append(Case("crop-3000", "TileProducer.crop", _crop(3000)[0], "stale",
                      "the kept-point counter and scan (tile_producer.hip:141)",
                      [("t2h_tile_crop_workspace_bytes", (3000,), ">0")], _crop(3000)[1]))
    cases.append(Case("bias-relu-bwd-3x5x7", "grid.conv_bias_act on a 5 x 5 convolution (library forward, fused bias / ReLU backward, "
                      "grid.py:92)", *_bias_relu(3, 5, 7, 16)[:1], "nan", "float partial sums of db (grid_fused.hip:387)",
                      [("t2h_bias_relu_bwd_workspace_bytes", (3 * 5 * 7, 16), ">0")], _bias_relu(3, 5, 7, 16)[1]))
    model_queries = [("t2h_mean_bias_bwd_workspace_bytes", (16384, 64), ">0"), ("t2h_cell_order_len", (1, 8, 1), ">0")]
    cases.append(Case("train-step-depth4-49152", "Trainer.train_step x 2, coalesce_tiles = 1 (test_hip_model.py's bit-reproducible step)",
                      _model(True)[0], "stale", "every workspace of the step, integer ones included; the split-K, slab and "
                      "coarse-walk partials of grid.py, mlp.py:94 / :166, ops.py and deferred.py are floats only", model_queries,
                      _model(True)[1],
                      # the last two: the tile build's and the split-weight cache's buffers are banded workspaces of this step --
                      # a refactor that allocates them by hand again takes them out of the guard, and fails here
                      sites=("deferred.py:56", "deferred.py:271", "deferred.py:498", "mlp.py:693", "grid.py", "/tile.py:", _SPLIT_SITE),
                      nan_sites=("grid.py", "mlp.py:94", "mlp.py:166", "ops.py", "deferred.py"), loose=True))
    cases.append(Case("inference-depth4-49152", "TomoSAR2Height.forward under no_grad", _model(False)[0], "stale",
                      "as the training row", [], _model(False)[1], sites=("deferred.py:56", "grid.py"),
                      nan_sites=("grid.py", "mlp.py:94", "ops.py", "deferred.py")))
    return cases + _sizing_cases()


CASES = _cases()


def _bits(t):
    t = t.detach().clone(memory_format=torch.contiguous_format).reshape(-1)
    return t.view(torch.uint8) if t.numel() else t


class _switches:
    def __init__(self, setup):
        self.setup = setup

    def __enter__(self):
        import importlib
        self.old = []
        for path, value in self.setup.items():
            mod, attr = path.rsplit(".", 1)
            m = importlib.import_module("tomosar2height_amd." + mod)
            self.old.append((m, attr, getattr(m, attr)))
            setattr(m, attr, value)

    def __exit__(self, *exc):
        for m, attr, value in self.old:
            setattr(m, attr, value)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_result_does_not_depend_on_what_the_scratch_held(case):
    from tomosar2height_amd import _lib
    with _switches(case.setup):
        lib = _lib.load()
        for name, args, sign in case.queries:
            size = int(getattr(lib, name)(*args))
            print(f"{case.id}: {name}{args} = {size} bytes, fill {case.fill}, bit-identical mode")
            assert (size > 0) == (sign == ">0"), (name, args, size, sign)
        clean = case.run(11)
        torch.cuda.synchronize()
        if case.check is None:                                   # (rows with a reference are judged by it; a TIN raster is NaN off the hull)
            assert all(bool(torch.isfinite(v).all()) for v in clean.values() if v.is_floating_point())
        if case.check is not None:
            case.check(clean, 11)
        with guarded_scratch("record") as rec:                   # the same calls on another input of the same shape, over zeros
            case.run(12)
        with guarded_scratch(case.fill, record=rec.log, nan_sites=case.nan_sites) as g:
            got = case.run(11)
        assert any(e[0] == "ws" for e in g.log), "no workspace was handed out"
        handed = {e[1] for e in g.log}
        for name, args, sign in case.queries:                    # the package asked THIS query and allocated what it returned
            if sign == ">0" and not case.loose and not name.endswith("_len"):
                assert int(getattr(lib, name)(*args)) in handed, (name, args, sorted(handed)[-8:])
        seen = sorted({e[5] for e in g.log if e[0] == "ws"})            # a site: a substring, or a tuple of them that all occur
        assert all(any(_hit(s, (key,)) for s in seen) for key in case.sites), (case.sites, seen)
        print(f"{case.id}: workspaces " + ", ".join(f"{e[1]} B at {e[5].rsplit('/', 1)[-1]}" for e in g.log if e[0] == "ws")[:4000])
        assert got.keys() == clean.keys()
        for k in clean:
            assert got[k].shape == clean[k].shape and got[k].dtype == clean[k].dtype, k
            assert torch.equal(_bits(got[k]), _bits(clean[k])), f"{case.id}: {k} depends on what the scratch held before"


# ------------------------------------------------------------------------------------------------ the batched refresh, under guard
def _mixed_weights(seed):
    """25 small weights, one buffer each, the six kinds in turn and two sizes of each; every fourth matrix is a column slice of a
    wider one.  ``[(weight, cache -> its buffer)]`` in the order the cache will hold them: t2h_split_weights_batch takes 24 buffers
    a launch, so the 25th is alone in the second."""
    g = _gen(seed)
    out = []
    for i in range(25):
        kind, big = i % 6, (i // 6) & 1
        if kind < 2:                                                         # 3x3 [Cout,Cin,3,3], forward / transposed
            cin, cout = (32, 64) if big else (32, 32)
            w = _cl(torch.randn(cout, cin, 3, 3, generator=g))
            out.append((w, lambda c, w=w, t=kind == 1: c.get(w, t)))
        elif kind < 4:                                                       # a matrix read as [K,N] / as [N,K]
            k, n = (64, 32) if big else (16, 64)
            rows, cols = (k, n) if kind == 2 else (n, k)
            w = torch.randn(rows, cols + (16 if i % 4 == 3 else 0), generator=g).to(_dev())[:, :cols]
            out.append((w, lambda c, w=w, kn=kind == 2: c.get_gemm(w, kn)))
        else:                                                                # ConvTranspose2d weight [Cin,Cout,2,2] as [K,N] / [N,K]
            cin, cout = (64, 16) if big else (32, 32)
            w = _cl(torch.randn(cin, cout, 2, 2, generator=g))
            out.append((w, lambda c, w=w, kn=kind == 4: c.get_up(w, kn)))
    return out


def _refresh_twice(h2):
    """Fill a cache, then twice: change every weight in place and ``refresh()``.  After each refresh every buffer must hold the bytes
    of a fresh single prepare of the same weight into a new cache (test_hip_conv.py's
    test_batched_weight_preparation_equals_the_single_calls).  Of an fp16 buffer's 256-byte trailer the words [0] and [3] are the two
    max slots: the batch alternates between them (0 by the single prepare, then 3, then 0 again) while a fresh single prepare always
    uses 0, so those two words hold different bytes by design -- compared are the planes and the trailer words [1] (2^-e_w) and [2] (e_w)."""
    from tomosar2height_amd import grid
    cache, weights = grid.SplitWeightCache(), _mixed_weights(4)
    bufs = [get(cache) for _w, get in weights]
    assert len(cache.entries) == 25 and len({b.data_ptr() for b in bufs}) == 25
    snaps = []
    for rnd in range(2):
        with torch.no_grad():
            for i, (w, _get) in enumerate(weights):                         # scale changes: the fp16 buffers' exponents move
                w.mul_(1.7 + 0.25 * i) if (i + rnd) % 2 else w.add_(0.25 * (i + 1))
        cache.refresh()
        for i, ((_w, get), got) in enumerate(zip(weights, bufs)):
            ref = get(grid.SplitWeightCache())
            assert got.shape == ref.shape
            if h2:
                assert torch.equal(got[:-256], ref[:-256]), (rnd, i)
                assert torch.equal(got[-256:].view(torch.int32)[1:3], ref[-256:].view(torch.int32)[1:3]), (rnd, i)
            else:
                assert torch.equal(got, ref), (rnd, i)
        snaps.append([b.clone() for b in bufs])
    return snaps


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_batched_refresh_of_25_buffers_stays_inside_them(mode, monkeypatch):
    """The seam between the two launches of a 25-buffer refresh and the fp16 trailer's max slot going 0 -> 3 -> 0, over banded
    buffers that start from 0xFF: equal to the single prepares (``_refresh_twice``), to the unguarded run bit for bit (whole
    buffers: both runs make the same sequence of slots), and no band damaged (checked when the block exits)."""
    from tomosar2height_amd import grid
    monkeypatch.setattr(grid, "CONV_PRECISION", mode)
    clean = _refresh_twice(mode == "f16x2")
    torch.cuda.synchronize()
    with guarded_scratch("nan") as g:
        got = _refresh_twice(mode == "f16x2")
    split = [e for e in g.log if e[0] == "ws" and _hit(e[5], (_SPLIT_SITE,))]
    assert len(split) == 25 + 2 * 25, len(split)                            # the cache's buffers and the fresh single prepares
    assert bool((split[0][3][:split[0][4]] == 0xFF).all())                   # (they are banded)
    for rnd in range(2):
        for i, (a, b) in enumerate(zip(got[rnd], clean[rnd])):
            assert torch.equal(a, b), (rnd, i)
