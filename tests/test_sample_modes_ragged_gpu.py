"""GPU: sample_mode = 'bicubic' / 'nearest' on RAGGED tile indices through the public path -- ``ops.sample_plane_mode``, an ALTO
level constructed with the mode, and the Trainer's default (coalescing) path with such levels.  The ragged path runs on
t2h_sample_rows_fwd / _bwd (csrc/bicubic.hip): its adjoint is a gather in a fixed order, so a tile inside a batch equals the
tile alone bit for bit and a training window is reproducible bit for bit."""
import numpy as np
import pytest
import torch

from detinit import det_init_, synth_cloud

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _clouds(sizes, seed):
    return [torch.rand(1, n, 3, generator=torch.Generator().manual_seed(seed + i)).to(DEV) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("mode", ["bicubic", "nearest"])
def test_sample_plane_mode_on_a_ragged_index_equals_every_tile_alone(mode, channels_last):
    from tomosar2height_amd import ops
    from tomosar2height_amd.tile import TileIndex
    reso, r, channels = 16, 8, 5
    clouds = _clouds((50, 300, 1), 40)
    tile = TileIndex(clouds, reso)
    assert tile.ragged
    gen = torch.Generator().manual_seed(41)
    plane = torch.randn(3, channels, r, r, generator=gen).to(DEV)
    g = torch.randn(tile.n_points, channels, generator=gen).to(DEV)

    def run(t, p, gout, fn=lambda t, p: ops.sample_plane_mode(t, p, mode)):
        p = p.clone()
        if channels_last:
            p = p.contiguous(memory_format=torch.channels_last)
        p.requires_grad_(True)
        out = fn(t, p)
        out.backward(gout)
        assert tuple(p.grad.shape) == tuple(p.shape)
        assert p.grad.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        return out.detach(), p.grad

    out, grad = run(tile, plane, g)
    assert tuple(out.shape) == (tile.n_points, channels) and bool(torch.isfinite(out).all())
    again = run(tile, plane, g)
    assert torch.equal(out.view(torch.int32), again[0].view(torch.int32)) and torch.equal(grad.view(torch.int32), again[1].view(torch.int32))
    for b, c in enumerate(clouds):
        s, e = tile.starts[b], tile.starts[b + 1]
        own = TileIndex([c], reso)                                         # the tile's own (one-cloud) ragged index
        o, gr = run(own, plane[b:b + 1], g[s:e])
        assert torch.equal(out[s:e].view(torch.int32), o.view(torch.int32)), (mode, b)
        assert torch.equal(grad[b:b + 1].contiguous().view(torch.int32), gr.contiguous().view(torch.int32)), (mode, b)
        regular = TileIndex(c, reso)                                       # the same rows as a regular B = 1 index, new entry direct
        o, gr = run(regular, plane[b:b + 1], g[s:e], fn=lambda t, p: ops._SampleRows.apply(p, t, mode))
        assert torch.equal(out[s:e].view(torch.int32), o.view(torch.int32)), (mode, b)
        assert torch.equal(grad[b:b + 1].contiguous().view(torch.int32), gr.contiguous().view(torch.int32)), (mode, b)


@pytest.mark.parametrize("mode", ["bicubic", "nearest"])
def test_alto_level_with_a_sample_mode_on_a_ragged_index(mode):
    """``DownConv(..., sample_mode=m)`` on three clouds of different sizes in one index: every tile's raster against the same level
    evaluated with torch's operators on that tile (tests/test_operator_seam.py's bicubic level, its bar)."""
    from tomosar2height_amd import ops
    from tomosar2height_amd.encoder.alto import DownConv
    from tomosar2height_amd.tile import TileIndex
    torch.manual_seed(5)
    lvl = DownConv(32, 32, 0, False, depth=3, sample_mode=mode).to(DEV)
    lvl.channels_last = True
    sizes = (500, 3000, 1200)
    clouds = _clouds(sizes, 60)
    plane = torch.randn(3, 32, 32, 32, generator=torch.Generator().manual_seed(7)).to(DEV).contiguous(memory_format=torch.channels_last)
    c_last = [torch.randn(1, n, 32, generator=torch.Generator().manual_seed(80 + i)).to(DEV) for i, n in enumerate(sizes)]
    tile = TileIndex(clouds, 32)
    c_sorted = torch.cat([c_last[b][0][tile.perm[tile.starts[b]:tile.starts[b + 1]].long()] for b in range(3)])
    with torch.no_grad():
        pooled, raster, g, c = lvl(tile, plane, None, c_sorted, None)
        x = torch.relu(lvl.conv2(torch.relu(lvl.conv1(plane))))
        for b, cloud in enumerate(clouds):
            n = sizes[b]
            vgrid = 2.0 * cloud[..., :2][:, :, None] - 1.0
            s = torch.nn.functional.grid_sample(x[b:b + 1], vgrid, padding_mode="border", align_corners=True, mode=mode)
            cc = lvl.fc_comm(s.squeeze(-1).transpose(1, 2)) + lvl.fc_c(c_last[b])
            idx = ops.coordinate2index(cloud, 32)
            want = torch.zeros(1, 32, 32 * 32, device=DEV)
            cnt = torch.zeros(1, 1, 32 * 32, device=DEV)
            want.scatter_add_(2, idx.expand(-1, 32, -1), cc.transpose(1, 2))
            cnt.scatter_add_(2, idx, torch.ones(1, 1, n, device=DEV))
            want = (want / cnt.clamp_min(1)).reshape(1, 32, 32, 32)
            err = ((raster[b:b + 1] - want).abs().max() / want.abs().max()).item()
            print(f"alto-level-ragged {mode} tile={b} {err:.3e}")
            assert err <= 2e-5, (mode, b, err)


def test_trainer_default_path_with_bicubic_levels_is_reproducible():
    """Four tiles of different N handed to ``train_step`` one by one under the default coalescing (one ragged micro-batch), ALTO
    levels with sample_mode='bicubic' set by hand: the window ends in one optimizer step, everything is finite, and the same
    window from the same initial weights gives the same parameters bit for bit (the adjoint adds in a fixed order).

    A Trainer coalesces only once its gradient bucket exists: the first tile of its life is issued alone, as a regular [1, N, 3]
    batch, and regular batches keep the atomic adjoint.  So the window under test is preceded by the same four tiles at learning
    rate 0, which lays out the bucket and leaves every weight as it was (asserted bit for bit); the window under test then starts
    from the initial weights and all four of its tiles form one ragged micro-batch."""
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.encoder.alto import _PointGridLevel
    from tomosar2height_amd.trainer import Trainer
    cfg = berlin_config()
    cfg.model.encoder_kwargs.unet_kwargs.depth = 4
    tiles = [{"inputs": synth_cloud(n, seed=500 + i).to(DEV),
              "dsm": (torch.rand(1, 512, 512, generator=torch.Generator().manual_seed(i)) * 30).to(DEV)}
             for i, n in enumerate((6000, 4100, 7300, 5003))]

    def run():
        model = det_init_(TomoSAR2Height(cfg), seed=21).to(DEV)
        model.set_channels_last(True)
        levels = [m for m in model.modules() if isinstance(m, _PointGridLevel)]
        assert levels
        for m in levels:
            m.sample_mode = "bicubic"
        optimizer = torch.optim.SGD(model.parameters(), lr=0.0)
        tr = Trainer(model, optimizer, device=DEV, optimize_every=4, use_cloud=True)
        assert tr.coalesce_tiles == 4
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        assert [tr.train_step(t) for t in tiles] == [False, False, False, True]          # lays out the bucket, changes nothing
        assert all(torch.equal(before[k].view(torch.int32), p.detach().view(torch.int32)) for k, p in model.named_parameters())
        for group in optimizer.param_groups:
            group["lr"] = 1e-3
        ended = []
        for t in tiles:
            ended.append(tr.train_step(t))
            assert len(tr._coalesced) == (len(ended) if len(ended) < 4 else 0)             # held until the fourth: one micro-batch
        torch.cuda.synchronize()
        assert ended == [False, False, False, True] and tr.accumulated_steps == 0
        assert np.isfinite(float(tr.last_avg_loss))
        after = {k: p.detach().clone() for k, p in model.named_parameters()}
        assert all(bool(torch.isfinite(p).all()) for p in after.values())
        assert any(not torch.equal(before[k], after[k]) for k in after)
        return after

    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
