"""GPU: t2h_sample_rows_fwd / _bwd (csrc/bicubic.hip) -- 'bicubic' and 'nearest' sampling on the rows of a tile index, regular or
ragged, with a gather adjoint -- through ``_lib.call`` on the raw entry points, every operand inside a banded buffer of
tests/scratch_guard.py (outputs start as NaN).

Indices at resolution 8 (nbits = 3): three tiles of 1, 37 and 300 rows in one ragged index, with coordinates inside [0, 1)
("inside") or with the full list of resample_ref.points, points outside [0, 1) included ("outside": the build clamps them into
the border cells and keeps their raw coordinates in the sorted rows), and one regular index (B = 2, N = 37).  Planes at
r = 8, 4, 2, 1; C in {1, 5, 32}; both layouts; both modes.

1. forward: the rows of tile b equal t2h_sample_{bicubic,nearest}_fwd on that tile's rows alone, bit for bit;
2. forward and adjoint against the float64 restatement under the bars derived in resample_ref.py (worst err / bar <= 1);
3. adjoint: two calls give equal bits, a tile inside a batch equals the tile's own B = 1 index bit for bit, unreached pixels are +0.0.
"""
import numpy as np
import pytest
import torch

import resample_ref as rr
from scratch_guard import guarded_scratch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, NBITS = 8, 3
SIZES = (1, 37, 300)
PLANES = (8, 4, 2, 1)
CHANNELS = (1, 5, 32)
MODES = {"nearest": 0, "bicubic": 1}
_cache = {}


def room(n):
    from tomosar2height_amd import _lib
    n = max(int(n), 1)
    return _lib.workspace(4 * n, DEV).view(torch.float32)[:n]


def put(a):
    buf = room(a.size)
    if a.size:
        buf[:a.size].copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel()))
    return buf


def to_memory(a, cl):
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if cl else np.ascontiguousarray(a)


def from_memory(buf, shape, cl):
    b, c, h, w = shape
    a = buf[:b * c * h * w].cpu().numpy()
    return a.reshape(b, h, w, c).transpose(0, 3, 1, 2) if cl else a.reshape(b, c, h, w)


def call(name, *args):
    from tomosar2height_amd import _lib
    _lib.call(name, *args, _lib.stream())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def report(entry, case, got, want, bar):
    assert not np.isnan(got).any(), f"{entry} {case}: an output element was never written"
    ratio = rr.worst_ratio(got, want, bar)
    print(f"sample-rows-ratio {entry} {case} {ratio:.4f}")
    return ratio


def cloud(n, sample, inside):
    """float32 [n, 3]: rows of ``rr.points(8, 3, .)``; ``inside``: coordinates outside [0, 1) folded into it."""
    p = rr.points(R, 3, max(n, 37))[sample][:n].copy()
    if inside:
        xy = p[:, :2].astype(np.float64)
        fold = (xy - np.floor(xy)).astype(np.float32)
        fold[fold >= 1.0] = 0.0
        p[:, :2] = np.where((xy >= 0.0) & (xy < 1.0), p[:, :2], fold)
        assert (p[:, :2] >= 0).all() and (p[:, :2] < 1).all()
    return p


def index(kind):
    """dict(tile, spans, clouds, single): the index of a case, the row span of every tile, and every tile's own B = 1 index."""
    if kind in _cache:
        return _cache[kind]
    from tomosar2height_amd.tile import TileIndex
    if kind == "regular":
        clouds = [cloud(37, 0, True), cloud(37, 1, True)]
        tile = TileIndex(torch.from_numpy(np.stack(clouds)).to(DEV), R)
    else:
        clouds = [cloud(n, i % 2, kind == "inside") for i, n in enumerate(SIZES)]
        if kind == "outside":
            clouds[0] = np.asarray([[1.4, 1.0, 0.5]], np.float32)
        tile = TileIndex([torch.from_numpy(c).to(DEV) for c in clouds], R)
        assert tile.ragged and tile.dim == 4 and tile.nbits == NBITS
    bad = sum(int(((c[:, :2] < 0) | (c[:, :2] >= 1)).any(axis=1).sum()) for c in clouds)
    assert tile.out_of_domain() == bad and (bad > 0) == (kind == "outside")
    spans = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    single = [TileIndex(torch.from_numpy(c[None]).to(DEV), R) for c in clouds]
    pts = tile.pts.cpu().numpy()
    for b, one in enumerate(single):        # the sorted rows keep the raw coordinates, tile by tile in the same order
        assert np.array_equal(bits(pts[spans[b]:spans[b + 1], :3]), bits(one.pts.cpu().numpy()))
    _cache[kind] = dict(tile=tile, spans=spans, clouds=clouds, single=single, pts=pts)
    return _cache[kind]


def operands(kind, r, channels):
    """(plane [B, C, r, r], g [rows, C]) float32, seeded by the case."""
    ix = index(kind)
    rng = np.random.default_rng([r, channels, len(kind)])
    return (rng.standard_normal((ix["tile"].B, channels, r, r)).astype(np.float32),
            rng.standard_normal((ix["tile"].n_points, channels)).astype(np.float32))


def reference(kind, r, channels):
    key = ("ref", kind, r, channels)
    if key not in _cache:
        ix = index(kind)
        plane, g = operands(kind, r, channels)
        out = []
        for b in range(ix["tile"].B):
            s, e = ix["spans"][b], ix["spans"][b + 1]
            p, gb, pl = ix["pts"][None, s:e], g[None, s:e], plane[b:b + 1]
            near_grad, near_mag, near_count = rr.sample_nearest_adjoint(gb, p, r)
            bar_adj, reach = rr.sample_bicubic_adjoint_bar(gb, p, r)
            out.append(dict(y=rr.sample_bicubic(pl, p)[0], bar=rr.sample_bicubic_bar(pl, p)[0], near=rr.sample_nearest(pl, p)[0],
                            gp=rr.sample_bicubic_adjoint(gb, p, r)[0], bar_gp=bar_adj[0], reach=reach[0],
                            near_gp=near_grad[0], bar_near_gp=(rr.gamma(near_count)[:, None] * near_mag)[0], near_count=near_count[0]))
        _cache[key] = out
    return _cache[key]


def rows_args(tile):
    return tile.pts.data_ptr(), tile.dim, tile.off0.data_ptr(), tile.B, tile.N, tile.nbits


CASES = [(kind, r) for kind in ("inside", "regular", "outside") for r in PLANES]


@pytest.mark.parametrize("kind,r", [c for c in CASES if c[0] != "outside"], ids=lambda v: str(v))
def test_forward_equals_the_single_tile_entry_points_bit_for_bit(kind, r):
    ix = index(kind)
    tile, spans = ix["tile"], ix["spans"]
    rows = tile.n_points
    for channels in CHANNELS:
        plane, _ = operands(kind, r, channels)
        for cl in (0, 1):
            for mode, m in MODES.items():
                with guarded_scratch(fill="nan"):
                    pl = put(to_memory(plane, cl))
                    out, alone = room((rows + 3) * channels), room(rows * channels)
                    call("t2h_sample_rows_fwd", pl.data_ptr(), *rows_args(tile), r, channels, cl, m, out.data_ptr())
                    for b in range(tile.B):
                        s, e = int(spans[b]), int(spans[b + 1])
                        call(f"t2h_sample_{mode}_fwd", pl[b * channels * r * r:].data_ptr(), tile.pts[s:e].data_ptr(), tile.dim, 1, e - s, r,
                             channels, cl, alone[s * channels:].data_ptr())
                    got, want = out.cpu().numpy(), alone.cpu().numpy()
                tag = f"{kind} r={r} C={channels} cl={cl} {mode}"
                assert not np.isnan(want).any(), tag
                assert np.array_equal(bits(got[:rows * channels]), bits(want)), tag
                assert np.isnan(got[rows * channels:]).all(), f"{tag}: rows past the index were written"


@pytest.mark.parametrize("kind,r", CASES, ids=lambda v: str(v))
def test_forward_and_adjoint_against_float64_and_the_adjoint_is_deterministic_per_tile(kind, r):
    ix = index(kind)
    tile, spans = ix["tile"], ix["spans"]
    rows, nb = tile.n_points, tile.B
    worst = 0.0
    for channels in CHANNELS:
        plane, g = operands(kind, r, channels)
        ref = reference(kind, r, channels)
        for cl in (0, 1):
            for mode, m in MODES.items():
                tag = f"{kind} r={r} C={channels} cl={cl} {mode}"
                n_plane = nb * channels * r * r
                with guarded_scratch(fill="nan"):
                    pl, gd = put(to_memory(plane, cl)), put(g)
                    out, first, second = room(rows * channels), room(n_plane), room(n_plane)
                    alone = room(n_plane)
                    call("t2h_sample_rows_fwd", pl.data_ptr(), *rows_args(tile), r, channels, cl, m, out.data_ptr())
                    call("t2h_sample_rows_bwd", gd.data_ptr(), *rows_args(tile), r, channels, cl, m, first.data_ptr())
                    call("t2h_sample_rows_bwd", gd.data_ptr(), *rows_args(tile), r, channels, cl, m, second.data_ptr())
                    for b, one in enumerate(ix["single"]):              # the tile's own B = 1 index (regular, dim = 3)
                        call("t2h_sample_rows_bwd", gd[int(spans[b]) * channels:].data_ptr(), *rows_args(one), r, channels, cl, m,
                             alone[b * channels * r * r:].data_ptr())
                    assert torch.equal(first.view(torch.int32), second.view(torch.int32)), f"{tag}: two runs differ"
                    assert torch.equal(first.view(torch.int32), alone.view(torch.int32)), f"{tag}: a tile differs from its own index"
                    got = out.cpu().numpy().reshape(rows, channels)
                    grad = from_memory(first, (nb, channels, r, r), cl)
                assert not np.isnan(grad).any(), f"{tag}: a plane-gradient element was never written"
                for b in range(nb):
                    s, e = int(spans[b]), int(spans[b + 1])
                    t = f"{tag} tile={b}"
                    if mode == "bicubic":
                        worst = max(worst, report("t2h_sample_rows_fwd", t, got[s:e], ref[b]["y"], ref[b]["bar"]))
                        worst = max(worst, report("t2h_sample_rows_bwd", t, grad[b], ref[b]["gp"], ref[b]["bar_gp"]))
                        unreached = ref[b]["reach"] == 0
                    else:
                        assert np.array_equal(bits(got[s:e]), bits(ref[b]["near"])), f"t2h_sample_rows_fwd {t}"
                        worst = max(worst, report("t2h_sample_rows_bwd", t, grad[b], ref[b]["near_gp"], ref[b]["bar_near_gp"]))
                        unreached = ref[b]["near_count"] == 0
                    assert not bits(grad[b][:, unreached]).any(), f"{t}: an unreached pixel is not +0.0"
    assert worst <= 1.0


def test_zero_rows():
    """A regular batch of no rows: T2H_OK, the forward output untouched, the plane gradient all +0.0."""
    with guarded_scratch(fill="nan"):
        pl, pts, off0 = room(2 * 5 * 16), room(4), room(2 * 64 + 1)
        out, grad = room(8), room(2 * 5 * 16)
        for m in (0, 1):
            call("t2h_sample_rows_fwd", pl.data_ptr(), pts.data_ptr(), 3, off0.data_ptr(), 2, 0, NBITS, 4, 5, 0, m, out.data_ptr())
            call("t2h_sample_rows_bwd", out.data_ptr(), pts.data_ptr(), 3, off0.data_ptr(), 2, 0, NBITS, 4, 5, 0, m, grad.data_ptr())
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()) and not bool(grad.view(torch.int32).any())
            grad.fill_(float("nan"))


def test_refusals_launch_nothing():
    from tomosar2height_amd import _lib
    ix = index("inside")
    tile = ix["tile"]
    with guarded_scratch(fill="nan"):
        pl, out = room(3 * 5 * 64), room(tile.n_points * 5)
        for entry in ("t2h_sample_rows_fwd", "t2h_sample_rows_bwd"):
            for args, message in (((*rows_args(tile), 8, 5, 0, 2), "mode must be"), ((*rows_args(tile), 16, 5, 0, 1), "power of two"),
                                  ((*rows_args(tile)[:2], None, *rows_args(tile)[3:], 8, 5, 0, 1), "null pointer"),
                                  ((tile.pts.data_ptr(), 2, *rows_args(tile)[2:], 8, 5, 0, 1), "dim=2")):
                with pytest.raises(_lib.T2HLibraryError, match=message):
                    call(entry, pl.data_ptr(), *args, out.data_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isnan(pl).all()) and bool(torch.isnan(out).all())
