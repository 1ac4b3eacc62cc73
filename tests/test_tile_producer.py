"""Tile producer (reference dataset.py:229-278): oracle vs the fixture built from the reference's own
utility functions (CPU) and the device kernels vs both (GPU).  Selected indices bit exact; coordinates within one
float32 ulp (the reference multiplies by an inverted 4x4 matrix, the restatements use the closed form)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import producer_ref

Z_SPAN = 156.5 - (-33.7)


def _ulp_close(got, want, min_equal=0.99):
    """one float32 ulp, or 1e-7 absolute near zero (the reference's matrix form leaves ~1e-17 instead of an exact 0
    at the z-min point), and bit-equal for > 99 % of the values (`min_equal`: a statistic over a tile; a chunk of three
    points that all sit one float64 step from an edge has none, and passes 0)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=1.2e-7, atol=1e-7)
    if min_equal:
        assert (got == want).mean() > min_equal


def test_oracle_matches_reference_fixture():
    g = load_golden("tile_producer")
    assert int(g["n_3"]) == 0 and int(g["n_0"]) > 100
    for i in range(4):
        idx, pts, z_shift = producer_ref.produce_tile(g["chunk"], g["anchors"][i], z_span=Z_SPAN)
        if int(g[f"n_{i}"]) == 0:
            assert idx.size == 0
            continue
        assert np.array_equal(idx, g[f"index_{i}"])
        if i == 0:
            assert 0 not in idx and 1 not in idx and 2 in idx                  # points ON the window edge are excluded
        _ulp_close(pts, g[f"inputs_{i}"])
        assert z_shift == float(g[f"zshift_{i}"][0])


@pytest.mark.gpu
def test_device_producer_matches_fixture_and_feeds_the_model():
    from tomosar2height_amd.producer import TileProducer
    g = load_golden("tile_producer")
    dev = torch.device("cuda:0")
    prod = TileProducer(torch.from_numpy(g["chunk"]).to(dev))
    for i in range(4):
        tile = prod.crop(g["anchors"][i], with_index=True)
        if int(g[f"n_{i}"]) == 0:
            assert not bool(tile["is_valid"][0]) and "inputs" not in tile
            continue
        assert bool(tile["is_valid"][0])
        assert np.array_equal(tile["index"].cpu().numpy(), g[f"index_{i}"])
        _ulp_close(tile["inputs"][0].cpu().numpy(), g[f"inputs_{i}"])
        assert tile["z_shift"].item() == float(g[f"zshift_{i}"][0])
        assert tile["inputs"].shape[0] == 1 and tile["inputs"].dtype == torch.float32
    # a large random chunk against the oracle, then straight into the tile index
    rng = np.random.RandomState(0)
    chunk = np.stack([rng.uniform(1000, 3000, 300000), rng.uniform(5000, 7000, 300000), rng.uniform(0, 80, 300000)], 1)
    prod = TileProducer(torch.from_numpy(chunk).to(dev))
    tile = prod.crop((1500.0, 5600.0), with_index=True)
    idx, pts, _ = producer_ref.produce_tile(chunk, (1500.0, 5600.0), z_span=Z_SPAN)
    assert np.array_equal(tile["index"].cpu().numpy(), idx)
    _ulp_close(tile["inputs"][0].cpu().numpy(), pts)
    from tomosar2height_amd.tile import TileIndex
    t = TileIndex(tile["inputs"], 256)
    assert t.out_of_domain() == 0 and t.n_points == idx.size


AUG = [(r, f) for r in range(4) for f in (-1, 0, 1)]


def test_oracle_augmentation_matches_reference_fixture():
    """flip_mat @ rot_mat on the points and rot90 / flip on the rasters (dataset.py:253-328) against the fixture composed
    from the reference's own utilities."""
    g = load_golden("tile_producer_aug")
    row, col, ph, pw = (int(v) for v in g["row_col_shape"])
    for rot, flip in AUG:
        tag = f"r{rot}_f{flip + 1}"
        idx, pts, _ = producer_ref.produce_tile(g["chunk"], g["anchor"], z_span=Z_SPAN, rot_times=rot, flip_dim=flip)
        assert np.array_equal(idx, g[f"index_{tag}"]), tag
        _ulp_close(pts, g[f"inputs_{tag}"])
        assert np.array_equal(producer_ref.raster_patch(g["dsm_data"][None], row, col, (ph, pw), rot, flip), g[f"dsm_{tag}"]), tag
        assert np.array_equal(producer_ref.raster_patch(g["image"], row, col, (ph, pw), rot, flip), g[f"image_{tag}"]), tag


def _near_edge_rows(chunk, anchor, rows, patch=512.0):
    """the rows of `rows` whose float64 normalised x or y lies within 2^-24 of 0 or 1 (the same under every quarter turn and
    flip, which only swap and mirror the two axes): there, and only there, the reference's inverted 4 x 4 matrix (quarter-turn
    cos = 6e-17) and the closed form may round to different sides of the float32 re-crop."""
    n = (np.asarray(chunk, np.float64)[rows, :2] - (np.asarray(anchor, np.float64) + patch / 2)) / patch + 0.5
    near = (np.minimum(np.abs(n), np.abs(1.0 - n)) <= 2.0 ** -24).any(1)
    return set(int(r) for r in np.asarray(rows)[near])


def _against_reference_fixture(idx, pts, want_idx, want_pts, allowed, tag, min_equal=0.99):
    """index sets equal except at `allowed` rows; coordinates of the common rows within `_ulp_close`.  Returns the rows
    that disagree."""
    idx, want_idx = np.asarray(idx).astype(np.int64), np.asarray(want_idx).astype(np.int64)
    differ = set(int(r) for r in np.setxor1d(idx, want_idx))
    assert differ <= allowed, f"{tag}: rows {sorted(differ - allowed)} disagree with the reference away from a planted near-edge row"
    _, ia, ib = np.intersect1d(idx, want_idx, assume_unique=True, return_indices=True)
    assert np.array_equal(ia, np.sort(ia)) and np.array_equal(ib, np.sort(ib))           # both keep the chunk's order
    if ia.size:
        _ulp_close(np.asarray(pts)[ia], want_pts[ib], min_equal)
    return differ


def test_oracle_matches_reference_edges_fixture():
    """The oracle at the edges of both crops (tests/golden/make_golden.py:tile_producer_edges_fixture): negative z_shift carried
    by a point the re-crop may drop, points one float64 step inside each window edge, points on the edges, -0.0 beside +0.0,
    and a chunk whose re-crop is empty.  z_shift equal; indices equal except -- at most -- at planted near-edge rows."""
    g = load_golden("tile_producer_edges")
    chunk, anchor = g["chunk"], g["anchor"]
    assert chunk[:, 2].min() == -33.0 and (chunk[:, 2] < 0).sum() > 500 and chunk[:, 2].max() > 70
    assert np.signbit(chunk[g["zero_rows"][0], 2]) and not np.signbit(chunk[g["zero_rows"][1], 2])
    for prefix, cloud, rows in (("", chunk, g["near_rows"]), ("tiny_", g["tiny_chunk"], g["tiny_near_rows"])):
        allowed = _near_edge_rows(cloud, anchor, rows)
        assert allowed == set(int(r) for r in rows)                                       # every planted row IS near an edge
        first = g[prefix + "first_index"]
        assert set(int(r) for r in rows) <= set(int(r) for r in first)                    # strictly inside in float64
        removed = []
        for rot, flip in AUG:
            tag = f"{prefix}r{rot}_f{flip + 1}"
            idx, pts, z_shift = producer_ref.produce_tile(cloud, anchor, z_span=Z_SPAN, rot_times=rot, flip_dim=flip)
            assert z_shift == float(g[prefix + "zshift"][0]), tag
            differ = _against_reference_fixture(idx, pts, g[f"{prefix}index_{tag[len(prefix):]}"],
                                                g[f"{prefix}inputs_{tag[len(prefix):]}"], allowed, tag,
                                                min_equal=0.99 if prefix == "" else 0)
            print(f"{tag}: oracle keeps {idx.size} of {first.size} first-crop points; rows disagreeing with the reference: "
                  f"{sorted(differ)}")
            assert set(first) - set(idx) <= allowed                                       # the re-crop only ever removes planted rows
            removed.append(first.size - idx.size)
        assert min(removed) > 0 if prefix == "" else min(removed) == 0 and max(removed) == 3
    assert not np.isin(g["on_edge_rows"], g["first_index"]).any()                         # ON an edge: outside the strict crop
    assert int(g["zmin_row"][0]) in g["first_index"] and int(g["zmin_row"][0]) not in g["index_r0_f0"]
    assert any(int(g["zmin_row"][0]) in g[f"index_r{r}_f{f + 1}"] for r, f in AUG)          # z_shift set by a dropped point
    assert g["tiny_index_r0_f0"].size == 0 and g["tiny_first_index"].size == 3


@pytest.mark.gpu
def test_device_augmented_tiles_match_fixture():
    from tomosar2height_amd.producer import RasterPatcher, TileProducer, TileSource
    g = load_golden("tile_producer_aug")
    dev = torch.device("cuda:0")
    row, col, ph, pw = (int(v) for v in g["row_col_shape"])
    prod = TileProducer(torch.from_numpy(g["chunk"]).to(dev))
    # a raster whose pixel (row, col) holds the window's bottom-left corner: 32 m pixels, 16 x 16 pixel patches
    px = 32.0
    left, top = float(g["anchor"][0]) - col * px, float(g["anchor"][1]) + (row + 1) * px
    dsm = RasterPatcher(torch.from_numpy(g["dsm_data"]).to(dev), left, top, (px, px))
    img = RasterPatcher(torch.from_numpy(g["image"]).to(dev), left, top, (px, px))
    assert dsm.patch_shape == (ph, pw) and dsm.query_col_row(float(g["anchor"][0]) + px / 2, float(g["anchor"][1]) + px / 2) == (col, row)
    for rot, flip in AUG:
        tag = f"r{rot}_f{flip + 1}"
        tile = prod.crop(g["anchor"], with_index=True, rot_times=rot, flip_dim=flip)
        assert np.array_equal(tile["index"].cpu().numpy(), g[f"index_{tag}"]), tag
        _ulp_close(tile["inputs"][0].cpu().numpy(), g[f"inputs_{tag}"])
        assert np.array_equal(dsm.patch(g["anchor"], rot, flip).cpu().numpy(), g[f"dsm_{tag}"]), tag
        assert np.array_equal(img.patch(g["anchor"], rot, flip).cpu().numpy(), g[f"image_{tag}"]), tag

    class _Fixed:                         # the augmentation draw of dataset.py:253-263, pinned
        def __init__(self, seq): self.seq = list(seq)
        def choice(self, n): return self.seq.pop(0)
    src = TileSource(prod, dsm, img, flip_augm=True, rotate_augm=True, rng=_Fixed([3, 1]))     # rot 3, flip key index 1 -> 0
    t = src.get(g["anchor"])
    assert (t["rotate"], t["flip"]) == (3, 0) and t["dsm"].shape == (1, ph, pw) and t["image"].shape == (1, 3, ph, pw)
    assert np.array_equal(t["dsm"].cpu().numpy(), g["dsm_r3_f1"]) and np.array_equal(t["image"][0].cpu().numpy(), g["image_r3_f1"])
    # the same tile produced on a side stream (the prefetching form: the host's point-count read waits for the crop only,
    # not for a training step running on the main stream) -- while the main stream is kept busy -- is bit-identical
    busy = torch.randn(4096, 4096, device=dev)
    for _ in range(4):
        busy = busy @ busy * 1e-4
    src2 = TileSource(prod, dsm, img, flip_augm=True, rotate_augm=True, rng=_Fixed([3, 1]), stream=torch.cuda.Stream())
    t2 = src2.get(g["anchor"])
    for k in ("inputs", "dsm", "image"):
        assert torch.equal(t2[k], t[k]), k
    assert (t2["rotate"], t2["flip"]) == (3, 0)
    with pytest.raises(RuntimeError, match="leave the"):
        dsm.patch((left - 10 * px, float(g["anchor"][1])))


# ---- the crop kernels at their edges: every expected value below is the oracle's, numpy's or the reference fixture's ---------
# NaN coordinates are out of scope: the reference's torch.min would propagate a NaN z into z_shift, the kernel's integer key
# does not -- a known difference that no test here covers.
ANCHOR = (1500.0, 5600.0)
CROP_TILE = 2048                           # points per workgroup of the count / scatter kernels (csrc/tile_producer.hip)


def _inside(x):
    """the float64 next to window edge `x` on the inner side: kept by the first crop, 0.0f / 1.0f (or 2^-51) after the cast"""
    lo_edge = x in ANCHOR
    return np.nextafter(x, np.inf if lo_edge else -np.inf)


def _seeded_chunk(p, seed, lo=(1000.0, 5000.0), hi=(3000.0, 7000.0), z=(-30.0, 80.0)):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(lo[0], hi[0], p), rng.uniform(lo[1], hi[1], p), rng.uniform(z[0], z[1], p)], 1)


def _producer(chunk):
    from tomosar2height_amd.producer import TileProducer
    return TileProducer(torch.from_numpy(np.ascontiguousarray(chunk, np.float64)).to("cuda:0"))


def _crop_vs_oracle(prod, chunk, anchor=ANCHOR, rot=0, flip=-1, min_equal=0.99):
    """one device crop against the oracle: validity, shapes, the index bit exact, coordinates `_ulp_close`, z_shift `==`"""
    tile = prod.crop(anchor, with_index=True, rot_times=rot, flip_dim=flip)
    idx, pts, z_shift = producer_ref.produce_tile(chunk, anchor, z_span=Z_SPAN, rot_times=rot, flip_dim=flip)
    assert bool(tile["is_valid"][0]) == (idx.size > 0) and tile["is_valid"].shape == (1,)
    assert np.array_equal(tile["min_bound"].numpy(), np.asarray(anchor, np.float64))
    assert np.array_equal(tile["max_bound"].numpy(), np.asarray(anchor, np.float64) + 512.0)
    if idx.size == 0:
        assert "inputs" not in tile and "index" not in tile and "z_shift" not in tile
        return tile, idx, pts, z_shift
    assert tile["inputs"].shape == (1, idx.size, 3) and tile["inputs"].dtype == torch.float32
    assert tile["index"].shape == (idx.size,) and tile["z_shift"].shape == (1,) and tile["z_shift"].dtype == torch.float64
    assert np.array_equal(tile["index"].cpu().numpy(), idx)
    _ulp_close(tile["inputs"][0].cpu().numpy(), pts, min_equal)
    assert tile["z_shift"].item() == z_shift
    return tile, idx, pts, z_shift


def _raw_crop(chunk, anchor=ANCHOR, rot=0, flip=-1):
    """the two C entry points on buffers of the test's own, pre-filled with junk: (count, z_shift) as the host reads them"""
    from tomosar2height_amd import _lib
    dev = torch.device("cuda:0")
    p = chunk.shape[0]
    pts = torch.from_numpy(np.ascontiguousarray(chunk, np.float64)).to(dev) if p else torch.zeros(1, 3, dtype=torch.float64, device=dev)
    out = torch.full((max(p, 1), 3), -7.0, dtype=torch.float32, device=dev)
    count = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    z = torch.full((1,), 1.5, dtype=torch.float64, device=dev)
    nbytes = _lib.ws_bytes("t2h_tile_crop_workspace_bytes", p)
    ws = _lib.workspace(nbytes, dev)
    _lib.call("t2h_tile_crop_normalise_aug", _lib.ptr(pts), p, anchor[0], anchor[1], anchor[0] + 512.0, anchor[1] + 512.0, 512.0, 512.0,
              Z_SPAN, rot, flip, _lib.ptr(out), 0, _lib.ptr(count), _lib.ptr(z), _lib.ptr(ws), nbytes, _lib.stream())
    _lib.call("t2h_tile_crop_finish", _lib.ptr(z), _lib.stream())
    return int(count.item()), float(z.item())


@pytest.mark.gpu
def test_device_crop_matches_oracle_and_reference_on_the_edges_fixture():
    """All 12 augmentations of the edges fixture: device == oracle everywhere, planted rows included (they share the closed
    form); device vs the reference fixture under the cap of `test_oracle_matches_reference_edges_fixture`."""
    g = load_golden("tile_producer_edges")
    for prefix, cloud, rows in (("", g["chunk"], g["near_rows"]), ("tiny_", g["tiny_chunk"], g["tiny_near_rows"])):
        prod = _producer(cloud)
        allowed = _near_edge_rows(cloud, g["anchor"], rows)
        for rot, flip in AUG:
            tag = f"r{rot}_f{flip + 1}"
            tile, idx, _, _ = _crop_vs_oracle(prod, cloud, g["anchor"], rot, flip, min_equal=0.99 if prefix == "" else 0)
            if idx.size == 0:
                assert set(int(r) for r in g[f"{prefix}index_{tag}"]) <= allowed, tag
                continue
            assert tile["z_shift"].item() == float(g[prefix + "zshift"][0]), tag
            _against_reference_fixture(tile["index"].cpu().numpy(), tile["inputs"][0].cpu().numpy(), g[f"{prefix}index_{tag}"],
                                       g[f"{prefix}inputs_{tag}"], allowed, prefix + tag, min_equal=0.99 if prefix == "" else 0)


def _planted_ends(chunk):
    """edge points in rows 0-2 and in the last three rows; row 0 carries the global z minimum"""
    p = chunk.shape[0]
    chunk[0] = (_inside(ANCHOR[0] + 512.0), 5800.5, -33.0)
    chunk[1] = (1700.25, _inside(ANCHOR[1]), 12.0)
    chunk[2] = (ANCHOR[0], 5900.0, -32.0)                                        # ON the edge: never kept
    chunk[p - 3] = (1900.75, _inside(ANCHOR[1] + 512.0), 40.0)
    chunk[p - 2] = (_inside(ANCHOR[0]), 6000.0, -0.0)
    chunk[p - 1] = (1800.0, 6100.0, 79.5)                                        # plainly inside: the very last row is kept
    return chunk


@pytest.mark.gpu
@pytest.mark.parametrize("rot,flip", [(0, -1), (1, 0), (2, 1)])
def test_device_crop_scan_with_two_counts_per_thread(rot, flip):
    """P = 2048 * 257 + 5: 258 block counts, so each scan thread owns two (`per` = 2) and the last block holds five points."""
    p = CROP_TILE * 257 + 5
    chunk = _planted_ends(_seeded_chunk(p, 21))
    tile, idx, _, z_shift = _crop_vs_oracle(_producer(chunk), chunk, rot=rot, flip=flip)
    first = np.nonzero((chunk[:, 0] > 1500) & (chunk[:, 0] < 2012) & (chunk[:, 1] > 5600) & (chunk[:, 1] < 6112))[0]
    assert z_shift == -33.0 and idx[-1] == p - 1 and 0 < first.size - idx.size <= 4 and 2 not in idx
    assert (idx >= CROP_TILE * 257).sum() >= 1 and idx.size > 30000


@pytest.mark.gpu
def test_device_crop_scan_with_three_counts_per_thread_exact_offsets():
    """P = 2048 * 600 (`per` = 3): kept points only in block 300 (the first of scan thread 100's three) and in the last block
    (the last of thread 199's): the scatter offsets of the last block are exactly block 300's total."""
    p = CROP_TILE * 600
    chunk = _seeded_chunk(p, 22, lo=(100.0, 100.0), hi=(900.0, 900.0))           # nothing near the window
    inside = _seeded_chunk(1037, 23, lo=(1500.0, 5600.0), hi=(2012.0, 6112.0))
    rows = np.concatenate([CROP_TILE * 300 + np.sort(np.random.RandomState(24).choice(CROP_TILE, 37, replace=False)),
                           CROP_TILE * 599 + np.sort(np.random.RandomState(25).choice(CROP_TILE, 1000, replace=False))])
    chunk[rows] = inside
    prod = _producer(chunk)
    for rot, flip in ((0, -1), (3, 0)):
        _, idx, _, _ = _crop_vs_oracle(prod, chunk, rot=rot, flip=flip)
        assert np.array_equal(idx, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0, 1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097])
def test_device_crop_sizes(p):
    """Partial waves, partial and exactly full 2048-point tiles, one point more; the count kernel walks a tile as (item, thread),
    the scatter kernel as (wave, item, lane)."""
    half = 106.0                                                                  # 512^2 / 724^2: the window keeps about half
    chunk = _seeded_chunk(4097, 31, lo=(1500.0 - half, 5600.0 - half), hi=(2012.0 + half, 6112.0 + half))[:p]
    _, idx, _, _ = _crop_vs_oracle(_producer(chunk), chunk, min_equal=0.99 if p >= 63 else 0)
    if p >= 63:
        assert 0.3 < idx.size / p < 0.7
    if p == 0:
        import math
        count, z = _raw_crop(chunk)
        assert count == 0 and math.isnan(z)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_negative", "mixed", "signed_zeros", "minimum_outside"])
def test_device_crop_z_minimum_key(kind):
    """The order-preserving integer image of z (negative doubles take their own branch): z_shift is numpy's minimum over the
    FIRST crop; a smaller z outside the window is ignored."""
    p = 5000
    z = {"all_negative": (-33.0, -1.0), "mixed": (-20.0, 60.0), "signed_zeros": (0.5, 50.0), "minimum_outside": (-10.0, 50.0)}[kind]
    chunk = _seeded_chunk(p, 41, z=z)
    if kind == "signed_zeros":
        chunk[2500], chunk[2501] = (1760.0, 5860.0, -0.0), (1761.0, 5861.0, 0.0)
    if kind == "minimum_outside":
        chunk[1234] = (1400.0, 5800.0, -33.5)
    first = (chunk[:, 0] > 1500) & (chunk[:, 0] < 2012) & (chunk[:, 1] > 5600) & (chunk[:, 1] < 6112)
    tile, idx, _, _ = _crop_vs_oracle(_producer(chunk), chunk)
    assert first.sum() > 200 and tile["z_shift"].item() == chunk[first, 2].min()
    if kind in ("all_negative", "mixed"):
        assert tile["z_shift"].item() < 0.0
    if kind == "minimum_outside":
        assert chunk[:, 2].min() == -33.5 < tile["z_shift"].item() and 1234 not in idx
    if kind == "signed_zeros":
        assert tile["z_shift"].item() == 0.0                                      # either zero: the sign bit is not asserted
        zn = tile["inputs"][0, :, 2].cpu().numpy()[np.searchsorted(idx, [2500, 2501])]
        assert zn[0] == zn[1] == 0.0


@pytest.mark.gpu
def test_device_crop_recrop_empties_the_tile():
    """The fixture's tiny chunk: three first-crop survivors, all cast onto 1.0f, so the re-crop leaves nothing.  The device
    reports `is_valid` false with count 0.  (The reference would return an empty but "valid" tile here: dataset.py:235 tests the
    first crop only.)  z_shift is still the finite minimum of the first crop."""
    g = load_golden("tile_producer_edges")
    tiny = g["tiny_chunk"]
    assert g["tiny_first_index"].size == 3 and g["tiny_index_r0_f0"].size == 0
    tile = _producer(tiny).crop(g["anchor"], with_index=True)
    assert not bool(tile["is_valid"][0]) and "inputs" not in tile
    count, z = _raw_crop(tiny, tuple(g["anchor"]))
    assert count == 0 and z == tiny[g["tiny_first_index"], 2].min() == float(g["tiny_zshift"][0]) == -7.5


@pytest.mark.gpu
def test_device_crop_producer_reuse():
    """One TileProducer: a large result, a tiny one, an empty one, the first again -- stale `_out` / `_src` / `_count` and the
    0xff key memset between calls."""
    chunk = _seeded_chunk(20000, 51)
    prod = _producer(chunk)
    sizes = [_crop_vs_oracle(prod, chunk, a, rot, flip, min_equal)[1].size
             for a, rot, flip, min_equal in ((ANCHOR, 0, -1, 0.99), ((2950.0, 6950.0), 2, 0, 0), ((9000.0, 9000.0), 0, -1, 0),
                                             (ANCHOR, 0, -1, 0.99))]
    assert sizes[0] == sizes[3] > 1000 and 0 < sizes[1] < 100 and sizes[2] == 0


# ---- t2h_raster_patch against producer_ref.raster_patch, bit exact ------------------------------------------------------------
def _unique_raster(c, dtype):
    """pixel (c, r, col) holds c * 10^4 + r * 10^2 + col: exact in float32, so a wrong index map cannot hit an equal value"""
    return (np.arange(c)[:, None, None] * 1e4 + np.arange(37)[None, :, None] * 1e2 + np.arange(53)[None, None, :]).astype(dtype)


def _device_raster_patch(raster, row0, col0, ph, pw, rot, flip):
    from tomosar2height_amd import _lib
    c, h, w = raster.shape
    out = torch.full((c, ph, pw), -1.0, dtype=torch.float32, device=raster.device)
    _lib.call("t2h_raster_patch", _lib.ptr(raster), 1 if raster.dtype == torch.float64 else 0, c, h, w, row0, col0, ph, pw, rot, flip,
              _lib.ptr(out), _lib.stream())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c,dtype", [(1, np.float32), (3, np.float64)])
@pytest.mark.parametrize("ph,pw", [(16, 16), (5, 9), (1, 1), (37, 53)])
def test_device_raster_patch_shapes_and_borders(c, dtype, ph, pw):
    """Square and non-square patches (a non-square one is legal for 0 and 2 quarter turns) flush with each raster border, at every
    corner and inside; C * ph * pw off the 256 multiple; float32 and float64 sources."""
    host = _unique_raster(c, dtype)
    raster = torch.from_numpy(host).to("cuda:0")
    h, w = 37, 53
    places = sorted({(0, 0), (0, w - pw), (h - ph, 0), (h - ph, w - pw), (min(7, h - ph), min(11, w - pw))})
    for rot, flip in AUG:
        if ph != pw and rot % 2:
            continue
        got = [_device_raster_patch(raster, r0, c0, ph, pw, rot, flip) for r0, c0 in places]
        for (r0, c0), out in zip(places, got):
            want = producer_ref.raster_patch(host, r0 + ph - 1, c0, (ph, pw), rot, flip)
            assert want.dtype == np.float32 and np.array_equal(out.cpu().numpy(), want), (r0, c0, rot, flip)


@pytest.mark.gpu
def test_device_raster_patch_refusals():
    raster = torch.from_numpy(_unique_raster(1, np.float32)).to("cuda:0")
    for rot in (1, 3):
        with pytest.raises(RuntimeError, match="quarter-turn needs a square patch"):
            _device_raster_patch(raster, 3, 4, 5, 9, rot, -1)
    for r0, c0 in ((-1, 4), (37 - 5 + 1, 4), (3, -1), (3, 53 - 9 + 1)):
        with pytest.raises(RuntimeError, match="leave the 37 x 53 raster"):
            _device_raster_patch(raster, r0, c0, 5, 9, 0, -1)
    assert np.array_equal(_device_raster_patch(raster, 37 - 5, 53 - 9, 5, 9, 0, -1).cpu().numpy(),
                          producer_ref.raster_patch(_unique_raster(1, np.float32), 36, 44, (5, 9)))
