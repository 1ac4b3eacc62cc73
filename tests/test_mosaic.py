"""DSM mosaic (reference generator.py:85-157): blend weights pinned by the fixture produced from the
reference's own static method; device accumulate / finalize against the numpy oracle."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import mosaic_ref


def test_blend_weight_oracle_and_product_match_reference_fixture():
    from tomosar2height_amd.generator import DSMGenerator
    g = load_golden("mosaic_blend_weight")
    for k in g.files:
        if k.startswith("w512"):
            continue
        _, shape, a, b = k.split("_")
        r, c = (int(v) for v in shape.split("x"))
        pct = (float(a), float(b))
        np.testing.assert_allclose(mosaic_ref.linear_blend_patch_weight((r, c), pct), g[k], rtol=0, atol=1e-15)
        np.testing.assert_array_equal(DSMGenerator._linear_blend_patch_weight((r, c), list(pct)).numpy(), g[k])
    w = DSMGenerator._linear_blend_patch_weight((512, 512), [0.5, 0.5]).numpy()          # the shipped configuration
    np.testing.assert_array_equal(w[0, :], g["w512_row0"])
    np.testing.assert_array_equal(w[:, 0], g["w512_col0"])
    np.testing.assert_array_equal(w[255:257, 255:257], g["w512_centre"])
    assert w.min() == pytest.approx(1e-6) and w.max() == 1.0


def test_cal_shape_and_col_row():
    from tomosar2height_amd.generator import DSMGenerator
    assert DSMGenerator.cal_dsm_shape((10.0, 20.0), (1034.5, 788.0), (1.0, 1.0)) == (768, 1024)
    gen = DSMGenerator.__new__(DSMGenerator)
    gen.l_bound, gen.t_bound, gen.pixel_size = 10.0, 788.0, [1.0, 1.0]
    assert gen.query_col_row(10.5, 787.5) == (0, 0) == mosaic_ref.col_row(10.5, 787.5, 10.0, 788.0, (1.0, 1.0))
    assert gen.query_col_row(522.49, 276.5) == (512, 511)


@pytest.mark.gpu
def test_mosaic_accumulate_finalize_vs_oracle():
    from tomosar2height_amd.generator import DSMGenerator
    dev = torch.device("cuda:0")
    gen = DSMGenerator(model=None, device=dev, tiles=[], bounds=(0.0, 0.0, 160.0, 130.0), patch_size=(64.0, 64.0))
    assert gen.dsm_shape == (130, 160)
    g = torch.Generator().manual_seed(0)
    tiles = [(torch.randn(1, 64, 64, 1, generator=g) * 20, t, l) for t, l in ((0, 0), (0, 32), (32, 0), (32, 32), (60, 96), (66, 40))]
    dsm = torch.zeros(gen.dsm_shape, dtype=torch.float64, device=dev)
    weight = torch.zeros_like(dsm)
    for h, t, l in tiles:
        gen.accumulate(dsm, weight, h.to(dev), t, l)
    from tomosar2height_amd import _lib
    _lib.call("t2h_mosaic_finalize", _lib.ptr(dsm), _lib.ptr(weight), dsm.numel(), _lib.stream())
    want = mosaic_ref.mosaic([(h[0, :, :, 0].numpy(), t, l) for h, t, l in tiles], gen.dsm_shape,
                             mosaic_ref.linear_blend_patch_weight((64, 64), (0.5, 0.5)))
    got = dsm.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()       # uncovered pixels stay NaN
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=1e-12, atol=1e-12)
    assert (np.nan_to_num(got) >= 0).all()


@pytest.mark.gpu
def test_generate_dsm_end_to_end():
    """2 x 2 sliding tiles (stride 256 m, as conf/dataset/base.yaml:29) through the HIP model and the mosaic kernels
    against the oracle model + numpy mosaic."""
    from detinit import det_init_
    from oracle import torch_ref
    from tomosar2height_amd import TomoSAR2Height
    from tomosar2height_amd.config import berlin_config
    from tomosar2height_amd.generator import DSMGenerator
    from tomosar2height_amd.synthetic import berlin_tile
    dev = torch.device("cuda:0")
    cfg = berlin_config()
    ref = det_init_(torch_ref.TomoSAR2Height(cfg), seed=17)
    model = TomoSAR2Height(cfg)
    model.load_state_dict(ref.state_dict())
    model.to(dev)
    tiles = []
    for i, (x0, y0) in enumerate(((0.0, 0.0), (256.0, 0.0), (0.0, 256.0), (256.0, 256.0))):
        t = berlin_tile(40 + i, n_points=3000)
        t["min_bound"] = torch.tensor([[x0, y0, 0.0]])
        t["max_bound"] = torch.tensor([[x0 + 512.0, y0 + 512.0, 100.0]])
        tiles.append(t)
    tiles.append({"is_valid": torch.tensor([False])})                       # skipped like generator.py:133-134
    gen = DSMGenerator(model, dev, tiles, bounds=(0.0, 0.0, 768.0, 768.0))
    got = gen.generate_dsm().cpu().numpy()
    ref.eval()
    ref_tiles = []
    with torch.no_grad():
        for t in tiles[:4]:
            h = ref(input_cloud=t["inputs"])[0][0, :, :, 0].numpy()
            l, _ = mosaic_ref.col_row(t["min_bound"][0, 0].item() + 0.5, t["min_bound"][0, 1].item() + 0.5, 0.0, 768.0, (1, 1))
            _, top = mosaic_ref.col_row(t["max_bound"][0, 0].item() - 0.5, t["max_bound"][0, 1].item() - 0.5, 0.0, 768.0, (1, 1))
            ref_tiles.append((h, top, l))
    want = mosaic_ref.mosaic(ref_tiles, (768, 768), mosaic_ref.linear_blend_patch_weight((512, 512), (0.5, 0.5)))
    assert got.shape == (768, 768) and not np.isnan(got).any()
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-4 * scale


# ---- the two C entry points at edge shapes: float64 against the float64 numpy oracle, rtol = atol = 1e-12 as above (the kernel's
# `+= h * w` may contract to one fused multiply-add where numpy rounds twice, so bit equality is not owed) ----------------------
PATCH, MOSAIC = (40, 300), (130, 700)       # H != W; W spans two 256-thread blocks with a 44-column tail


def _patch_weight():
    """`mosaic_ref.linear_blend_patch_weight` on the 40 x 300 patch.  The reference (generator.py:94-110, restated verbatim by the
    oracle and the product) sizes the ROW ramp from the column count: blend percents (0.5, 0.5) ask for a 150-row ramp on 40 rows
    and raise in all three.  (0.5, 0.0625) is the widest pair of binary fractions the rule accepts here -- 20-column and 18-row
    ramps -- and keeps the 1e-3 * 1e-3 = 1e-6 corner weight; the accumulate kernel does not look at the weights' structure."""
    w = mosaic_ref.linear_blend_patch_weight(PATCH, (0.5, 0.0625))
    assert w.shape == PATCH and w[0, 0] == w[-1, -1] == 1e-6 and w.max() == 1.0
    return w


def _heights(k, seed=0):
    """per-pixel unique ramp plus noise, float32"""
    rng = np.random.RandomState(seed + k)
    return (np.arange(PATCH[0] * PATCH[1]).reshape(PATCH) * 0.01 + 7.0 * k + rng.standard_normal(PATCH)).astype(np.float32)


def _device_mosaic(tiles, shape, patch_weight, flip_rows=1, finalize=True):
    """tiles through t2h_mosaic_accumulate (and t2h_mosaic_finalize) called directly, so that t_row / l_col are free"""
    from tomosar2height_amd import _lib
    dev = torch.device("cuda:0")
    dsm = torch.zeros(shape, dtype=torch.float64, device=dev)
    weight = torch.zeros_like(dsm)
    pw = torch.from_numpy(patch_weight).to(dev)
    for height, t, l in tiles:
        h = torch.from_numpy(np.ascontiguousarray(height, np.float32)).to(dev)
        assert h.shape == pw.shape
        _lib.call("t2h_mosaic_accumulate", _lib.ptr(h), h.shape[0], h.shape[1], _lib.ptr(pw), _lib.ptr(dsm), _lib.ptr(weight),
                  shape[0], shape[1], t, l, flip_rows, _lib.stream())
    if finalize:
        _lib.call("t2h_mosaic_finalize", _lib.ptr(dsm), _lib.ptr(weight), dsm.numel(), _lib.stream())
    return dsm.cpu().numpy(), weight.cpu().numpy()


def _same_mosaic(got, want):
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(np.nan_to_num(got), np.nan_to_num(want), rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_mosaic_wide_patch_second_block_tail_and_overlaps():
    """40 x 300 patches on a 130 x 700 mosaic: the second x block and its `x >= W` tail, H != W, a tile flush with the bottom and
    right borders, overlaps of two and three tiles, one starting at column 256."""
    w = _patch_weight()
    tiles = [(_heights(k), t, l) for k, (t, l) in enumerate(((0, 0), (20, 150), (90, 400), (45, 256)))]
    got, _ = _device_mosaic(tiles, MOSAIC, w)
    want = mosaic_ref.mosaic(tiles, MOSAIC, w)
    assert np.isnan(want).any() and not np.isnan(want[90:, 400:]).any() and not np.isnan(want[:40, :300]).any()
    _same_mosaic(got, want)
    assert (np.nan_to_num(got) >= 0).all()


@pytest.mark.gpu
def test_mosaic_flip_rows_off():
    """flip_rows = 0 takes the height rows as they are: the oracle (which always flips) fed the pre-flipped heights."""
    w = _patch_weight()
    tiles = [(_heights(k, seed=10), t, l) for k, (t, l) in enumerate(((3, 5), (30, 250)))]
    got, _ = _device_mosaic(tiles, MOSAIC, w, flip_rows=0)
    _same_mosaic(got, mosaic_ref.mosaic([(h[::-1], t, l) for h, t, l in tiles], MOSAIC, w))
    assert not np.array_equal(np.nan_to_num(got), np.nan_to_num(mosaic_ref.mosaic(tiles, MOSAIC, w)))


@pytest.mark.gpu
def test_mosaic_clips_tiles_that_leave_the_mosaic():
    """include/t2h.h: "region rows/cols that fall outside the mosaic are skipped" -- through the C ABI (DSMGenerator.accumulate
    refuses such tiles, like the reference's slice `+=`), against numpy with the slice clipped."""
    from tomosar2height_amd.generator import DSMGenerator
    w = _patch_weight()
    tiles = [(_heights(k, seed=20), t, l) for k, (t, l) in enumerate(((-10, -20), (110, 650), (-39, 699)))]

    def clipped(tiles, shape):
        dsm, weight = np.zeros(shape), np.zeros(shape)
        for height, t, l in tiles:
            hw = np.asarray(height, np.float32)[::-1].astype(np.float64) * w
            r0, r1, c0, c1 = max(t, 0), min(t + PATCH[0], shape[0]), max(l, 0), min(l + PATCH[1], shape[1])
            dsm[r0:r1, c0:c1] += hw[r0 - t:r1 - t, c0 - l:c1 - l]
            weight[r0:r1, c0:c1] += w[r0 - t:r1 - t, c0 - l:c1 - l]
        return dsm, weight

    want_dsm, want_weight = clipped(tiles, MOSAIC)
    touched = want_weight > 0
    assert touched.sum() == 30 * 280 + 20 * 50 + 1 and touched[0, 699] and touched[129, 699] and touched[0, 0]
    got_dsm, got_weight = _device_mosaic(tiles, MOSAIC, w, finalize=False)
    assert not got_dsm[~touched].view(np.int64).any() and not got_weight[~touched].view(np.int64).any()   # bit-for-bit zero
    np.testing.assert_allclose(got_dsm, want_dsm, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got_weight, want_weight, rtol=1e-12, atol=1e-12)
    got, _ = _device_mosaic(tiles, MOSAIC, w)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = want_dsm / want_weight
    _same_mosaic(got, np.where(np.isnan(mean), np.nan, np.maximum(mean, 0.0)))
    dev = torch.device("cuda:0")
    gen = DSMGenerator(model=None, device=dev, tiles=[], bounds=(0.0, 0.0, 700.0, 130.0), patch_size=(40.0, 40.0))
    gen.patch_weight = torch.from_numpy(w).to(dev)
    assert gen.dsm_shape == MOSAIC
    dsm = torch.zeros(MOSAIC, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="is not inside the"):
        gen.accumulate(dsm, torch.zeros_like(dsm), torch.from_numpy(tiles[1][0]).to(dev), 110, 650)
    assert not dsm.any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_mosaic_finalize_pixel_outcomes(n):
    """Flat vectors (a 1 x n patch on a 1 x n mosaic) through accumulate and finalize against the oracle, every pixel one of:
    never covered (weight 0) -> NaN; its only contribution a NaN height -> NaN (the kernel keeps NaN where fmax would drop it);
    a negative weighted mean -> 0.0; weight 1e-6 only (the blend corner) -> the height at full relative accuracy."""
    rng = np.random.RandomState(n)
    for shift in range(4 if n == 1 else 1):
        kind = (np.arange(n) + shift) % 4
        height = (rng.uniform(5.0, 90.0, n) * np.where(kind == 2, -1.0, 1.0)).astype(np.float32)
        height[kind == 1] = np.nan
        w = np.select([kind == 0, kind == 3], [0.0, 1e-6], rng.uniform(0.1, 1.0, n))[None]
        tiles = [(height[None], 0, 0)]
        want = mosaic_ref.mosaic(tiles, (1, n), w)
        assert np.isnan(want[0, kind <= 1]).all() and (want[0, kind == 2] == 0.0).all()
        np.testing.assert_allclose(want[0, kind == 3], height[kind == 3].astype(np.float64), rtol=1e-15)
        got, _ = _device_mosaic(tiles, (1, n), w)
        _same_mosaic(got, want)
        assert (got[0, kind == 2] == 0.0).all()
        np.testing.assert_allclose(got[0, kind == 3], want[0, kind == 3], rtol=1e-12, atol=0)
