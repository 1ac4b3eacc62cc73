"""-m gpu: the sum matrices of the finest deferred resolution by occupied row (T2H_COMPACT_SUMS, include/t2h.h: compact per-cell matrices).

  * the occupied-row list of a level (``deferred.cell_rows``) against a numpy restatement, exactly;
  * two deferred levels (r = 16, then r = 32 on a tile of R = 32; the r = 32 matrices are the compact ones) forward and backward with the
    switch on and off, every new matrix filled with NaN before use (``deferred._empty``): rasters, dQ, dbase and the bias gradients (the
    whole of dconst's chain) bit for bit, the weight-gradient product ``x^T dacc`` -- re-associated over rows -- of both forms against its
    float64 restatement: the compact form's largest error over sum |x . dacc| may exceed the dense form's by at most 2 x (one more
    re-association of an fp32 sum).

Shapes: R = 32 and about 2 000 points per tile in five clusters, so that 30-60 % of the 1024 finest cells are empty (asserted), B = 1 and a
ragged B = 3; the occupied rows (553 and 1680) are no multiple of the weight gradient's row chunks and cross them.  ``tiny``: 400 points in
a few cells, fewer than 128 occupied rows.  At these sizes (fewer than 4096 rows) the two row-wise products run on the fp32 kernels, which
compute every row independently and ignore the row count: everything but x^T dacc is bit-identical.

``r64`` / ``r64wide`` / ``r64tiny``: one tile of R = 64 (4096 finest cells, the smallest matrix that takes the split 1-tap kernel), source
widths that are multiples of 64.  The recorded kernel symbols are asserted: with 64 channels at the compact level ``x @ A`` (1024 -> 64) runs
``bx3_rows_kernel<..,false>`` and ``dacc @ A^T`` (64 -> 1024) its persistent form ``<..,true>``; with 128 channels (``r64wide``) both run the
plain form.  2444 occupied rows end 12 rows into a 128-row tile (140 into a 256-row one); ``r64tiny`` has 86, inside the first tile.
The split kernel scales a staged tile by its largest magnitude before splitting into fp16 pieces, and a compact tile holds other rows
than a dense one: what lies downstream of a split product is NOT bit-identical between the two forms.  So for these cases
  * every split product of either form is checked by itself, over its rows in use, against float64 with the bound of
    tests/test_launch_census.py: |got - ref| <= c sum |a b|, c = max(2^-21, 4 e32) -- 2^-21 the contract of the fp16 two-way split, e32
    the error of torch's CPU fp32 product of the same operands;
  * the compact run is repeated with 3e30 instead of NaN behind the rows in use and must give the same bits: a staged tail value of
    either kind would change the block scale or the sums (this pins the early return and the zero staging of the last tile);
  * what no split product of the compact level feeds (the r = 32 raster, the bias gradients) stays bit-identical to the dense form; the
    rest agrees to 4e-5 of the max-norm -- twice the 2e-5 that tests/test_hip_gemm.py allows one product against float64, each form being
    one split product away from exact.  Measured (printed): dQ 7.8e-8 and 1.6e-8, dbase 1.3e-10 in ``r64tiny``, 0 elsewhere (tiles of
    like-sized random numbers mostly share their power-of-two scale); weight gradients 1.7e-7 .. 3.8e-7.

The rows are ARGUMENTS of the launch that uses them (the last ones, behind ``stream``), so a launch acts on nothing but its own:
  * ``t2h_gemm_bx3`` / ``t2h_linear_wgrad`` with a row count, then the same call without: the second is the dense product, bit for bit;
  * ``t2h_segsum_bwd_multi`` with the rows of a level that no plane has: refused before any launch;
  * ``t2h_sample_relu_cellsums2`` (no such argument) right after a compact ``t2h_sample_relu_cellsums_ordered``: the dense layout.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _clustered(n, seed, sigma=0.13, k=5):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(k, 2, generator=g) * 0.8 + 0.1
    which = torch.randint(0, k, (n,), generator=g)
    xy = (c[which] + sigma * torch.randn(n, 2, generator=g)).clamp(0.001, 0.999)
    return torch.cat([xy, torch.rand(n, 1, generator=g)], 1).reshape(1, n, 3)


def _rows_ref(clouds, r):
    """numpy restatement: occupied cells in plane order within a tile, tile after tile."""
    p = r * r
    occ = np.zeros(len(clouds) * p, bool)
    for b, c in enumerate(clouds):
        xy = c.reshape(-1, c.shape[-1])[:, :2].numpy()
        ix, iy = (xy[:, 0] * np.float32(r)).astype(np.int64), (xy[:, 1] * np.float32(r)).astype(np.int64)
        occ[b * p + iy * r + ix] = True
    cell_of_row = np.flatnonzero(occ).astype(np.int32)
    row_of_cell = np.full(occ.size, -1, np.int32)
    row_of_cell[cell_of_row] = np.arange(cell_of_row.size, dtype=np.int32)
    return row_of_cell, cell_of_row


def _case_clouds(case, r, sizes=(300, 517)):
    g = torch.Generator().manual_seed(11)
    out = []
    for b, n in enumerate(sizes):
        pts = torch.rand(1, n, 3, generator=g)
        if case == "quadrant":                              # nothing in x, y >= 1 / 2
            pts[..., :2] *= torch.tensor([0.5, 1.0]) if b == 0 else torch.tensor([1.0, 0.5])
            pts[0, : n // 2, :2] *= 0.5
        elif case == "full":                                # one point at the centre of every cell, the rest anywhere
            assert n >= r * r
            i = torch.arange(r * r)
            pts[0, : r * r, 0], pts[0, : r * r, 1] = ((i % r) + 0.5) / r, ((i // r) + 0.5) / r
        elif case == "one":                                 # all points of a tile in one cell
            cx, cy = (3, 5) if b == 0 else (r - 1, 0)
            pts[..., 0], pts[..., 1] = (cx + 0.1 + 0.8 * pts[..., 0]) / r, (cy + 0.1 + 0.8 * pts[..., 1]) / r
        out.append(pts.clamp_(0.0, 0.9999))
    return out


@pytest.mark.parametrize("case,R,level", [("quadrant", 16, 0), ("quadrant", 32, 0), ("full", 16, 0), ("full", 32, 1), ("one", 16, 0),
                                          ("one", 32, 0)])
def test_row_list(case, R, level):
    from tomosar2height_amd import deferred
    from tomosar2height_amd.tile import TileIndex
    r = R >> level
    clouds = _case_clouds(case, r)
    tile = TileIndex([c.to(_dev()) for c in clouds], R)
    buf = deferred.cell_rows(tile, level)
    assert deferred.cell_rows(tile, level) is buf                                   # cached on the index
    torch.cuda.synchronize()
    p = tile.B * r * r
    got = buf.cpu().numpy()
    row_of_cell, cell_of_row = _rows_ref(clouds, r)
    n_rows = int(got[2 * p])
    assert n_rows == cell_of_row.size
    assert np.array_equal(got[:p], row_of_cell)
    assert np.array_equal(got[p:p + n_rows], cell_of_row)
    if case == "full":
        assert n_rows == p and np.array_equal(got[:p], np.arange(p))
    if case == "one":
        assert n_rows == tile.B


def _run(clouds, compact, fill, monkeypatch, R=32, cb=32, chans=(128, 128)):
    """Two deferred levels (r = R / 2, then r = R) forward + backward; what comes out, every weight-gradient product with its operands,
    every split (t2h_gemm_bx3) product with its operands, and the (tag, kernel symbol) pairs of the row-wise products."""
    from tomosar2height_amd import _lib, deferred, mlp
    from tomosar2height_amd.tile import TileIndex
    monkeypatch.setattr(deferred, "COMPACT_SUMS", compact)
    monkeypatch.setattr(deferred, "_empty", (lambda *s, **k: torch.empty(*s, **k).fill_(fill)) if fill is not None else torch.empty)
    dev = _dev()
    tile = TileIndex([c.to(dev) for c in clouds], R)
    g = torch.Generator().manual_seed(5)
    base = torch.randn(tile.n_points, cb, generator=g).to(dev).requires_grad_()
    fcs, qs = [], []
    for r, c, cprev in ((R // 2, chans[0], cb), (R, chans[1], chans[0])):
        fc_b, fc_c = torch.nn.Linear(2 * c, c), torch.nn.Linear(cprev, c)
        for m in (fc_b, fc_c):
            with torch.no_grad():
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / m.weight.shape[1] ** 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            m.to(dev)
        fcs.append((fc_b, fc_c))
        qs.append(torch.randn(tile.B * r * r, 2 * c, generator=g).to(dev).requires_grad_())
    products, splits, orig, orig_bx3 = [], [], mlp.linear_wgrad_, mlp._gemm_bx3

    def recording(dy, x, dw, db, *a, **kw):
        orig(dy, x, dw, db, *a, **kw)
        if a or kw.get("relu_in"):
            return
        alone = torch.empty_like(dw)
        orig(dy, x, alone, None, row_limit=kw.get("row_limit"))
        products.append((dy.detach().clone(), x.detach().clone(), alone, kw.get("row_limit") is not None))

    def recording_bx3(x, w, w_is_kn, bias, mask, y, relu_out, accumulate, tag, row_limit=None):
        orig_bx3(x, w, w_is_kn, bias, mask, y, relu_out, accumulate, tag, row_limit)
        if x.shape[0] == tile.B * R * R and not accumulate and bias is None and mask is None:       # the compact level's products
            splits.append((tag, x.detach().clone(), w.detach().clone(), w_is_kn, y.detach().clone(), row_limit is not None))
    monkeypatch.setattr(mlp, "linear_wgrad_", recording)
    monkeypatch.setattr(mlp, "_gemm_bx3", recording_bx3)
    state = deferred.Deferred(tile, [1, 0], list(chans), base)
    assert (state.compact_lv == 0) == compact
    with _lib.KernelTimeline() as tl:
        rasters = [state.advance(q, r, fc_b, fc_c) for q, r, (fc_b, fc_c) in zip(qs, (R // 2, R), fcs)]
        loss = sum((ra * torch.randn(ra.shape, generator=g).to(dev)).sum() for ra in rasters)
        loss.backward()
        torch.cuda.synchronize()
    monkeypatch.setattr(mlp, "linear_wgrad_", orig)
    monkeypatch.setattr(mlp, "_gemm_bx3", orig_bx3)
    symbols = {(rec[0], rec[5]) for rec in tl.records if rec[0].startswith(("t2h_linear_dgrad", "t2h_linear_fwd"))}
    n_rows = int(state.rows[2 * tile.B * R * R].item()) if compact else None
    exact = {"raster0": rasters[0].detach(), "raster1": rasters[1].detach(), "dq0": qs[0].grad, "dq1": qs[1].grad, "dbase": base.grad}
    for i, (fc_b, fc_c) in enumerate(fcs):
        exact[f"db1_{i}"], exact[f"dbc_{i}"] = fc_b.bias.grad, fc_c.bias.grad
    weights = {f"dw{i}{j}": m.weight.grad for i, pair in enumerate(fcs) for j, m in enumerate(pair)}
    return exact, weights, products, n_rows, splits, symbols


def _product_error(products, n_rows):
    """Largest |got - x^T dacc (float64)| / sum |x . dacc| over the weight-gradient products; the compact one over its rows in use."""
    worst = 0.0
    for dy, x, got, limited in products:
        if limited:
            dy, x = dy[:n_rows], x[:n_rows]
        ref = dy.double().t() @ x.double()
        scale = dy.double().abs().t() @ x.double().abs()
        worst = max(worst, float(((got.double() - ref).abs() / scale.clamp_min(1e-300)).max()))
    return worst


def _check_splits(splits, n_rows, what):
    """Every split product over its rows in use against float64: |got - ref| <= max(2^-21, 4 e32) sum |a b| (tests/test_launch_census.py)."""
    for tag, x, w, w_is_kn, y, limited in splits:
        if limited:
            x, y = x[:n_rows], y[:n_rows]
        wk = w if w_is_kn else w.t()
        ref = x.double() @ wk.double()
        scale = (x.double().abs() @ wk.double().abs()).clamp_min(1e-300)
        e32 = float((((x.cpu() @ wk.cpu()).double() - ref.cpu()).abs() / scale.cpu()).max())
        c = max(2.0 ** -21, 4.0 * e32)
        err = float(((y.double() - ref).abs() / scale).max())
        print(f"[compact] {what} {tag}: max error / sum |a b| = {err:.3e} (bound {c:.3e}, e32 {e32:.3e})")
        assert torch.isfinite(y).all() and err <= c, (what, tag, err, c)


CLOUDS = {"b1": [(2100, 0)], "b3": [(2100, 1), (1500, 2), (2600, 3)], "tiny": [(400, 4)]}


@pytest.mark.parametrize("case", ["b1", "b3", "tiny"])
def test_levels_compact_against_dense(case, monkeypatch):
    clouds = [_clustered(n, seed, sigma=0.012 if case == "tiny" else 0.13) for n, seed in CLOUDS[case]]
    occupied = sum(len(np.unique(_rows_ref([c], 32)[1])) for c in clouds)
    frac_empty = 1.0 - occupied / (1024.0 * len(clouds))
    print(f"[compact] {case}: {occupied} occupied rows of {1024 * len(clouds)}, {frac_empty:.3f} empty")
    if case == "tiny":
        assert occupied < 128
    else:
        assert 0.3 <= frac_empty <= 0.6 and occupied % 128 != 0 and occupied > 128
    dense, dense_w, dense_products, _, _, _ = _run(clouds, False, float("nan"), monkeypatch)
    comp, comp_w, comp_products, n_rows, _, _ = _run(clouds, True, float("nan"), monkeypatch)
    plain, plain_w, _, _, _, _ = _run(clouds, True, None, monkeypatch)
    assert n_rows == occupied
    assert any(limited for *_, limited in comp_products) and not any(limited for *_, limited in dense_products)
    for name in dense:
        assert torch.isfinite(comp[name]).all(), name
        assert torch.equal(comp[name], plain[name]), f"{name}: what lies behind the rows in use changed the result"
        diff = float((comp[name] - dense[name]).abs().max())
        print(f"[compact] {case} {name}: max |compact - dense| = {diff:.3e} (max |dense| {float(dense[name].abs().max()):.3e})")
    for name in dense_w:
        assert torch.isfinite(comp_w[name]).all(), name
        assert torch.equal(comp_w[name], plain_w[name]), name
    e_dense, e_comp = _product_error(dense_products, None), _product_error(comp_products, n_rows)
    print(f"[compact] {case} x^T dacc: max error / sum |x . dacc|: dense {e_dense:.3e}, compact {e_comp:.3e}")
    for name in dense:
        assert torch.equal(comp[name], dense[name]), name
    assert e_comp <= 2.0 * e_dense


# (points, seed, cluster spread), base width, channels of the two levels, symbols of (x @ A, dacc @ A^T) at the compact level
SPLIT_CASES = {"r64": ((8300, 8, 0.13), 640, (128, 64), (",false>", ",true>")),
               "r64wide": ((8300, 8, 0.13), 128, (128, 128), (",false>", ",false>")),
               "r64tiny": ((8300, 6, 0.009), 640, (128, 64), (",false>", ",true>"))}


@pytest.mark.parametrize("case", list(SPLIT_CASES))
def test_split_products_stop_at_the_row_count(case, monkeypatch):
    (n, seed, sigma), cb, chans, (sym_dgrad, sym_fwd) = SPLIT_CASES[case]
    clouds = [_clustered(n, seed, sigma=sigma)]
    occupied = len(_rows_ref(clouds, 64)[1])
    print(f"[compact] {case}: {occupied} occupied rows of 4096, {1.0 - occupied / 4096.0:.3f} empty")
    if case == "r64tiny":
        assert occupied < 128
    else:
        assert 0.3 <= 1.0 - occupied / 4096.0 <= 0.6 and occupied % 128 not in (0, 127) and occupied % 256 != 0
    kw = dict(R=64, cb=cb, chans=chans)
    dense, dense_w, dense_products, _, dense_splits, dense_sym = _run(clouds, False, float("nan"), monkeypatch, **kw)
    comp, comp_w, comp_products, n_rows, comp_splits, comp_sym = _run(clouds, True, float("nan"), monkeypatch, **kw)
    huge, huge_w, _, _, _, _ = _run(clouds, True, 3.0e30, monkeypatch, **kw)
    assert n_rows == occupied
    # the two row-wise products of the compact level ran on the split kernel, in the forms named, with and without the row count
    k_all = cb + 2 * chans[0] + 2 * chans[1]
    want = {f"t2h_linear_dgrad[N={k_all},K={chans[1]}]": sym_dgrad, f"t2h_linear_fwd[K={chans[1]},N={k_all}]": sym_fwd}
    for sym in (dense_sym, comp_sym):
        got = dict(sym)
        for tag, tail in want.items():
            assert got.get(tag, "").startswith("bx3_rows_kernel<") and got[tag].endswith(tail), (tag, got.get(tag))
    assert len(comp_splits) == 2 and all(limited for *_, limited in comp_splits) and len(dense_splits) == 2
    _check_splits(dense_splits, None, f"{case} dense")
    _check_splits(comp_splits, n_rows, f"{case} compact")
    for name in list(dense) + list(dense_w):
        a, b, d = (comp | comp_w)[name], (huge | huge_w)[name], (dense | dense_w)[name]
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name}: what lies behind the rows in use changed the result"
        rel = float((a - d).abs().max()) / float(d.abs().max())
        print(f"[compact] {case} {name}: max |compact - dense| / max |dense| = {rel:.3e}")
        if name in ("raster0", "db1_0", "dbc_0", "db1_1", "dbc_1"):
            assert torch.equal(a, d), name
        else:
            assert rel <= 4e-5, (name, rel)
    e_dense, e_comp = _product_error(dense_products, None), _product_error(comp_products, n_rows)
    print(f"[compact] {case} x^T dacc: max error / sum |x . dacc|: dense {e_dense:.3e}, compact {e_comp:.3e}")
    assert e_comp <= 2.0 * e_dense


# ---- the rows are arguments: a compact launch leaves nothing behind for the launch after it ----------------------------------------
def _nan(*shape):
    return torch.full(shape, float("nan"), device=_dev())


def test_split_product_with_a_row_count_does_not_colour_the_next():
    """t2h_gemm_bx3 at M = 256, K = 64, N = 32 (the smallest supported shape with a second 128-row tile): with n_rows -> 100 the
    second tile is never written; the dense call right after it writes every row and equals the dense call made before, bit for bit."""
    from tomosar2height_amd import mlp
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(256, 64, generator=g).to(_dev()), (torch.randn(32, 64, generator=g) / 8).to(_dev())
    lim = torch.tensor([100], dtype=torch.int32, device=_dev())

    def product(row_limit):
        return mlp._gemm_bx3(x, w, False, None, None, _nan(256, 32), False, False, "t2h_linear_fwd[test]", row_limit)
    before, compact, after = product(None), product(lim.data_ptr()), product(None)
    torch.cuda.synchronize()
    assert torch.isnan(compact[128:]).all() and torch.isfinite(compact[:100]).all()
    assert torch.isfinite(before).all() and torch.isfinite(after).all()
    assert torch.equal(after, before)


def test_weight_gradient_with_a_row_count_does_not_colour_the_next():
    """t2h_linear_wgrad over M = 256 rows (K = N = 32): with n_rows -> 100 it is the dense product of the first 100 rows, bit for
    bit; the dense call right after it equals the dense call made before."""
    from tomosar2height_amd import mlp
    g = torch.Generator().manual_seed(4)
    dy, x = torch.randn(256, 32, generator=g).to(_dev()), torch.randn(256, 32, generator=g).to(_dev())
    lim = torch.tensor([100], dtype=torch.int32, device=_dev())

    def product(dy, x, row_limit=None):
        dw = _nan(32, 32)
        mlp.linear_wgrad_(dy, x, dw, None, row_limit=row_limit)
        return dw
    before, compact, after = product(dy, x), product(dy, x, lim.data_ptr()), product(dy, x)
    first100 = product(dy[:100], x[:100])
    torch.cuda.synchronize()
    assert torch.isfinite(before).all() and torch.isfinite(compact).all()
    assert torch.equal(compact, first100) and not torch.equal(compact, before)
    assert torch.equal(after, before)


def test_rows_of_a_level_that_no_plane_has_are_refused():
    """t2h_segsum_bwd_multi: a row list whose rows_level is none of levels[] is T2H_ERR_ARG, before any launch."""
    from tomosar2height_amd import _lib, deferred
    from tomosar2height_amd.tile import TileIndex
    tile = TileIndex([_clustered(2100, 0).to(_dev())], 32)
    c = 32
    planes = [(torch.ones(tile.B * 1024, c, device=_dev()), 0), (torch.ones(tile.B * 256, c, device=_dev()), 1)]
    arr, lvs, lds = deferred._plane_args(planes)
    rows = deferred.cell_rows(tile, 0)
    out = _nan(tile.n_points, c)
    with pytest.raises(_lib.T2HLibraryError, match=r"t2h_segsum_bwd_multi failed \(code -1\).*level 2"):
        _lib.call("t2h_segsum_bwd_multi", arr, lvs, lds, len(planes), _lib.ptr(tile.cell), tile.B, tile.N, tile.nbits, c, None, None,
                  _lib.ptr(out), _lib.stream(), rows.data_ptr(), 2)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_dense_cell_sums_right_after_compact_ones():
    """t2h_sample_relu_cellsums2 takes no rows: right after a t2h_sample_relu_cellsums_ordered that wrote its sums by occupied row
    (R = 32, sampling level r = 16, sums at r = 32, C = 256) it writes one row per cell, the same bits as when called first."""
    from tomosar2height_amd import _lib, deferred
    from tomosar2height_amd.tile import TileIndex
    clouds = [_clustered(2100, 0)]
    tile = TileIndex([cl.to(_dev()) for cl in clouds], 32)
    c, lv = 256, 1
    q = torch.randn(tile.B, 16, 16, c, generator=torch.Generator().manual_seed(9)).to(_dev())
    head = (_lib.ptr(q), _lib.ptr(tile.pts), tile.dim, _lib.ptr(tile.off0), tile.B, tile.N, tile.nbits, lv, 0, c)

    def dense():
        sums, pooled = _nan(tile.B * 1024, c), _nan(tile.B * 256, c)
        _lib.call("t2h_sample_relu_cellsums2", *head, _lib.ptr(sums), c, _lib.ptr(pooled), c, None, _lib.stream())
        return sums, pooled
    first = dense()
    rows = deferred.cell_rows(tile, 0)
    by_row, pooled = _nan(tile.B * 1024, c), _nan(tile.B * 256, c)
    _lib.call("t2h_sample_relu_cellsums_ordered", *head, _lib.ptr(by_row), c, _lib.ptr(pooled), c, None, None, _lib.stream(),
              rows.data_ptr())
    again = dense()
    torch.cuda.synchronize()
    row_of_cell, cell_of_row = _rows_ref(clouds, 32)
    n_rows = len(cell_of_row)
    assert 0 < n_rows < 1024
    assert torch.isnan(by_row[n_rows:]).all()                                        # (the launch in between was a compact one)
    assert torch.equal(by_row[:n_rows], first[0][torch.from_numpy(cell_of_row).long().to(_dev())])
    assert torch.equal(pooled, first[1])
    for a, b in zip(again, first):
        assert torch.isfinite(a).all() and torch.equal(a, b)
