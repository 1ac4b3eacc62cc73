"""Device interpolation baselines (tomosar2height_amd.interpolate, csrc/dsm_interp.hip) against the fixture made from the
reference's scripts/interpolate_nearest.py / interpolate_idw.py and against the numpy restatement tests/interp_ref.py.

Squared distances, the gathered (X, Y, Z) of the neighbour indices and the nearest raster are compared byte for byte with the
restatement on every pixel; the IDW raster to 32 * 2^-53 * max|z| (interp_ref.idw_bound; byte equality is what the fixed
order is expected to give and is printed).  Against the reference's own rasters the comparison leaves out the pixels whose k-th
and (k + 1)-th neighbours tie, as tests/test_interp_cpu.py does.
"""
import numpy as np
import pytest
import torch

import eval_ref
import inst_ref
import interp_ref
from test_interp_cpu import CASES, fixture_case

pytestmark = pytest.mark.gpu

_cache = {}


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def case(name):
    """The fixture case with its restatement (computed once, shared, never modified) and its device index."""
    from tomosar2height_amd import CloudIndex
    hit = _cache.get(name)
    if hit is None:
        c = fixture_case(name)
        u = interp_ref.unique_cloud(c["points"])
        c["ref_unique"] = u
        c["knn"] = {k: interp_ref.knn(u, 1.0, k) for k in (1, 3, 8)}
        c["ref_nearest"] = interp_ref.nearest(u)[0]
        c["ref_idw"] = interp_ref.idw(u)[0]
        c["index"] = CloudIndex(to_dev(c["points"]))
        hit = _cache[name] = c
    return hit


def check_index(index, points):
    """Unique cloud as a set of rows, M, bounds, and the cell structure: offsets ascending, every point in its cell."""
    u = interp_ref.unique_cloud(points)
    got = index.unique.cpu().numpy()
    assert index.n_unique == len(u) == len(got) and index.n_points == len(points)
    assert interp_ref.rows_as_set(got) == interp_ref.rows_as_set(u)
    assert index.bounds == (u[:, 0].min(), u[:, 0].max(), u[:, 1].min(), u[:, 1].max()) and index.origin == index.bounds[::2]
    gy, gx = index.cells
    off = index.cell_offsets.cpu().numpy()
    assert gx * gy + 1 <= len(off) and off[0] == 0 and (np.diff(off) >= 0).all() and (off[gx * gy:] == len(u)).all()
    h = index.cell_edge
    cx = np.minimum(np.floor((got[:, 0] - index.origin[0]) / h), gx - 1)
    cy = np.minimum(np.floor((got[:, 1] - index.origin[1]) / h), gy - 1)
    cell = (cy * gx + cx).astype(np.int64)
    assert (np.diff(cell) >= 0).all() and np.array_equal(off[:gx * gy + 1], np.searchsorted(cell, np.arange(gx * gy + 1)))
    return u


def check_all(points, resolution=1.0, ks=(1, 8)):
    """Index, kNN and both rasters of a small cloud against the restatement; returns the index."""
    from tomosar2height_amd import CloudIndex, grid_knn, idw_dsm, nearest_dsm
    index = CloudIndex(to_dev(points))
    u = check_index(index, points)
    got_u = index.unique.cpu().numpy()
    for k in ks:
        if k > len(u):
            continue
        d2, idx = grid_knn(index, resolution, k)
        want_d2, want_idx, _ = interp_ref.knn(u, resolution, k)
        assert tuple(d2.shape) == want_d2.shape == index.grid_shape(resolution) + (k,)
        assert d2.cpu().numpy().tobytes() == want_d2.tobytes(), (k, resolution)
        assert got_u[idx.cpu().numpy().astype(np.int64)].tobytes() == u[want_idx].tobytes(), (k, resolution)
    near, origin = nearest_dsm(index, resolution)
    assert origin == index.origin and near.cpu().numpy().tobytes() == interp_ref.nearest(u, resolution)[0].tobytes()
    k = min(8, len(u))
    idw, _ = idw_dsm(index, resolution, k=k)
    want = interp_ref.idw(u, resolution, k)[0]
    assert np.abs(idw.cpu().numpy() - want).max(initial=0.0) <= interp_ref.idw_bound(u[:, 2])
    return index


@pytest.mark.parametrize("name", CASES)
def test_unique_cloud_and_bounds(name):
    c = case(name)
    u = check_index(c["index"], c["points"])
    assert u.tobytes() == np.ascontiguousarray(c["unique"]).tobytes()              # the fixture's group-by result
    assert c["index"].origin == tuple(c["origin"]) and c["index"].grid_shape() == c["nearest"].shape


@pytest.mark.parametrize("k", (1, 3, 8))
@pytest.mark.parametrize("name", CASES)
def test_knn_matches_restatement_and_kd_tree(name, k):
    from tomosar2height_amd import grid_knn
    c = case(name)
    d2, idx = grid_knn(c["index"], 1.0, k)
    assert d2.is_cuda and d2.dtype == torch.float64 and idx.dtype == torch.int32
    want_d2, want_idx, tie = c["knn"][k]
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
    assert d2.shape == want_d2.shape and d2.tobytes() == want_d2.tobytes()
    assert idx.min() >= 0 and idx.max() < c["index"].n_unique
    got = c["index"].unique.cpu().numpy()[idx]                                     # [ny, nx, k, 3]: what pins the tie rule
    assert got.tobytes() == c["ref_unique"][want_idx].tobytes()
    assert np.array_equal(np.sqrt(d2), c["dist"][..., :k])                         # the k-d tree's own distances
    if name == "coarse":
        assert tie.mean() > 0.05


@pytest.mark.parametrize("name", CASES)
def test_rasters(name):
    from tomosar2height_amd import idw_dsm, nearest_dsm
    c = case(name)
    near, origin = nearest_dsm(c["index"])
    idw, origin2 = idw_dsm(c["index"])
    assert origin == origin2 == tuple(c["origin"]) and near.dtype == idw.dtype == torch.float64
    near, idw = near.cpu().numpy(), idw.cpu().numpy()
    assert near.tobytes() == c["ref_nearest"].tobytes()
    bound = interp_ref.idw_bound(c["ref_unique"][:, 2])
    gap = np.abs(idw - c["ref_idw"]).max()
    print(name, "IDW vs restatement:", gap / (bound / 32), "x 2^-53 max|z|; byte-equal:", idw.tobytes() == c["ref_idw"].tobytes())
    assert gap <= bound
    tie1, tie8 = c["knn"][1][2], c["knn"][8][2]
    assert near[~tie1].tobytes() == c["nearest"][~tie1].tobytes()                  # the reference's rasters, untied pixels
    gap = np.abs(idw - c["idw"])[~tie8].max()
    print(name, "IDW vs reference:", gap / (bound / 32), "x 2^-53 max|z|")
    assert gap <= bound
    a, _ = idw_dsm(to_dev(c["points"]), k=3)                                       # from points, and another k
    assert np.abs(a.cpu().numpy() - interp_ref.idw(c["ref_unique"], 1.0, 3)[0]).max() <= bound


@pytest.mark.parametrize("name", ("main", "coarse"))
def test_two_runs_same_bytes(name):
    from tomosar2height_amd import CloudIndex, grid_knn, idw_dsm, nearest_dsm
    c = case(name)
    first = c["index"]
    pts = to_dev(c["points"])
    for again in (CloudIndex(pts), CloudIndex(pts.to(torch.float64).clone())):
        assert again.unique.cpu().numpy().tobytes() == first.unique.cpu().numpy().tobytes()
        assert again.cell_offsets.cpu().numpy().tobytes() == first.cell_offsets.cpu().numpy().tobytes()
        assert (again.bounds, again.cells, again.cell_edge, again.n_unique) == (first.bounds, first.cells, first.cell_edge, first.n_unique)
        for a, b in zip(grid_knn(again, 1.0, 8), grid_knn(first, 1.0, 8)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        assert nearest_dsm(again)[0].cpu().numpy().tobytes() == nearest_dsm(first)[0].cpu().numpy().tobytes()
        assert idw_dsm(again)[0].cpu().numpy().tobytes() == idw_dsm(first)[0].cpu().numpy().tobytes()


def small_cloud(n, seed, extent=(20.0, 13.0), quantum=0.05):
    rng = np.random.default_rng(seed)
    xy = np.round(rng.random((n, 2)) * extent / quantum) * quantum
    return np.c_[392000.0 + xy[:, 0], 5820000.0 + xy[:, 1], rng.standard_normal(n) * 4 + 20]


def test_point_count_not_a_multiple_of_the_workgroup_and_float32_input():
    from tomosar2height_amd import CloudIndex
    pts = small_cloud(1000 + 27, 1)                                                # 1 027 = 4 x 256 + 3
    pts = np.r_[pts, pts[:100] + [0.0, 0.0, 1.5]]                                  # duplicates with a larger z
    check_all(pts)
    p32 = (small_cloud(300, 2) - [392000.0, 5820000.0, 0.0]).astype(np.float32)    # float32 is widened exactly
    index = CloudIndex(to_dev(p32))
    check_index(index, p32.astype(np.float64))


def test_all_points_in_one_cell_and_m_equal_k():
    pts = small_cloud(8, 3, extent=(3.0, 2.0))                                     # M == k == 8
    index = check_all(pts)
    assert index.n_unique == 8
    same = np.c_[np.full(40, 5.0), np.full(40, 7.0), np.arange(40.0)]              # one (x, y): one cell, M = 1, empty raster
    index = check_all(same, ks=(1,))
    assert index.n_unique == 1 and index.cells == (1, 1) and index.unique.cpu().numpy().tolist() == [[5.0, 7.0, 39.0]]
    dense = np.c_[5.0 + np.arange(300) * 1e-4, 7.0 + (np.arange(300) % 7) * 1e-4, np.arange(300.0)]
    check_all(np.r_[dense, [[9.5, 11.5, 1.0]]])                                    # 300 points in the corner cell of a wide box


def test_empty_grid_and_raster_smaller_than_a_tile():
    from tomosar2height_amd import grid_knn, idw_dsm, nearest_dsm
    line = np.c_[np.linspace(10.0, 19.5, 20), np.full(20, 3.0), np.arange(20.0)]   # ymin == ymax
    index = check_all(line)
    assert index.grid_shape() == (0, 10)
    assert tuple(nearest_dsm(index)[0].shape) == (0, 10) and tuple(idw_dsm(index)[0].shape) == (0, 10)
    assert tuple(grid_knn(index, 1.0, 4)[0].shape) == (0, 10, 4)
    index = check_all(small_cloud(60, 4, extent=(5.3, 3.2)))                       # a few nodes: a corner of one tile
    ny, nx = index.grid_shape()
    assert 0 < ny <= 4 and 0 < nx <= 6


def test_point_on_xmax_and_other_resolutions():
    pts = small_cloud(400, 5, extent=(33.0, 18.0), quantum=0.5)
    pts = np.r_[pts, [[392000.0, 5820000.0, 40.0], [392033.0, 5820004.0, 50.0], [392010.0, 5820018.0, 60.0], [392033.0, 5820018.0, 70.0]]]
    index = check_all(pts)
    assert index.bounds[1] == 392033.0 and index.bounds[3] == 5820018.0 and index.grid_shape() == (18, 33)
    for resolution in (0.5, 2.0):
        check_all(pts, resolution, ks=(8,))
    assert index.grid_shape(0.5) == (36, 66) and index.grid_shape(2.0) == (9, 17)


def test_refusals():
    from tomosar2height_amd import CloudIndex, grid_knn, idw_dsm, nearest_dsm
    pts = small_cloud(50, 6)
    for bad in (np.nan, np.inf, -np.inf):
        for col in (0, 1, 2):
            p = pts.copy()
            p[17, col] = bad
            with pytest.raises(ValueError, match="1 of 50 points.*non-finite"):
                CloudIndex(to_dev(p))
    few = CloudIndex(to_dev(np.r_[pts[:5], pts[:5] + [0.0, 0.0, 1.0]]))            # M = 5 < k = 8
    assert few.n_unique == 5
    with pytest.raises(ValueError, match="5 distinct"):
        idw_dsm(few)
    with pytest.raises(ValueError, match="5 distinct"):
        grid_knn(few, 1.0, 6)
    nearest_dsm(few)
    idw_dsm(few, k=5)
    with pytest.raises(ValueError, match="power"):
        idw_dsm(few, k=5, power=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nearest_dsm(torch.from_numpy(pts))
    with pytest.raises(TypeError, match="float64"):
        CloudIndex(to_dev(pts).to(torch.int64))


def test_idw_raster_feeds_both_evaluators():
    """idw_dsm -> DSMEvaluator.eval / BuildingEvaluator.eval with no host copy in between: equal to the restatements fed the
    same raster."""
    from tomosar2height_amd import BuildingEvaluator, DSMEvaluator, idw_dsm
    c = case("main")
    dsm, (xmin, ymin) = idw_dsm(c["index"])
    host = dsm.cpu().numpy()
    H, W = host.shape
    rng = np.random.default_rng(11)
    gt = (host + rng.standard_normal((H, W)) * 1.5).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    for _ in range(12):
        y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
        mask[y:y + rng.integers(2, 9), x:x + rng.integers(2, 9)] = 1
    # row 0 of the baseline is ymin; the evaluators only need the two rasters on one grid
    ev = DSMEvaluator(to_dev(gt), bounds=(xmin, ymin), other_masks={"building": to_dev(mask.astype(bool))})
    stats, diff = ev.eval(dsm)
    want, want_diff = eval_ref.evaluate(host, gt, None, {"building": mask.astype(bool)})
    eval_ref.assert_stats(stats, want)
    eval_ref.assert_diff(diff.cpu().numpy(), want_diff)
    got, rec = BuildingEvaluator(to_dev(mask), to_dev(gt), bounds=(xmin, ymin)).eval(dsm)
    want, labels, counts, pm, gm = inst_ref.evaluate(host, gt, mask)
    assert rec["labels"].cpu().numpy().tobytes() == labels.tobytes() and rec["counts"].cpu().numpy().tobytes() == counts.tobytes()
    assert inst_ref.same_floats(rec["pred_median"].cpu().numpy(), pm) and inst_ref.same_floats(rec["gt_median"].cpu().numpy(), gm)
    inst_ref.assert_metrics(got, want)
    assert got["n_buildings"] >= 3 and got["n_valid"] == got["n_buildings"]
