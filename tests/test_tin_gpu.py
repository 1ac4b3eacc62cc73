"""Device Delaunay-linear baseline (tomosar2height_amd.interpolate.delaunay_dsm / grid_simplex, csrc/dsm_tin.hip) against the
fixture made with scipy's griddata / find_simplex on shifted coordinates and against the numpy restatement tests/tin_ref.py.

Per fixture case: the NaN mask equals the reference's; the triangle of every non-ambiguous node is find_simplex's (as a set of
points: the device's rows are in cell order); barycentric coordinates and raster are byte-equal to the restatement evaluated
on the device's own triangles; the raster lies within the fixture's ``units_bound`` of griddata's; no node reached the pivot
cap; two runs give the same bytes.  Only ambiguous nodes (at most 0.5 % of a case's finite nodes) are left out, and only of
the comparisons with the reference.
"""
import numpy as np
import pytest
import torch

import eval_ref
import inst_ref
import tin_ref
from test_tin_cpu import CASES, fixture_case

pytestmark = pytest.mark.gpu

_cache = {}


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def case(name):
    """The fixture case with the device's index, triangles, coordinates and raster (computed once, shared, never modified)."""
    from tomosar2height_amd import CloudIndex, delaunay_dsm, grid_simplex
    hit = _cache.get(name)
    if hit is None:
        c = fixture_case(name)
        c["index"] = CloudIndex(to_dev(c["points"]))
        tri, bary, c["simplex_status"] = grid_simplex(c["index"], c["resolution"], return_status=True)
        dsm, c["origin"], c["status"] = delaunay_dsm(c["index"], c["resolution"], return_status=True)
        assert tri.dtype == torch.int32 and bary.dtype == dsm.dtype == torch.float64 and dsm.is_cuda
        c["dev_unique"] = c["index"].unique.cpu().numpy()
        c["dev_tri"], c["dev_bary"], c["dev_dsm"] = tri.cpu().numpy(), bary.cpu().numpy(), dsm.cpu().numpy()
        hit = _cache[name] = c
    return hit


def check_against_restatement(u, tri, bary, dsm, resolution):
    """bary and raster byte-equal to the restatement on the device's own triangles; rows ascending; lambda inside [0, 1]."""
    ok = tri[..., 0] >= 0
    assert ((tri >= 0).all(-1) == ok).all() and tri.max(initial=-1) < len(u)
    assert (tri[ok][:, 0] < tri[ok][:, 1]).all() and (tri[ok][:, 1] < tri[ok][:, 2]).all()
    want = tin_ref.barycentric(u, tri, resolution)
    assert bary.tobytes() == want.tobytes()
    assert dsm.tobytes() == tin_ref.linear(u, tri, resolution).tobytes()
    assert np.array_equal(np.isnan(dsm), ~ok)
    if ok.any():
        assert bary[ok].min() >= -2.0 ** -30


@pytest.mark.parametrize("name", CASES)
def test_fixture_case(name):
    c = case(name)
    u, tri, dsm = c["dev_unique"], c["dev_tri"], c["dev_dsm"]
    assert c["origin"] == (c["unique"][:, 0].min(), c["unique"][:, 1].min()) and dsm.shape == c["dsm"].shape
    assert tin_ref.unique_cloud(u).tobytes() == c["unique"].tobytes()
    assert np.array_equal(np.isnan(dsm), np.isnan(c["dsm"]))                      # the NaN mask, every node
    assert np.array_equal(tri[..., 0] < 0, np.isnan(c["dsm"]))
    clear = ~c["ambiguous"]
    got, want = tin_ref.vertex_sets(u, tri), tin_ref.vertex_sets(c["unique"], c["tri"])
    assert got[clear].tobytes() == want[clear].tobytes()                           # find_simplex's triangles
    check_against_restatement(u, tri, c["dev_bary"], dsm, c["resolution"])
    finite = ~np.isnan(dsm)
    gap = tin_ref.units(dsm, c["dsm"], u, tri)[finite & clear].max()
    print(name, "device vs griddata:", gap, "units; bound", c["units_bound"], "status", c["status"])
    assert gap <= c["units_bound"]
    for st in (c["status"], c["simplex_status"]):
        assert st["capped"] == 0 and st["unresolved"] == 0
    assert c["status"] == c["simplex_status"]
    hull = c["index"].hull().cpu().numpy()
    assert c["index"].hull() is c["index"].hull() and hull.dtype == np.int32      # cached on the index
    P = u[hull, :2] - c["origin"]
    nxt = np.roll(P, -1, 0)
    assert (P[:, 0] * nxt[:, 1] - P[:, 1] * nxt[:, 0]).sum() > 0                   # counter-clockwise
    a, b, d = P, nxt, np.roll(P, -2, 0)
    assert ((b[:, 0] - a[:, 0]) * (d[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (d[:, 0] - a[:, 0]) > 0).all()
    allp = u[:, :2] - c["origin"]
    for k in range(len(P)):                                                       # every point on or left of every edge
        cr = (b[k, 0] - a[k, 0]) * (allp[:, 1] - a[k, 1]) - (b[k, 1] - a[k, 1]) * (allp[:, 0] - a[k, 0])
        assert cr.min() >= 0


@pytest.mark.parametrize("name", CASES)
def test_two_runs_same_bytes(name):
    from tomosar2height_amd import CloudIndex, delaunay_dsm, grid_simplex
    c = case(name)
    again = CloudIndex(to_dev(c["points"]).clone())
    assert again.hull().cpu().numpy().tobytes() == c["index"].hull().cpu().numpy().tobytes()
    tri, bary = grid_simplex(again, c["resolution"])
    dsm, _ = delaunay_dsm(again, c["resolution"])
    assert tri.cpu().numpy().tobytes() == c["dev_tri"].tobytes() and bary.cpu().numpy().tobytes() == c["dev_bary"].tobytes()
    assert dsm.cpu().numpy().tobytes() == c["dev_dsm"].tobytes()
    dsm2, _ = delaunay_dsm(to_dev(c["points"]), c["resolution"])                    # from points
    assert dsm2.cpu().numpy().tobytes() == c["dev_dsm"].tobytes()


def test_node_on_a_point_returns_its_height():
    c = case("on_node")
    u, dsm = c["unique"], c["dev_dsm"]
    o = c["origin"]
    for x, y in ((0.0, 0.0), (7.0, 5.0), (11.5, 3.0)):
        row = np.flatnonzero((u[:, 0] == o[0] + x) & (u[:, 1] == o[1] + y))
        assert len(row) == 1 and c["ambiguous"][int(y * 2), int(x * 2)]
        assert dsm[int(y * 2), int(x * 2)] == u[row[0], 2]
        lam = c["dev_bary"][int(y * 2), int(x * 2)]
        assert sorted(np.abs(lam).tolist()) == [0.0, 0.0, 1.0]


def run_small(points, resolution=1.0):
    """A structural case: triangles by brute force where the cloud is small, always the restatement on the device's triangles."""
    from tomosar2height_amd import CloudIndex, delaunay_dsm, grid_simplex
    index = CloudIndex(to_dev(points))
    tri, bary, st = grid_simplex(index, resolution, return_status=True)
    dsm, origin, st2 = delaunay_dsm(index, resolution, return_status=True)
    assert st["capped"] == st["unresolved"] == 0 and st == st2 and origin == index.origin
    u, tri, bary, dsm = index.unique.cpu().numpy(), tri.cpu().numpy(), bary.cpu().numpy(), dsm.cpu().numpy()
    assert tuple(dsm.shape) == index.grid_shape(resolution) and tri.shape == dsm.shape + (3,)
    check_against_restatement(u, tri, bary, dsm, resolution)
    ref_u = tin_ref.unique_cloud(np.asarray(points, np.float64))
    if len(ref_u) <= 64 and dsm.size:
        want, count = tin_ref.brute_force(ref_u, resolution)
        sure = count <= 1                                                         # off the edges: one triangle, or none
        assert np.array_equal(tri[..., 0] < 0, count == 0)
        assert tin_ref.vertex_sets(u, tri)[sure].tobytes() == tin_ref.vertex_sets(ref_u, want)[sure].tobytes()
    return index, tri, dsm


def exact_cloud(n, seed, extent=(20.0, 13.0)):
    """Coordinates offset + d, d a multiple of 2^-16: the shift and every orientation test are exact."""
    rng = np.random.default_rng(seed)
    xy = np.floor(rng.random((n, 2)) * extent * 65536) / 65536
    return np.c_[389000.0 + xy[:, 0], 5819000.0 + xy[:, 1], np.round(rng.random(n) * 60 + 30, 3)]


def test_one_triangle_and_four_points():
    three = np.array([[389000.0, 5819000.0, 10.0], [389006.5, 5819001.0, 20.0], [389002.0, 5819005.25, 40.0]])
    index, tri, dsm = run_small(three)
    assert index.n_unique == 3 and index.hull().shape[0] == 3 and dsm.shape == (6, 7)
    assert (tri[tri[..., 0] >= 0] == [0, 1, 2]).all() and dsm[0, 0] == 10.0 and np.isnan(dsm[5, 6])
    four = np.r_[three, [[389006.0, 5819006.0, 5.0]]]
    index, tri, dsm = run_small(four)
    assert index.n_unique == 4 and index.hull().shape[0] == 4 and len({tuple(t) for t in tri[tri[..., 0] >= 0]}) == 2
    run_small(np.r_[three, [[389003.0, 5819002.0, 7.0]]])                          # the fourth inside the triangle: three triangles


def test_all_points_in_one_cell_and_a_small_raster():
    dense = np.c_[389005.0 + (np.arange(40) % 8) / 1024, 5819007.0 + (np.arange(40) // 8) / 2048 + (np.arange(40) % 3) / 8192,
                  np.arange(40.0)]
    index, tri, dsm = run_small(np.r_[dense, [[389009.5, 5819010.5, 1.0], [389005.0, 5819011.0, 2.0]]])
    assert 0 < dsm.size < 256                                                     # one corner of one 16 x 16 tile
    index, tri, dsm = run_small(exact_cloud(60, 4, extent=(5.3, 3.2)))
    assert 0 < dsm.shape[0] <= 4 and 0 < dsm.shape[1] <= 6
    index, tri, dsm = run_small(exact_cloud(50, 5, extent=(0.9, 0.8)))             # every point inside the first raster cell
    assert dsm.shape == (1, 1)
    # N = 7 < 8: the cell edge 8 * max(w, h) / N exceeds the extent, so the index is ONE cell -- ring 0 covers the grid at once
    # and every verification scans that cell alone
    for seed in (8, 9):
        index, tri, dsm = run_small(exact_cloud(7, seed, extent=(9.0, 7.0)))
        assert index.cells == (1, 1) and index.n_unique == 7 and dsm.size >= 20 and (tri[..., 0] >= 0).sum() >= 5
    index, tri, dsm = run_small(exact_cloud(7, 10, extent=(9.0, 7.0)), 0.25)         # the same with several tiles over the one cell
    assert index.cells == (1, 1) and dsm.shape[1] > 16


def test_empty_raster_and_degenerate_clouds():
    from tomosar2height_amd import CloudIndex, delaunay_dsm, grid_simplex
    thin = np.array([[10.0, 3.0, 1.0], [14.5, 3.0, 2.0], [12.0, 3.0, 5.0]])
    for pts in (thin, thin[:2], thin[:1], np.c_[np.arange(9.0), 2.0 * np.arange(9.0) + 1.0, np.arange(9.0)],
                np.r_[thin[:2], thin[:2] + [0.0, 0.0, 4.0]]):
        index = CloudIndex(to_dev(pts))
        for fn in (delaunay_dsm, grid_simplex):
            with pytest.raises(ValueError, match="span no area"):
                fn(index)
    with pytest.raises(ValueError, match="span no area"):
        delaunay_dsm(to_dev(thin))
    flat = np.array([[10.0, 3.0, 1.0], [14.5, 3.25, 2.0], [12.0, 3.5, 5.0]])      # an area, but no raster row (ymax - ymin < res)
    index = CloudIndex(to_dev(flat))
    dsm, _ = delaunay_dsm(index, 1.0)
    assert tuple(dsm.shape) == (1, 5)
    dsm, _, st = delaunay_dsm(index, 8.0, return_status=True)
    assert tuple(dsm.shape) == (1, 1) and st["capped"] == 0
    level = np.array([[10.0, 3.0, 1.0], [10.0, 3.5, 2.0], [10.25, 3.25, 5.0]])
    index = CloudIndex(to_dev(level))
    assert index.grid_shape(0.5) == (1, 1) and index.grid_shape(1.0) == (1, 1)
    wide = CloudIndex(to_dev(np.array([[0.0, 0.0, 1.0], [4.0, 0.0, 2.0], [2.0, 0.0, 3.0], [1.0, 0.0, 3.0]])))
    assert wide.grid_shape() == (0, 4)
    with pytest.raises(ValueError, match="span no area"):                         # ymin == ymax is always collinear
        delaunay_dsm(wide)
    tri, bary = grid_simplex(CloudIndex(to_dev(flat + [0, 0, 0])), 1.0)
    assert tuple(tri.shape) == (1, 5, 3) and tuple(bary.shape) == (1, 5, 3)


def test_point_count_not_a_multiple_of_the_workgroup_and_float32_input():
    from tomosar2height_amd import CloudIndex, delaunay_dsm
    pts = exact_cloud(1000 + 27, 1, extent=(33.0, 18.0))                          # 1 027 = 4 x 256 + 3
    pts = np.r_[pts, pts[:100] + [0.0, 0.0, 1.5]]
    run_small(pts)
    run_small(pts, 0.5)
    p32 = (exact_cloud(300, 2) - [389000.0, 5819000.0, 0.0]).astype(np.float32)   # float32 is widened exactly
    index, tri, dsm = run_small(p32)
    same, _ = delaunay_dsm(CloudIndex(to_dev(p32.astype(np.float64))))
    assert same.cpu().numpy().tobytes() == dsm.tobytes()


def test_hole_wider_than_several_tiles():
    """A ring of points around an empty disc of radius 40 m (five 16-node tiles across): the nodes in the hole take triangles
    whose circumcircles span it, found after many rings."""
    rng = np.random.default_rng(7)
    xy = np.floor(rng.random((6000, 2)) * 100.0 * 65536) / 65536
    xy = xy[np.hypot(xy[:, 0] - 50.0, xy[:, 1] - 50.0) > 40.0]
    pts = np.c_[389000.0 + xy[:, 0], 5819000.0 + xy[:, 1], np.round(rng.random(len(xy)) * 60 + 30, 3)]
    index, tri, dsm = run_small(pts)
    assert dsm.shape == (100, 100) and not np.isnan(dsm[20:80, 20:80]).any()
    P = index.unique.cpu().numpy()[:, :2] - index.origin
    span = np.hypot(*(P[tri[50, 50, 0]] - P[tri[50, 50, 1]]))
    assert span > 20.0                                                            # the centre's triangle crosses the hole
    # empty circumcircle of a sample of the hole's nodes, straight from the definition
    for j, i in ((50, 50), (35, 60), (62, 41), (50, 20)):
        a, b, c = P[tri[j, i]]
        if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) < 0:
            b, c = c, b
        det, bound = tin_ref.incircle(a, b, c, P)
        det[tri[j, i]] = 0.0
        assert not (det > bound).any()


def test_refusals():
    from tomosar2height_amd import CloudIndex, delaunay_dsm, grid_simplex
    pts = exact_cloud(50, 6)
    index = CloudIndex(to_dev(pts))
    for res in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="resolution"):
            delaunay_dsm(index, res)
        with pytest.raises(ValueError, match="resolution"):
            grid_simplex(index, res)
    with pytest.raises(TypeError, match="CloudIndex"):
        grid_simplex(to_dev(pts))
    with pytest.raises(RuntimeError, match="no CPU path"):
        delaunay_dsm(torch.from_numpy(pts))
    with pytest.raises(TypeError, match="float64"):
        delaunay_dsm(to_dev(pts).to(torch.int64))
    with pytest.raises(TypeError, match="torch tensor"):
        delaunay_dsm(pts)
    p = pts.copy()
    p[17, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        delaunay_dsm(to_dev(p))


def test_delaunay_raster_feeds_both_evaluators():
    """delaunay_dsm -> DSMEvaluator.eval / BuildingEvaluator.eval with no host copy in between: equal to the restatements fed
    the same raster (NaN outside the hull included)."""
    from tomosar2height_amd import BuildingEvaluator, DSMEvaluator, delaunay_dsm
    c = case("mid")
    dsm, (xmin, ymin) = delaunay_dsm(c["index"], c["resolution"])
    host = dsm.cpu().numpy()
    assert host.tobytes() == c["dev_dsm"].tobytes() and np.isnan(host).any()
    H, W = host.shape
    rng = np.random.default_rng(11)
    gt = (np.nan_to_num(host, nan=50.0) + rng.standard_normal((H, W)) * 1.5).astype(np.float32)
    mask = np.zeros((H, W), np.uint8)
    for _ in range(12):
        y, x = rng.integers(0, H - 8), rng.integers(0, W - 8)
        mask[y:y + rng.integers(2, 9), x:x + rng.integers(2, 9)] = 1
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
    assert got["n_buildings"] >= 3
