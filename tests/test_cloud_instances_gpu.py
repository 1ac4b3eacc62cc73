"""Device point-cloud building-wise metrics (tomosar2height_amd.cloud_instances, csrc/dsm_cloud.hip) against the fixture made
from the reference's scripts/evaluator_instance.py:139-291 and against the numpy restatement tests/cloud_inst_ref.py.

Point labels, per-building counts, float64 medians and heights are compared byte for byte (any NaN equals any NaN).  MedAE-B
is an exact order statistic of exactly computed |d|: byte-equal to the restatement.  MAE-B and RMSE-B are compared with the
restatement's (math.fsum) to 1e-12 relative, the bar for fixed-order float64 sums in test_instances_gpu.py, and with the
reference's sklearn numbers to 4 K 2^-53 relative: sklearn sees a float32 y_true beside a float64 y_pred and works in float64
(printed by tests/golden/make_golden_cloud_instances.py), two summation orders of K non-negative float64 terms differ by at
most 2 (K - 1) units of 2^-53, and the division and the root add their own roundings.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cloud_inst_ref
from cloud_inst_ref import same_floats
from conftest import ROOT, load_golden
from test_cloud_instances_cpu import CASES, MODES, THREE, fixture_case, sklearn_bound

pytestmark = pytest.mark.gpu

UNIT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)                         # pixel (col, row) covers [col, col + 1) x [row, row + 1)
SIZES = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 9001]         # 9 001 compacted keys span three chunks of 4 096


def dev():
    return torch.device("cuda:0")


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(rec):
    return {k: v.cpu().numpy() for k, v in rec.items()}


def assert_metrics(got, want):
    """Integers and MedAE-B / max_abs exact, the two sums to 1e-12 relative."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key, w in want.items():
        g = got[key]
        print(key, g, w)
        if w is None or isinstance(w, int):
            assert g == w and type(g) is type(w), (key, g, w)
        elif key in ("MedAE-B", "max_abs"):
            assert isinstance(g, float) and (g == w or (np.isnan(g) and np.isnan(w))), (key, g, w)
        else:
            assert isinstance(g, float) and (g == w or abs(g - w) <= 1e-12 * abs(w)), (key, g, w)


def check_eval(ev, points, mask, dtm, ndsm, transform, mode):
    """One eval against the restatement; returns (metrics, record as numpy)."""
    got, rec = ev.eval(to_dev(points), mode=mode)
    want, ref = cloud_inst_ref.evaluate(points, mask, dtm, ndsm, transform, mode)
    assert all(v.is_cuda for v in rec.values())
    rec = host(rec)
    assert ref["n_bad"] == 0
    for key in ("labels", "point_label", "counts"):
        assert rec[key].dtype == np.int32 and rec[key].tobytes() == ref[key].tobytes(), key
    for key in ("pred_median", "dtm_median", "ndsm_median", "height"):
        assert same_floats(rec[key], ref[key]), key
    assert_metrics(got, want)
    return got, rec


def evaluator(mask, dtm, ndsm, transform, **kw):
    from tomosar2height_amd import CloudBuildingEvaluator
    return CloudBuildingEvaluator(to_dev(mask), to_dev(dtm), to_dev(ndsm), tuple(transform), **kw)


@pytest.mark.parametrize("name", CASES)
def test_fixture_case_matches_the_reference(name):
    c = fixture_case(load_golden("cloud_instances"), name)
    K = int(c["labels"].max())
    ev = evaluator(c["mask"], c["dtm"], c["ndsm"], c["transform"])
    for mode in MODES:
        got, rec = check_eval(ev, c["points"], c["mask"], c["dtm"], c["ndsm"], c["transform"], mode)
        for key in ("labels", "point_label", "counts"):
            assert rec[key].tobytes() == c[key].tobytes(), key
        for key in ("pred_median", "dtm_median", "ndsm_median", "height"):
            assert same_floats(rec[key], c[key]), key
        for key, want in zip(THREE, c["three_" + mode]):
            print(mode, key, got[key], float(want), abs(got[key] - float(want)) / float(want), sklearn_bound(K))
            assert abs(got[key] - float(want)) <= sklearn_bound(K) * float(want), (mode, key, got[key], float(want))
        covered = int((c["counts"] > 0).sum())
        assert got["n_buildings"] == K and got["n_covered"] == covered < K
        assert (got["n_valid"], got["n_nan"]) == ((K, 0) if mode == "all" else (covered, K - covered))
    assert ev.buildings()[3] is ev.buildings()[3]                 # labels and raster medians are computed once


def cloud_of(segments, seed, extra=500):
    """Points in shuffled order over a [1, len + 1] label plane (pixel j has label j; pixel 0 is background): building k
    receives exactly ``segments[k - 1]`` as its z values; ``extra`` points fall on the background."""
    rng = np.random.default_rng(seed)
    K = len(segments)
    labels = np.arange(K + 1, dtype=np.int32)[None, :]
    z = np.concatenate([np.asarray(s, np.float64) for s in segments] + [rng.standard_normal(extra)])
    col = np.concatenate([np.full(len(s), k, np.float64) for k, s in enumerate(segments, 1)] + [np.zeros(extra)])
    pts = np.stack([col + rng.random(z.size) * 0.999, rng.random(z.size) * 0.999, z], 1)
    return pts[rng.permutation(z.size)], labels


def check_medians(segments, seed=0):
    from tomosar2height_amd import assign_points, point_medians
    pts, labels = cloud_of(segments, seed)
    K = len(segments)
    p_dev = to_dev(pts)
    point_label = assign_points(p_dev, to_dev(labels), UNIT)
    want_label, _ = cloud_inst_ref.assign(pts, labels, UNIT)
    assert point_label.dtype == torch.int32 and point_label.cpu().numpy().tobytes() == want_label.tobytes()
    counts, med = point_medians(p_dev, point_label, K)
    assert counts.dtype == torch.int32 and med.dtype == torch.float64 and med.is_cuda
    want_counts, want = cloud_inst_ref.point_medians(pts[:, 2], want_label, K)
    assert counts.cpu().numpy().tobytes() == want_counts.tobytes() and want_counts.tolist() == [len(s) for s in segments]
    got = med.cpu().numpy()
    assert same_floats(got, want), np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0][:10]
    with np.errstate(invalid="ignore", over="ignore"):
        numpy_median = np.array([np.median(np.asarray(s, np.float64)) if len(s) else np.nan for s in segments])
    assert same_floats(got, numpy_median)
    z_only, med_z = point_medians(p_dev[:, 2], point_label, K)                  # a strided 1-D view of z
    assert z_only.cpu().numpy().tobytes() == want_counts.tobytes() and same_floats(med_z.cpu().numpy(), want)
    return got


@pytest.mark.parametrize("bump", (0, 1))
def test_medians_every_size_class(bump):
    """0, 1, 2; the one-wave class up to 64; the LDS sort up to 2 048; the radix select above: each threshold - 1, at it, + 1,
    with odd and even counts (bump), continuous z and z from about 50 values (long runs of equal digits in the radix passes)."""
    rng = np.random.default_rng(7 + bump)
    sizes = [n + bump if n else 0 for n in SIZES]
    check_medians([rng.standard_normal(n) * 10 + 40 for n in sizes], seed=1)
    check_medians([np.round(rng.standard_normal(n) * 8) * 0.125 for n in sizes], seed=2)


def test_medians_special_values():
    rng = np.random.default_rng(9)
    inf, nan, big, tiny = np.inf, np.nan, np.finfo(np.float64).max, 5e-324
    last_byte = lambda n: (1.0 + np.arange(n, dtype=np.float64) * 2.0 ** -52)[rng.permutation(n)]      # n <= 256: one digit
    segments = [
        np.full(5, 3.25), np.full(70, 3.25), np.full(2500, -3.25),                                    # all equal
        last_byte(64), last_byte(255), last_byte(256), np.tile(last_byte(256), 10), -np.tile(last_byte(255), 9),
        [-0.0], [-0.0, 0.0], [0.0, -0.0, -0.0], np.where(rng.random(2600) < 0.5, -0.0, 0.0),          # signed zeros
        [inf], [-inf, inf], [-inf, -inf, 1.0], [1.0, inf, inf, 2.0], np.r_[rng.standard_normal(2100), np.full(2200, inf)],
        np.r_[rng.standard_normal(2100), np.full(2200, -inf)],
        [tiny, 0.0, -tiny], [tiny, 2 * tiny], np.r_[np.arange(3000) * tiny, -np.arange(100) * tiny],  # denormals
        [big, big, big], [big, big], np.full(2501, -big),                                             # x + x would overflow
        [1.0, nan, 2.0], [nan, 1.0], [nan], np.r_[rng.standard_normal(99), nan], np.r_[rng.standard_normal(100), -nan],
        np.r_[rng.standard_normal(2999), nan], np.r_[rng.standard_normal(3000), nan], np.r_[np.full(2500, inf), nan],
    ]
    got = check_medians(segments, seed=4)
    assert np.nonzero(np.isnan(got))[0].tolist() == [13] + list(range(24, 32))                        # (-inf + inf) / 2, and the NaNs
    assert got[8:12].view(np.uint64).tolist() == [0, 0, 0, 0]                                         # +0, as numpy's mean
    assert got[21] == big and np.isinf(got[22]) and got[23] == -big


def test_geometry_edges_outside_and_flipped_rows():
    from tomosar2height_amd import assign_points
    R, C = 5, 7
    labels = (np.arange(R * C, dtype=np.int32) + 1).reshape(R, C)
    # north-up with a negative e: row = (top - y) / 2, col = (x - left) / 0.5
    t = (0.5, 0.0, 100.0, 0.0, -2.0, 50.0)
    xs = [100.0, 100.0 - 1e-9, 103.5, 103.5 - 1e-9, 103.5 + 1e-9, 101.0, 101.5, 1e300, -1e300, 100.25, 100.25, 100.25, 100.25]
    ys = [50.0, 50.0, 50.0, 50.0, 50.0, 48.0, 46.0, 45.0, 45.0, 1e300, -1e300, 40.0, 40.0 - 1e-9]
    pts = np.stack([xs, ys, np.zeros(len(xs))], 1)
    want, n_bad = cloud_inst_ref.assign(pts, labels, t)
    assert n_bad == 0
    #            fx = 0  < 0   = C   < C   > C   (2, 1)  (3, 2)  far right / left      far up / down        fy = R, just below
    assert want.tolist() == [1, 1, 7, 7, 7, 10, 18, 7 * 2 + 7, 7 * 2 + 1, 1, 29, 29, 29]
    got = assign_points(to_dev(pts), to_dev(labels), t)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    # one pixel: everything lands on it
    one = assign_points(to_dev(pts), to_dev(np.array([[9]], np.int32)), t)
    assert one.cpu().numpy().tolist() == [9] * len(xs)
    # a rotated transform and many points exactly on pixel corners
    rng = np.random.default_rng(11)
    t = (0.5, 0.125, 392000.25, -0.0625, -0.5, 5820000.5)
    labels = rng.integers(0, 50, (37, 61)).astype(np.int32)
    col, row = rng.integers(-3, 65, 5000).astype(np.float64), rng.integers(-3, 41, 5000).astype(np.float64)
    pts = np.stack([col * t[0] + row * t[1] + t[2], col * t[3] + row * t[4] + t[5], rng.standard_normal(5000)], 1)
    want, n_bad = cloud_inst_ref.assign(pts, labels, t)
    got = assign_points(to_dev(pts), to_dev(labels), t)
    assert n_bad == 0 and got.cpu().numpy().tobytes() == want.tobytes()


def small_case(seed=5, R=24, C=31, n_points=900):
    rng = np.random.default_rng(seed)
    mask = np.zeros((R, C), np.uint8)
    for _ in range(9):
        y, x = rng.integers(0, R - 3), rng.integers(0, C - 3)
        mask[y:y + rng.integers(1, 6), x:x + rng.integers(1, 6)] = 1
    dtm = (rng.standard_normal((R, C)) + 30).astype(np.float32)
    ndsm = (np.abs(rng.standard_normal((R, C))) * 3 + 8 * mask).astype(np.float32)
    t = (1.0, 0.0, 392000.0, 0.0, -1.0, 5820000.0 + R)
    pts = np.stack([392000.0 + rng.random(n_points) * C, 5820000.0 + rng.random(n_points) * R,
                    38 + rng.standard_normal(n_points)], 1)
    return mask, dtm, ndsm, t, pts


def test_degenerate_inputs_and_refusals():
    from tomosar2height_amd import CloudBuildingEvaluator, assign_points, point_medians
    mask, dtm, ndsm, t, pts = small_case()
    ev = evaluator(mask, dtm, ndsm, t)
    K = ev.buildings()[1]
    assert K > 3
    # N = 0: every building is uncovered
    none = np.zeros((0, 3))
    got, rec = check_eval(ev, none, mask, dtm, ndsm, t, "valid_only")
    assert got["n_valid"] == 0 and got["n_covered"] == 0 and got["n_nan"] == K and got["RMSE-B"] is None and got["MedAE-B"] is None
    assert rec["point_label"].shape == (0,) and not rec["counts"].any() and np.isnan(rec["pred_median"]).all()
    got, rec = check_eval(ev, none, mask, dtm, ndsm, t, "all")
    assert got["n_valid"] == K and got["n_covered"] == 0 and got["RMSE-B"] > 0
    # N = 1, and a strided view of a wider point list
    check_eval(ev, pts[:1], mask, dtm, ndsm, t, "all")
    wide = to_dev(np.concatenate([pts, np.full((pts.shape[0], 2), np.nan)], 1))
    a, rec_a = ev.eval(wide[:, :3], mode="all")
    b, rec_b = check_eval(ev, pts, mask, dtm, ndsm, t, "all")
    assert not wide[:, :3].is_contiguous() and a == b
    for key in ("point_label", "counts", "pred_median", "height"):
        assert rec_a[key].cpu().numpy().tobytes() == rec_b[key].tobytes(), key
    # K = 0
    empty = evaluator(np.zeros_like(mask), dtm, ndsm, t)
    got, rec = empty.eval(to_dev(pts), mode="all")
    assert got == {"RMSE-B": None, "MAE-B": None, "MedAE-B": None, "max_abs": None, "n_buildings": 0, "n_valid": 0, "n_nan": 0,
                   "n_covered": 0}
    assert rec["counts"].numel() == 0 and rec["height"].numel() == 0 and not rec["point_label"].any()
    counts, med = point_medians(to_dev(pts), torch.zeros(pts.shape[0], dtype=torch.int32, device=dev()), 0)
    assert counts.numel() == 0 and med.numel() == 0 and med.dtype == torch.float64
    # refusals
    labels = ev.buildings()[0]
    with pytest.raises(TypeError, match="float64"):
        ev.eval(to_dev(pts.astype(np.float32)))
    with pytest.raises(TypeError, match="float64"):
        assign_points(to_dev(pts.astype(np.float32)), labels, t)
    bad = pts.copy()
    bad[3, 0], bad[7, 1], bad[9, 0] = np.nan, np.inf, -np.inf
    with pytest.raises(ValueError, match="3 of 900 points"):
        ev.eval(to_dev(bad))
    with pytest.raises(ValueError, match="3 of 900 points"):
        assign_points(to_dev(bad), labels, t)
    bad_z = pts.copy()
    bad_z[:, 2] = np.nan                                          # a NaN z is data, not a refusal: NaN medians
    got, _ = check_eval(ev, bad_z, mask, dtm, ndsm, t, "valid_only")
    assert got["n_valid"] == 0 and got["n_covered"] > 0
    for singular in ((1.0, 2.0, 0.0, 2.0, 4.0, 0.0), (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)):
        with pytest.raises(ValueError, match="singular"):
            CloudBuildingEvaluator(to_dev(mask), to_dev(dtm), to_dev(ndsm), singular)
        with pytest.raises(ValueError, match="singular"):
            assign_points(to_dev(pts), labels, singular)
    with pytest.raises(ValueError, match="mode"):
        ev.eval(to_dev(pts), mode="some")
    nan_ndsm = ndsm.copy()
    nan_ndsm[mask != 0] = np.nan
    ev_nan = evaluator(mask, dtm, nan_ndsm, t)
    with pytest.raises(ValueError, match="nDSM medians are NaN"):
        ev_nan.eval(to_dev(pts), mode="all")
    got, _ = check_eval(ev_nan, pts, mask, dtm, nan_ndsm, t, "valid_only")
    assert got["n_valid"] == 0 and got["n_nan"] == K


def test_modes_differ_on_uncovered_buildings():
    mask, dtm, ndsm, t, pts = small_case(seed=6)
    labels, K = cloud_inst_ref.inst_ref.label(mask)
    point_label, _ = cloud_inst_ref.assign(pts, labels, t)
    pts = pts[(point_label != 2) & (point_label != K)]            # two buildings lose all their points
    ev = evaluator(mask, dtm, ndsm, t)
    only, rec = check_eval(ev, pts, mask, dtm, ndsm, t, "valid_only")
    every, rec_all = check_eval(ev, pts, mask, dtm, ndsm, t, "all")
    assert rec["counts"][1] == 0 and rec["counts"][K - 1] == 0 and np.isnan(rec["height"][[1, K - 1]]).all()
    assert rec_all["height"].tobytes() == rec["height"].tobytes()           # before any NaN handling, in both modes
    covered = int((rec["counts"] > 0).sum())
    assert (only["n_valid"], only["n_nan"], only["n_covered"]) == (covered, K - covered, covered) and covered <= K - 2
    assert (every["n_valid"], every["n_nan"], every["n_covered"]) == (K, 0, covered)
    # an uncovered building counts as height 0 in "all": its |d| is its nDSM median
    d = np.abs(rec["ndsm_median"].astype(np.float64) - np.nan_to_num(rec["height"]))
    assert every["max_abs"] == d.max() and every["MedAE-B"] == float(np.median(d))
    assert every["MAE-B"] != only["MAE-B"] and every["RMSE-B"] > only["RMSE-B"]


def test_permuted_points_give_the_same_bytes():
    rng = np.random.default_rng(12)
    segments = [rng.standard_normal(n) for n in (1, 40, 64, 700, 2048, 5000, 2)]
    pts, labels = cloud_of(segments, seed=13)
    from tomosar2height_amd import assign_points, point_medians
    runs = []
    for order in (np.arange(pts.shape[0]), rng.permutation(pts.shape[0]), rng.permutation(pts.shape[0])):
        p = to_dev(pts[order])
        counts, med = point_medians(p, assign_points(p, to_dev(labels), UNIT), len(segments))
        runs.append((counts.cpu().numpy().tobytes(), med.cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2]


def float32_segments(seed=31):
    """Every size class of both key widths as float32 values that are multiples of 0.25 below 2^10: the mean of any two is a
    multiple of 0.125 and a float32, so np.median is exact in float32 and in float64 and no double rounding can enter."""
    rng = np.random.default_rng(seed)
    sizes = (1, 2, 64, 65, 2048, 2049, 4097, 9001)
    segments = [(np.round(rng.standard_normal(n) * 64) / 4 + 0.0).astype(np.float32) for n in sizes]   # (+ 0.0: no -0.0)
    segments[1][:] = (-1.5, 2.25)                                                # even count, opposite-signed middle pair
    segments[3][:] = -0.0                                                        # only negative zeros
    segments[4] = np.r_[-np.abs(segments[4][:1024]) - 0.25, np.abs(segments[4][1024:]) + 0.25][rng.permutation(2048)]
    segments[5][rng.integers(2049)] = np.nan
    return segments


def test_raster_and_cloud_medians_are_one_algorithm():
    """The float32 entry (segment_medians, 32-bit keys) and the float64 entry (point_medians, 64-bit keys) on the same
    segments: equal counts, and the raster medians are the cloud medians rounded once to float32, bit for bit."""
    from tomosar2height_amd import point_medians, segment_medians
    segments = float32_segments()
    K, total = len(segments), sum(s.size for s in segments)
    with np.errstate(invalid="ignore"):
        want32 = np.array([np.median(s) for s in segments], np.float32)
        want64 = np.array([np.median(s.astype(np.float64)) for s in segments], np.float64)
    nan = np.isnan(want64)
    assert nan.tolist() == [k == 5 for k in range(K)] and np.isnan(want32).tolist() == nan.tolist()
    assert want32[~nan].tobytes() == want64[~nan].astype(np.float32).tobytes()   # the inputs allow the comparison below
    middle = np.sort(segments[4])[1023:1025]
    assert want64[1] == 0.375 and middle[0] < 0 < middle[1] and want64[3].tobytes() == np.float64(0.0).tobytes()

    H, W = 131, 133                                                              # 17 423 pixels for 17 327 values
    values = np.zeros(H * W, np.float32)
    labels = np.zeros(H * W, np.int32)
    values[:total] = np.concatenate(segments)
    labels[:total] = np.concatenate([np.full(s.size, k, np.int32) for k, s in enumerate(segments, 1)])
    counts_r, med_r = segment_medians(to_dev(values.reshape(H, W)), to_dev(labels.reshape(H, W)), K)
    order = np.random.default_rng(32).permutation(H * W)
    counts_c, med_c = point_medians(to_dev(values.astype(np.float64)[order]), to_dev(labels[order]), K)
    assert med_r.dtype == torch.float32 and med_c.dtype == torch.float64
    counts_r, med_r, counts_c, med_c = (t.cpu().numpy() for t in (counts_r, med_r, counts_c, med_c))
    print(counts_r.tolist(), med_r.tolist(), med_c.tolist())
    assert counts_r.tolist() == counts_c.tolist() == [s.size for s in segments]
    assert np.isnan(med_r).tolist() == np.isnan(med_c).tolist() == nan.tolist()
    assert med_r[~nan].tobytes() == med_c[~nan].astype(np.float32).tobytes()
    assert med_r[~nan].tobytes() == want32[~nan].tobytes() and med_c[~nan].tobytes() == want64[~nan].tobytes()


def test_module_loads_alone_in_a_fresh_process():
    """Nothing but cloud_instances is imported: its load() must type what the labels (an int32 mask goes through the
    evaluator's predicate) and the raster medians call."""
    code = (
        "import torch\n"
        "from tomosar2height_amd.cloud_instances import CloudBuildingEvaluator\n"
        "d = torch.device('cuda:0')\n"
        "mask = torch.zeros(6, 8, dtype=torch.int32, device=d); mask[1:4, 2:5] = 7\n"
        "dtm = torch.full((6, 8), 2.0, device=d); ndsm = torch.full((6, 8), 5.0, dtype=torch.float64, device=d)\n"
        "ev = CloudBuildingEvaluator(mask, dtm, ndsm, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0))\n"
        "pts = torch.tensor([[2.5, 1.5, 9.0], [3.5, 2.5, 8.0], [0.5, 0.5, 100.0]], dtype=torch.float64, device=d)\n"
        "m, rec = ev.eval(pts, mode='valid_only')\n"
        "assert m['n_buildings'] == 1 and m['n_valid'] == 1 and m['MAE-B'] == 1.5 and m['MedAE-B'] == 1.5, m\n"
        "assert rec['point_label'].tolist() == [1, 1, 0] and rec['pred_median'].tolist() == [8.5]\n"
        "print('alone ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "alone ok" in out.stdout, out.stdout + out.stderr
