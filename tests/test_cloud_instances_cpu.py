"""CPU (no GPU needed): the numpy restatement of the point-cloud building-wise evaluation (tests/cloud_inst_ref.py) reproduces
the fixture made from the reference's own scripts/evaluator_instance.py, the inverse-transform helper is the stand-in's bit for
bit, and the boundary of include/t2h_cloud.h holds without a device."""
import numpy as np
import pytest
import torch

import cloud_inst_ref
from conftest import load_golden
from abi_ref import declared_symbols

THREE = ("RMSE-B", "MAE-B", "MedAE-B")
CASES = ("north_up", "rotated")
MODES = ("valid_only", "all")


def fixture_case(g, name):
    return {k: g[f"{name}_{k}"] for k in ("transform", "points", "mask", "dtm", "ndsm", "labels", "point_label", "counts",
                                          "pred_median", "dtm_median", "ndsm_median", "height", "three_valid_only", "three_all",
                                          "inverse")}


def sklearn_bound(K):
    """Relative.  sklearn sees a float64 prediction, so it works in float64 (printed by make_golden_cloud_instances.py): two
    summation orders of K non-negative float64 terms differ by at most 2 (K - 1) units of 2^-53, and the division and the
    root add their own roundings."""
    return 4 * K * 2.0 ** -53


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    g = load_golden("cloud_instances")
    assert [str(c) for c in g["cases"]] == list(CASES)
    c = fixture_case(g, name)
    K = int(c["labels"].max())
    assert c["points"].dtype == np.float64 and c["points"].shape[1] == 3 and 11000 < c["points"].shape[0] <= 12000
    assert c["mask"].shape == c["dtm"].shape == c["ndsm"].shape == (96, 160) and K > 90
    assert (c["counts"] == 0).sum() >= 3 and (c["counts"] == 1).sum() >= 1 and c["counts"].max() > 64
    assert not np.isnan(c["ndsm_median"]).any()
    if name == "rotated":
        assert c["transform"][1] != 0 and c["transform"][3] != 0
    for mode in MODES:
        got, rec = cloud_inst_ref.evaluate(c["points"], c["mask"], c["dtm"], c["ndsm"], c["transform"], mode)
        assert rec["n_bad"] == 0 and rec["labels"].tobytes() == c["labels"].tobytes()
        assert rec["point_label"].dtype == np.int32 and rec["point_label"].tobytes() == c["point_label"].tobytes()
        assert rec["counts"].dtype == np.int32 and rec["counts"].tobytes() == c["counts"].tobytes()
        for key in ("pred_median", "dtm_median", "ndsm_median", "height"):
            assert cloud_inst_ref.same_floats(rec[key], c[key]), key
        assert got["n_buildings"] == K and got["n_covered"] == int((c["counts"] > 0).sum()) < K
        assert got["n_valid"] == (K if mode == "all" else got["n_covered"]) and got["n_nan"] == K - got["n_valid"]
        for key, want in zip(THREE, c["three_" + mode]):
            assert abs(got[key] - float(want)) <= sklearn_bound(K) * float(want), (mode, key, got[key], float(want))
    assert not np.array_equal(c["three_all"], c["three_valid_only"])


def test_restatement_medians_follow_numpy():
    rng = np.random.default_rng(3)
    big = np.finfo(np.float64).max
    segments = [[-0.0], [-0.0, 0.0], [1.0, np.nan, 2.0], [np.inf, -np.inf], [big, big, big], [big, big], [5e-324, 0.0],
                rng.standard_normal(101), rng.integers(-3, 4, 100).astype(np.float64), []]
    z = np.concatenate([np.asarray(s, np.float64) for s in segments])
    lab = np.concatenate([np.full(len(s), k, np.int32) for k, s in enumerate(segments, 1)])
    order = rng.permutation(z.size)
    counts, med = cloud_inst_ref.point_medians(z[order], lab[order], len(segments))
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.array([np.median(np.asarray(s, np.float64)) if len(s) else np.nan for s in segments])
    assert cloud_inst_ref.same_floats(med, want) and counts.tolist() == [len(s) for s in segments]
    assert med[:2].view(np.uint64).tolist() == [0, 0] and med[4] == big and np.isinf(med[5]) and np.isnan(med[[2, 3, 9]]).all()


def test_inverse_coefficients_match_the_stand_in_bit_for_bit():
    from make_golden_cloud_instances import Transform
    from tomosar2height_amd.cloud_instances import inverse_coefficients
    g = load_golden("cloud_instances")
    rng = np.random.default_rng(4)
    transforms = [tuple(g[f"{name}_transform"]) for name in CASES]
    transforms += [tuple(rng.standard_normal(6) * (1.0, 0.1, 4e5, 0.1, 1.0, 6e6)) for _ in range(200)]
    for t in transforms:
        want = (~Transform(*t)).coeffs
        got = inverse_coefficients(t)
        assert all(type(v) is float for v in got)
        assert np.array(got).tobytes() == np.array(want).tobytes() == np.array(cloud_inst_ref.inverse(t)).tobytes(), t
    for name in CASES:
        assert np.array(inverse_coefficients(g[f"{name}_transform"])).tobytes() == g[f"{name}_inverse"].tobytes()
    assert inverse_coefficients(np.array([2.0, 0, 10, 0, -2.0, 20])) == (0.5, -0.0, -5.0, -0.0, -0.5, 10.0)
    for singular in ((1.0, 2.0, 0.0, 2.0, 4.0, 0.0), (0.0, 0.0, 1.0, 0.0, 0.0, 1.0)):
        with pytest.raises(ValueError, match="singular"):
            inverse_coefficients(singular)
    with pytest.raises(ValueError, match="six"):
        inverse_coefficients((1.0, 0.0, 0.0))


def test_cloud_header_matches_signatures_and_library():
    from tomosar2height_amd import _lib, cloud_instances, evaluator, instances, interpolate
    from tomosar2height_amd.csrc import build
    declared = declared_symbols("t2h_cloud.h")
    assert declared == sorted(cloud_instances.SIGNATURES) and len(declared) == 4
    assert all(name.startswith("t2h_cloud_") for name in declared)
    lib = cloud_instances.load()
    for name in declared:
        fn = getattr(lib, name)
        sig = cloud_instances.SIGNATURES[name]
        assert (fn.restype, list(fn.argtypes)) == (sig[0], sig[1]), name
    for name, sig in instances.SIGNATURES.items():           # load() types what the labels and raster medians go through
        assert list(getattr(lib, name).argtypes) == sig[1], name
    for header in ("t2h.h", "t2h_eval.h", "t2h_inst.h", "t2h_interp.h"):
        assert not any("t2h_cloud" in name for name in declared_symbols(header))
    others = list(_lib.SIGNATURES) + list(evaluator.SIGNATURES) + list(instances.SIGNATURES) + list(interpolate.SIGNATURES)
    assert not any("t2h_cloud" in name for name in others)
    assert _lib.ABI_VERSION == 20 == lib.t2h_abi_version()
    assert any(h.endswith("t2h_cloud.h") for h in build.PUBLIC_HEADERS)
    assert any(s.endswith("dsm_cloud.hip") for s in build.sources())
    text = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "t2h_cloud.h")).read()
    for name, value in (("TINY_MAX", cloud_instances.TINY_MAX), ("SMALL_MAX", cloud_instances.SMALL_MAX),
                        ("TABLE_COLS", cloud_instances.TABLE_COLS), ("MODE_VALID_ONLY", cloud_instances.MODES["valid_only"]),
                        ("MODE_ALL", cloud_instances.MODES["all"])):
        assert f"#define T2H_CLOUD_{name} {value} " in text, name
    assert cloud_instances.SMALL_MAX * 8 == 16 * 1024                 # the LDS of the one-workgroup sort


def test_cloud_entries_reject_bad_arguments_without_a_gpu():
    from tomosar2height_amd import cloud_instances
    lib = cloud_instances.load()
    n = None
    buf = np.zeros(1 << 16, np.float64)                   # host memory: valid-looking, aligned, never launched on
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    big, nan, inf = 1 << 30, float("nan"), float("inf")
    inv = (1.0, 0.0, -5.0, 0.0, -1.0, 9.0)
    cases = {
        # (points, N, stride, ra .. rf, labels, R, C, point_label, n_bad, stream)
        "t2h_cloud_assign": [(n, 9, 3, *inv, p, 8, 8, p, p, n), (p, 9, 3, *inv, n, 8, 8, p, p, n), (p, 9, 3, *inv, p, 8, 8, n, p, n),
                             (p, 9, 3, *inv, p, 8, 8, p, n, n), (p, -1, 3, *inv, p, 8, 8, p, p, n), (p, 1 << 31, 3, *inv, p, 8, 8, p, p, n),
                             (p, 9, 1, *inv, p, 8, 8, p, p, n), (p, 9, 3, *inv, p, 0, 8, p, p, n), (p, 9, 3, *inv, p, 8, -2, p, p, n),
                             (p, 9, 3, *inv, p, 1 << 16, 1 << 16, p, p, n), (p, 9, 3, nan, *inv[1:], p, 8, 8, p, p, n),
                             (p, 9, 3, *inv[:5], inf, p, 8, 8, p, p, n), (p + 4, 9, 3, *inv, p, 8, 8, p, p, n),
                             (p, 9, 3, *inv, p + 2, 8, 8, p, p, n)],
        # (z, stride, point_label, N, K, counts, medians, ws, ws_bytes, stream)
        "t2h_cloud_medians": [(n, 3, p, 9, 3, p, p, p, big, n), (p, 3, n, 9, 3, p, p, p, big, n), (p, 3, p, 9, 3, n, p, p, big, n),
                              (p, 3, p, 9, 3, p, n, p, big, n), (p, 3, p, 9, 3, p, p, n, big, n), (p, 0, p, 9, 3, p, p, p, big, n),
                              (p, 3, p, -1, 3, p, p, p, big, n), (p, 3, p, 1 << 31, 3, p, p, p, 1 << 40, n),
                              (p, 3, p, 9, -1, p, p, p, big, n), (p + 4, 3, p, 9, 3, p, p, p, big, n),
                              (p, 3, p, 9, 3, p, p + 4, p, big, n), (p, 3, p, 9, 3, p, p, p + 8, big, n)],
        # (pred_med, dtm_med, ref_med, counts, K, mode, n_bad, height, table, stream)
        "t2h_cloud_metrics": [(n, p, p, p, 3, 0, p, p, p, n), (p, n, p, p, 3, 0, p, p, p, n), (p, p, n, p, 3, 1, p, p, p, n),
                              (p, p, p, n, 3, 1, p, p, p, n), (p, p, p, p, 3, 1, p, n, p, n), (p, p, p, p, 3, 1, p, p, n, n),
                              (p, p, p, p, -1, 0, p, p, p, n), (p, p, p, p, 3, 2, p, p, p, n), (p, p, p, p, 3, -1, p, p, p, n),
                              (p + 4, p, p, p, 3, 0, p, p, p, n), (p, p, p, p, 3, 0, p, p + 4, p, n)],
    }
    launching = [k for k, (res, _a) in cloud_instances.SIGNATURES.items() if res is cloud_instances._i]
    assert sorted(cases) == sorted(launching)
    for name, rows in cases.items():
        for args in rows:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert len(lib.t2h_last_error_string()) > 8
    need = lib.t2h_cloud_medians_workspace_bytes(12000, 104)
    assert need >= 12 * 12000 and lib.t2h_cloud_medians_workspace_bytes(-1, 3) == 0
    assert lib.t2h_cloud_medians_workspace_bytes(1 << 31, 3) == 0 and lib.t2h_cloud_medians_workspace_bytes(100, -1) == 0
    assert lib.t2h_cloud_medians_workspace_bytes(0, 5) > 0          # no point at all is legal: every building is uncovered
    assert lib.t2h_cloud_medians(p, 3, p, 12000, 104, p, p, p, need - 1, n) == -3
    assert b"workspace" in lib.t2h_last_error_string()
    # linear in the points: the documented constants bound the workspace of the Berlin chunk's cloud
    N, K = 3_200_000, 5000
    assert lib.t2h_cloud_medians_workspace_bytes(N, K) <= 12 * N + (N // 2049 + 1) * (32 + 2048) + 12 * K + 8 * 5 + 12 * 256
    # K = 0 is valid and launches nothing
    assert lib.t2h_cloud_medians(p, 3, p, 9, 0, n, n, p, big, n) == 0


def test_cloud_instances_have_no_cpu_path():
    import tomosar2height_amd
    from tomosar2height_amd import CloudBuildingEvaluator, assign_points, cloud_instances, point_medians
    assert tomosar2height_amd.CloudBuildingEvaluator is cloud_instances.CloudBuildingEvaluator
    assert tomosar2height_amd.assign_points is cloud_instances.assign_points
    north_up = (1.0, 0.0, 0.0, 0.0, -1.0, 4.0)
    pts = torch.zeros(5, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        assign_points(pts, torch.zeros(4, 4, dtype=torch.int32), north_up)
    with pytest.raises(RuntimeError, match="no CPU path"):
        point_medians(pts, torch.zeros(5, dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        point_medians(pts[:, 2], torch.zeros(5, dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        CloudBuildingEvaluator(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4), torch.zeros(4, 4), north_up)
    with pytest.raises(ValueError, match="singular"):         # refused before anything touches a device
        assign_points(pts, torch.zeros(4, 4, dtype=torch.int32), (1.0, 1.0, 0.0, 1.0, 1.0, 0.0))
