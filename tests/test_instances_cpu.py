"""CPU (no GPU needed): the numpy restatement of the building-wise evaluation (tests/inst_ref.py) reproduces the fixture made
from the reference's own scripts/evaluator_instance.py, and the boundary of include/t2h_inst.h holds without a device."""
import numpy as np
import pytest
import torch

import inst_ref
from conftest import load_golden
from abi_ref import declared_symbols

THREE = ("RMSE-B", "MAE-B", "MedAE-B")


def reference_bound(*medians):
    """sklearn works in float32 there (a rounding in the subtraction, a float32 mean, a square root): 16 float32 ulps of the
    largest median, absolute."""
    return 2.0 ** -20 * max(float(np.abs(m).max()) for m in medians)


def test_restatement_reproduces_the_reference_fixture():
    g = load_golden("building_instances")
    for pred, suffix in ((g["pred"], ""), (g["pred64"], "64")):
        got, labels, counts, pm, gm = inst_ref.evaluate(pred, g["gt"], g["mask"])
        assert labels.dtype == np.int32 and labels.tobytes() == g["labels"].tobytes()
        assert got["n_buildings"] == int(g["labels"].max()) == 145 and got["n_nan"] == 0
        assert np.array_equal(counts, np.bincount(g["labels"].ravel())[1:])
        assert pm.tobytes() == g["pred" + suffix + "_median"].tobytes() and gm.tobytes() == g["gt_median"].tobytes()
        bound = reference_bound(pm, gm)
        for key, want in zip(THREE, g["three" + suffix]):
            assert abs(got[key] - float(want)) <= bound, (key, got[key], float(want), bound)
    assert (counts % 2 == 0).sum() > 10 and counts.min() == 1 and counts.max() > 300
    t_row, l_col, H, W = (int(v) for v in g["window"])
    win = (slice(t_row, t_row + H), slice(l_col, l_col + W))
    got, labels, _, pm, gm = inst_ref.evaluate(g["pred"][win], g["gt"][win], g["mask"][win])
    assert labels.tobytes() == g["labels_window"].tobytes()
    assert pm.tobytes() == g["pred_median_window"].tobytes() and gm.tobytes() == g["gt_median_window"].tobytes()
    for key, want in zip(THREE, g["three_window"]):
        assert abs(got[key] - float(want)) <= reference_bound(pm, gm), (key, got[key], float(want))


def test_restatement_labels_the_structural_masks_like_scipy():
    g = load_golden("building_instances")
    names = [str(n) for n in g["structural"]]
    assert len(names) == 12
    for name in names:
        for conn in (1, 2):
            labels, K = inst_ref.label(g[f"s_{name}"], conn)
            want = g[f"s_{name}_labels{conn}"]
            assert labels.tobytes() == want.tobytes() and K == int(want.max()), (name, conn)
    assert int(g["s_checker_67x131_labels1"].max()) == 4389 and int(g["s_checker_67x131_labels2"].max()) == 1
    assert int(g["s_corner_diagonals_labels1"].max()) == 4 and int(g["s_corner_diagonals_labels2"].max()) == 2


def test_restatement_medians_follow_numpy():
    rng = np.random.default_rng(1)
    labels = rng.integers(0, 9, (40, 50)).astype(np.int32)
    values = rng.standard_normal((40, 50)).astype(np.float32)
    values[labels == 3] = np.float32(-0.0)
    values[3, 4] = np.nan
    labels[3, 4] = 7
    values[np.nonzero(labels == 5)[0][0], np.nonzero(labels == 5)[1][0]] = np.inf
    counts, med = inst_ref.segment_medians(values, labels, 9)          # label 9 has no pixel
    want = np.array([np.median(values[labels == k]) if (labels == k).any() else np.nan for k in range(1, 10)], np.float32)
    assert inst_ref.same_floats(med, want) and counts[8] == 0 and np.isnan(med[6]) and np.isnan(med[8])
    assert not np.signbit(med[2]) and med[2] == 0                     # numpy's mean turns -0 into +0


def test_inst_header_matches_signatures_and_library():
    from tomosar2height_amd import _lib, evaluator, instances
    declared = declared_symbols("t2h_inst.h")
    assert declared == sorted(instances.SIGNATURES) and len(declared) == 5
    assert all(name.startswith("t2h_inst_") for name in declared)
    lib = instances.load()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (instances.SIGNATURES[name][0], instances.SIGNATURES[name][1]), name
    for header in ("t2h.h", "t2h_eval.h"):
        assert not any("t2h_inst" in name for name in declared_symbols(header))
    assert not any("t2h_inst" in name for name in list(_lib.SIGNATURES) + list(evaluator.SIGNATURES))
    assert _lib.ABI_VERSION == 20 == lib.t2h_abi_version()
    text = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "t2h_inst.h")).read()
    for name, value in (("TILE", instances.TILE), ("TINY_MAX", instances.TINY_MAX), ("SMALL_MAX", instances.SMALL_MAX),
                        ("TABLE_COLS", instances.TABLE_COLS)):
        assert f"#define T2H_INST_{name} {value} " in text, name


def test_inst_entries_reject_bad_arguments_without_a_gpu():
    from tomosar2height_amd import instances
    lib = instances.load()
    n = None
    buf = np.zeros(1 << 16, np.float64)                   # host memory: valid-looking, aligned, never launched on
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    big = 1 << 30
    cases = {
        # (mask, ld, R, C, connectivity, labels, n_labels, ws, ws_bytes, stream)
        "t2h_inst_label": [(n, 8, 8, 8, 2, p, p, p, big, n), (p, 8, 8, 8, 2, n, p, p, big, n), (p, 8, 8, 8, 2, p, n, p, big, n),
                           (p, 8, 8, 8, 2, p, p, n, big, n), (p, 8, 8, 8, 0, p, p, p, big, n), (p, 8, 8, 8, 3, p, p, p, big, n),
                           (p, 8, 0, 8, 2, p, p, p, big, n), (p, 8, 8, -1, 2, p, p, p, big, n), (p, 7, 8, 8, 2, p, p, p, big, n),
                           (p, 1 << 16, 1 << 16, 1 << 16, 2, p, p, p, big, n)],
        # (values, is_f64, ld, H, W, labels, K, counts, medians, ws, ws_bytes, stream)
        "t2h_inst_medians": [(n, 0, 8, 8, 8, p, 3, p, p, p, big, n), (p, 0, 8, 8, 8, n, 3, p, p, p, big, n),
                             (p, 0, 8, 8, 8, p, 3, n, p, p, big, n), (p, 0, 8, 8, 8, p, 3, p, n, p, big, n),
                             (p, 0, 8, 8, 8, p, 3, p, p, n, big, n), (p, 0, 8, 0, 8, p, 3, p, p, p, big, n),
                             (p, 0, 8, 8, 0, p, 3, p, p, p, big, n), (p, 0, 7, 8, 8, p, 3, p, p, p, big, n),
                             (p, 0, 8, 8, 8, p, -1, p, p, p, big, n), (p, 0, 8, 8, 8, p, 65, p, p, p, big, n),
                             (p, 2, 8, 8, 8, p, 3, p, p, p, big, n), (p + 4, 1, 8, 8, 8, p, 3, p, p, p, big, n)],
        # (pred_med, gt_med, K, table, stream)
        "t2h_inst_metrics": [(n, p, 3, p, n), (p, n, 3, p, n), (p, p, 3, n, n), (p, p, -1, p, n)],
    }
    launching = [k for k, (res, _a) in instances.SIGNATURES.items() if res is instances._i]
    assert sorted(cases) == sorted(launching)
    for name, rows in cases.items():
        for args in rows:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert len(lib.t2h_last_error_string()) > 8
    need = lib.t2h_inst_label_workspace_bytes(70, 101)
    assert need >= 4 * 70 * 101 and lib.t2h_inst_label_workspace_bytes(0, 5) == 0
    assert lib.t2h_inst_label_workspace_bytes(1 << 16, 1 << 16) == 0
    assert lib.t2h_inst_label(p, 101, 70, 101, 2, p, p, p, need - 1, n) == -3
    assert b"workspace" in lib.t2h_last_error_string()
    need = lib.t2h_inst_medians_workspace_bytes(70 * 101, 40)
    assert need >= 8 * 70 * 101 and lib.t2h_inst_medians_workspace_bytes(0, 0) == 0
    assert lib.t2h_inst_medians_workspace_bytes(100, 101) == 0 and lib.t2h_inst_medians_workspace_bytes(100, -1) == 0
    assert lib.t2h_inst_medians(p, 0, 101, 70, 101, p, 40, p, p, p, need - 1, n) == -3
    assert b"workspace" in lib.t2h_last_error_string()
    # linear in the pixels: the documented constants bound the Berlin chunk's workspace
    n_px, K = 1660 * 1990, 5000
    assert lib.t2h_inst_medians_workspace_bytes(n_px, K) <= 8 * n_px + (n_px // 2049 + 1) * (24 + 2048) + 12 * K + 8 * 5 + 12 * 256
    # K = 0 is valid and launches nothing
    assert lib.t2h_inst_medians(p, 0, 8, 8, 8, p, 0, p, p, p, big, n) == 0


def test_instances_have_no_cpu_path():
    import tomosar2height_amd
    from tomosar2height_amd import BuildingEvaluator, instances, label_components, segment_medians
    assert tomosar2height_amd.BuildingEvaluator is instances.BuildingEvaluator
    assert tomosar2height_amd.label_components is instances.label_components
    with pytest.raises(RuntimeError, match="no CPU path"):
        label_components(torch.zeros(4, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        segment_medians(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32), 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        BuildingEvaluator(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4), bounds=(0.0, 4.0))
    ev = BuildingEvaluator.__new__(BuildingEvaluator)
    ev.left, ev.top, ev.pixel_size = 10.0, 788.0, (1.0, 2.0)
    assert ev.window((10.5, 787.5)) == (0, 0) and ev.window((522.49, 276.5)) == (512, 255)
    ev.gt_dsm = torch.zeros(4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.eval(torch.zeros(4, 4))
