"""CPU (no GPU needed): the numpy restatement of the DSM evaluation (tests/eval_ref.py) reproduces the fixture made from the
reference's own DSMEvaluator.eval / dilate_mask, and the boundary of include/t2h_eval.h holds without a device."""
import numpy as np
import pytest
import torch

import eval_ref
from abi_ref import declared_symbols
from conftest import load_golden


def fixture_stats(g):
    keys = [str(k) for k in g["stat_keys"]]
    assert tuple(keys) == eval_ref.STAT_KEYS
    out = {}
    for name, row, none in zip(g["names"], g["table"], g["is_none"]):
        out[str(name)] = {k: None if isnone else (int(v) if k == "n_pixel" else float(v)) for k, v, isnone in zip(keys, row, none)}
    return out


def fixture_masks(g):
    return {"building": g["building"], "type": g["type"], "water": g["water"], "nothing": g["nothing"]}


def test_restatement_reproduces_the_reference_fixture():
    g = load_golden("dsm_evaluator")
    t_row, l_col = (int(v) for v in g["window"])
    stats, diff = eval_ref.evaluate(g["target"], g["gt"], g["gt_mask"], fixture_masks(g), t_row, l_col)
    want = fixture_stats(g)
    assert all(v is None for v in want["nothing"].values()) and want["overall"]["n_pixel"] > 7000
    eval_ref.assert_stats(stats, want)
    eval_ref.assert_diff(diff, g["diff"])
    assert np.isnan(g["diff"]).sum() > 100
    for k in (1, 2, 3):
        for plane in ("building", "corners", "line"):
            assert np.array_equal(eval_ref.dilate(g[plane], k), g[f"{plane}_dilated{k}"]), (plane, k)


def test_eval_header_matches_signatures_and_library():
    from tomosar2height_amd import _lib, evaluator
    declared = declared_symbols("t2h_eval.h")
    assert declared == sorted(evaluator.SIGNATURES) and len(declared) == 6
    assert all(name.startswith("t2h_eval_") for name in declared)
    lib = evaluator.load()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (evaluator.SIGNATURES[name][0], evaluator.SIGNATURES[name][1]), name
    # the pinned header and table stay as they were: nothing of the evaluator in them, same ABI version
    assert not any("eval" in name for name in declared_symbols("t2h.h"))
    assert not any(name.startswith("t2h_eval") for name in _lib.SIGNATURES)
    assert sorted(_lib.SIGNATURES) == declared_symbols("t2h.h")
    assert _lib.ABI_VERSION == 20 == lib.t2h_abi_version()


def test_eval_entries_reject_bad_arguments_without_a_gpu():
    from tomosar2height_amd import _lib, evaluator
    lib = evaluator.load()
    n = None
    buf = np.zeros(4096, np.float64)                      # host memory: valid-looking, aligned, never launched on
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    cases = {
        "t2h_eval_predicate": [(n, 0, 0, 0.0, n, 100, n), (p, 9, 0, 0.0, p, 100, n), (p, 0, 3, 0.0, p, 100, n), (p, 0, 0, 0.0, p, 0, n)],
        "t2h_eval_dilate": [(n, n, 4, 4, 2, n), (p, p + 64, 4, 4, 0, n), (p, p + 64, 4, 4, -1, n), (p, p, 4, 4, 1, n),
                            (p, p + 64, 0, 4, 1, n)],
        "t2h_eval_class_bits": [(n, 0, n, 0, n, 100, n), (n, 0, n, 16, p, 100, n), (n, 2, n, 1, p, 100, n), (n, 0, n, 0, p, 0, n)],
        "t2h_eval_residual": [(n, 1, 4, 4, n, 0, n, 8, 8, 0, 0, n, n, n), (p, 1, 4, 4, p, 0, p, 8, 8, 5, 0, p, p, n),
                              (p, 1, 4, 4, p, 0, p, 8, 8, 0, -1, p, p, n), (p, 1, 4, 9, p, 0, p, 8, 8, 0, 0, p, p, n),
                              (p, 1, 0, 4, p, 0, p, 8, 8, 0, 0, p, p, n)],
        "t2h_eval_stats": [(n, n, 100, 2, n, n, 0, n), (p, p, 100, 17, p, p, 1 << 30, n), (p, p, 100, 0, p, p, 1 << 30, n),
                           (p, p, 0, 2, p, p, 1 << 30, n), (p + 8, p, 100, 2, p, p, 1 << 30, n)],
    }
    launching = [k for k, (res, _a) in evaluator.SIGNATURES.items() if res is evaluator._i]
    assert sorted(cases) == sorted(launching)
    for name, rows in cases.items():
        for args in rows:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert len(lib.t2h_last_error_string()) > 8
    need = lib.t2h_eval_stats_workspace_bytes(100, 2)
    assert need > 0 and lib.t2h_eval_stats_workspace_bytes(100, 17) == 0 and lib.t2h_eval_stats_workspace_bytes(0, 2) == 0
    assert lib.t2h_eval_stats(p, p, 100, 2, p, p, need - 1, n) == -3
    assert b"workspace" in lib.t2h_last_error_string()
    assert lib.t2h_eval_stats_workspace_bytes(1660 * 1990, 16) >= 2 * 8 * 16 * 2 * 2 * 256 * 8


def test_evaluator_has_no_cpu_path():
    import tomosar2height_amd
    from tomosar2height_amd import DSMEvaluator, dilate_mask, evaluator
    assert tomosar2height_amd.DSMEvaluator is evaluator.DSMEvaluator and tomosar2height_amd.dilate_mask is evaluator.dilate_mask
    with pytest.raises(RuntimeError, match="no CPU path"):
        dilate_mask(torch.zeros(4, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        DSMEvaluator(torch.zeros(4, 4), bounds=(0.0, 4.0))
    ev = DSMEvaluator.__new__(DSMEvaluator)
    ev.left, ev.top, ev.pixel_size = 10.0, 788.0, (1.0, 2.0)
    assert ev.window((10.5, 787.5)) == (0, 0) and ev.window((522.49, 276.5)) == (512, 255)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.eval(torch.zeros(4, 4))
