"""CPU (no GPU needed): the C ABI of the PointNet++ adjoints (include/t2h_pnpp.h: t2h_group_max_bwd, t2h_index_transpose,
t2h_rows_gather_bwd) is declared, typed and validated before any launch, and their numpy restatement (tests/pnpp_grad_ref.py)
is consistent with itself: the transpose is the stable argsort, the float32 sums stay within the summation bound of float64."""
import os
import re

import numpy as np
import pytest

import pnpp_grad_ref as ref
import pnpp_ref
from abi_ref import declared_symbols
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t2h_group_max_bwd", "t2h_index_transpose", "t2h_rows_gather_bwd")
ERR_ARG = -1
P = 0x1000          # a non-null pointer value: every call below is refused before anything is dereferenced or launched


def test_header_signatures_and_symbols_agree_for_the_new_entries():
    from tomosar2height_amd import pointops
    declared = declared_symbols("t2h_pnpp.h")
    assert sorted(pointops.SIGNATURES) == declared and set(NEW) <= set(declared)
    header = open(os.path.join(ROOT, "include", "t2h_pnpp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:                                                  # one argument type per declared parameter
        params = re.search(name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        assert len(params) == len(pointops.SIGNATURES[name][1]), name
    assert ref.CHUNK == int(re.search(r"#define T2H_GATHER_CHUNK (\d+)", header).group(1))
    assert ref.LANES == int(re.search(r"#define T2H_GATHER_LANES (\d+)", header).group(1))
    assert "#define T2H_ABI_VERSION" not in header


def test_no_size_query_was_added():
    source = open(os.path.join(ROOT, "tomosar2height_amd", "csrc", "pnpp.hip")).read()
    assert re.findall(r"^T2H_API\s+size_t\s+(\w+)\s*\(", source, flags=re.M) == ["t2h_fps_workspace_bytes"]
    assert "atomicAdd(float" not in source.replace(" ", "") and "unsafeAtomicAdd" not in source


def entry(name):
    import tomosar2height_amd  # noqa: F401
    from tomosar2height_amd import _lib, pointops  # noqa: F401
    return _lib._entry(name)


def refused(name, *args):
    from tomosar2height_amd import _lib
    rc = entry(name)(*args)
    return rc == ERR_ARG and len(_lib.load().t2h_last_error_string()) > 0


def test_group_max_bwd_validates_before_launching():
    good = [P, 36, 5, 3, 33, P, P, 1, P, 36, None]                   # rows, ld, groups, nsample, C, out, gout, relu, grows, gld, stream
    for pos in (0, 5, 6, 8):
        assert refused("t2h_group_max_bwd", *[None if i == pos else a for i, a in enumerate(good)])
    for pos, bad in ((2, 0), (2, -1), (3, 0), (4, 0), (1, 32), (9, 32), (9, 0)):           # ld < C, gld < C
        assert refused("t2h_group_max_bwd", *[bad if i == pos else a for i, a in enumerate(good)])


def test_index_transpose_validates_before_launching():
    good = [P, 2, 35, 70, P, P, P, None]                             # idx, B, E, N, offsets, entries, cursor, stream
    for pos in (0, 4, 5, 6):
        assert refused("t2h_index_transpose", *[None if i == pos else a for i, a in enumerate(good)])
    for pos, bad in ((1, 0), (1, -2), (2, 0), (2, -5), (3, 0), (3, -1)):
        assert refused("t2h_index_transpose", *[bad if i == pos else a for i, a in enumerate(good)])


def test_rows_gather_bwd_validates_before_launching():
    good = [P, 36, 3, 5, None, 1, P, P, 2, 35, 70, P, None]          # g, gld, col0, D, weight, fan, offsets, entries, B, E, N, out, stream
    for pos in (0, 6, 7, 11):
        assert refused("t2h_rows_gather_bwd", *[None if i == pos else a for i, a in enumerate(good)])
    for pos, bad in ((5, 0), (5, 2), (5, 4), (5, -1), (3, 0), (3, -1), (1, 7), (2, -1), (8, 0), (9, 0), (10, 0), (10, -3)):
        assert refused("t2h_rows_gather_bwd", *[bad if i == pos else a for i, a in enumerate(good)])
    assert refused("t2h_rows_gather_bwd", *[3 if i == 5 else a for i, a in enumerate(good)])        # E = 35 is no multiple of fan = 3


@pytest.mark.parametrize("case", range(3))
def test_restated_transpose_is_the_stable_argsort(case):
    idx, n = ref.index_cases()[case]
    offsets, entries = ref.index_transpose(idx, n)
    flat = np.where((idx.reshape(-1) < 0) | (idx.reshape(-1) >= n), n - 1, idx.reshape(-1))
    assert np.array_equal(entries, np.argsort(flat, kind="stable").astype(np.int32))
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n))]).astype(np.int32))
    assert offsets.dtype == np.int32 and entries.dtype == np.int32
    if n == 70:
        assert offsets[14] == offsets[13] and (np.diff(offsets) > ref.CHUNK).any() == (idx.size > 35)


@pytest.mark.parametrize("fan,d", ((1, 1), (1, 5), (1, 128), (3, 5), (3, 128)))
def test_float32_restatement_within_the_summation_bound_of_float64(fan, d):
    rng = np.random.default_rng(100 * fan + d)
    if fan == 1:
        idx, n = ref.index_cases()[1]
        weight, col0 = None, 3
    else:
        targets, sources = rng.random((130, 3)).astype(np.float32), rng.random((3, 3)).astype(np.float32)
        idx, weight, _ = pnpp_ref.three_nn(targets, sources)
        n, col0 = 3, 0
    g = rng.standard_normal((idx.size // fan, col0 + d + 2)).astype(np.float32)
    offsets, entries = ref.index_transpose(idx, n)
    got = ref.rows_gather_bwd(g, col0, d, weight, fan, offsets, entries, n)
    want, bound = ref.rows_gather_bwd64(g, col0, d, weight, fan, offsets, entries, n)
    assert got.dtype == np.float32 and got.shape == (n, d)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    assert (bound[np.diff(offsets) > 1] > 0).all()


def test_restated_group_max_adjoint_on_ties_zeros_and_negative_maxima():
    rows = np.array([[1, 0, -2, 5], [3, 0, -1, 5], [3, 0, -3, 4]], np.float32)            # one group of three rows
    out = rows.max(0, keepdims=True)
    gout = np.array([[10, 20, 30, 40]], np.float32)
    plain = ref.group_max_bwd(rows, 3, out, gout, relu=False, gld=6)
    assert plain.tolist() == [[0, 20, 0, 40, 0, 0], [10, 0, 30, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    masked = ref.group_max_bwd(rows, 3, out, gout, relu=True, gld=6)
    assert masked.tolist() == [[0, 0, 0, 40, 0, 0], [10, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]]
    assert not np.signbit(masked).any()


def test_fixture_records_what_the_generator_asserted():
    g = load_golden("pnpp_grad")
    assert [str(c) for c in g["cases"]] == ["n700", "n700u", "n1536b2"] and int(g["max_stored"]) == 8192
    names = [str(n) for n in g["param_names"]]
    assert len(names) == 64 and {n.split(".")[0] for n in names} == {"sa1", "sa2", "sa3", "fp3", "fp2", "fp1"}
    assert not any("running" in n or "num_batches" in n for n in names)
    for case in ("n700", "n700u", "n1536b2"):
        for name, numel in zip(names, g["param_numel"]):
            a = g[f"{case}/{name}"]
            stride = -(-int(numel) // 8192)
            assert a.dtype == np.float32 and a.size == -(-int(numel) // stride) and np.any(a != 0)
            assert float(g[f"{case}/{name}_dev"]) > 0 and g[f"{case}/{name}_q"].dtype == np.float16
            assert np.abs(g[f"{case}/{name}_q"].astype(np.float64)).max() <= 1.0
        assert len(g[f"{case}/unet_with_grad"]) > 0
