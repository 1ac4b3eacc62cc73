"""CPU (no GPU needed): the numpy restatement of the interpolation baselines (tests/interp_ref.py) reproduces the fixture made
from the reference's own scripts/interpolate_nearest.py and scripts/interpolate_idw.py, and the boundary of
include/t2h_interp.h holds without a device."""
import numpy as np
import pytest
import torch

import interp_ref
from conftest import load_golden
from abi_ref import declared_symbols

CASES = ("main", "coarse", "sparse")
# largest share of pixels whose k-th and (k + 1)-th neighbours tie (the k-d tree may return either: left out of the
# comparison with the reference's rasters), as conditions
TIE_SHARE = {"main": 0.01, "coarse": 0.50, "sparse": 0.01}
SHAPES = {"main": (46, 71), "coarse": (46, 71), "sparse": (20, 30)}


def fixture_case(name):
    g = load_golden("interp_baselines")
    pts = g[f"{name}_points"]
    return {"points": pts, "unique": pts[g[f"{name}_keep"]], "nearest": g[f"{name}_nearest"], "idw": g[f"{name}_idw"],
            "origin": g[f"{name}_origin"], "dist": g[f"{name}_dist"]}


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    """Nearest: byte-equal on every pixel without a rank-k tie.  IDW: within 32 * 2^-53 * max|z| there (five roundings per
    term, seven additions of terms that sum to at most max|z|, doubled for the reference's pairwise sum).  Measured when the
    fixture was written: 3.44 (main), 4.84 (coarse), 3.54 (sparse) of those units; pixels left out: main 0 % / 0 %, coarse
    9.80 % at k = 1 and 15.74 % at k = 8, sparse 0 % / 0 %."""
    c = fixture_case(name)
    assert sorted(str(n) for n in load_golden("interp_baselines")["cases"]) == sorted(CASES)
    unique = interp_ref.unique_cloud(c["points"])
    assert unique.tobytes() == np.ascontiguousarray(c["unique"]).tobytes()          # the group-by result, in its X, Y order
    assert len(unique) < len(c["points"]) or name == "sparse"
    xs, ys, origin = interp_ref.grid(unique)
    assert (len(ys), len(xs)) == c["nearest"].shape == c["idw"].shape == SHAPES[name]
    assert tuple(c["origin"]) == origin and origin[0] > 2 ** 18 and np.float32(origin[1] + 0.01) != origin[1] + 0.01
    near, tie1 = interp_ref.nearest(unique)
    idw, tie8 = interp_ref.idw(unique)
    assert tie1.mean() <= TIE_SHARE[name] and tie8.mean() <= TIE_SHARE[name], (tie1.mean(), tie8.mean())
    assert near[~tie1].tobytes() == c["nearest"][~tie1].tobytes()
    bound = interp_ref.idw_bound(unique[:, 2])
    gap = np.abs(idw - c["idw"])[~tie8].max()
    print(name, "IDW gap", gap / (bound / 32), "x 2^-53 max|z|; left out", tie1.mean(), tie8.mean())
    assert gap <= bound, (gap, bound)
    d2, idx, _ = interp_ref.knn(unique, 1.0, 8)
    assert np.array_equal(np.sqrt(d2), c["dist"])                # the k-d tree's distances are sqrt(dx * dx + dy * dy)
    assert (d2[..., 0] == 0).sum() >= (100 if name == "coarse" else 1)              # the zero-distance branch is taken
    if name == "coarse":
        assert tie1.mean() > 0.05 and tie8.mean() > 0.05         # the case that pins the tie rule


def test_restatement_tie_rule_and_fixed_order():
    """Four points at the same distance of the node (0, 0) of a 2 x 2 grid: (d2, X, Y) picks them in X, then Y order."""
    u = np.array([[-1.0, -1.0, 7.0], [-1.0, 1.0, 1.0], [1.0, -1.0, 2.0], [1.0, 1.0, 3.0], [-1.0, 0.999, 5.0]])
    u = interp_ref.unique_cloud(u)
    assert u[:, 2].tolist() == [7.0, 5.0, 1.0, 2.0, 3.0]
    d2, idx, tie = interp_ref.knn(u + [1.0, 1.0, 0.0], 1.0, 2)   # origin (0, 0); node (1, 1) is the centre
    assert idx[1, 1].tolist() == [1, 0] and abs(d2[1, 1, 0] - (1.0 + 0.999 ** 2)) < 1e-12 and d2[1, 1, 1] == 2.0 and tie[1, 1]
    out, _ = interp_ref.idw(interp_ref.unique_cloud(np.array([[0.0, 0.0, 4.0], [2.0, 0.0, 8.0], [0.0, 2.0, 6.0]])), 1.0, 2)
    # node (0, 0) coincides with a point: weight 1 beside 1 / 4, not the point's z alone; (0, 2) comes before (2, 0)
    assert out.shape == (2, 2) and out[0, 0] == (1.0 / 1.25) * 4.0 + (0.25 / 1.25) * 6.0


def test_interp_header_matches_signatures_and_library():
    from tomosar2height_amd import _lib, evaluator, instances, interpolate
    from tomosar2height_amd.csrc import build
    declared = declared_symbols("t2h_interp.h")
    assert declared == sorted(interpolate.SIGNATURES) and len(declared) == 8
    assert all(name.startswith("t2h_interp_") for name in declared)
    lib = interpolate.load()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (interpolate.SIGNATURES[name][0], interpolate.SIGNATURES[name][1]), name
    for header in ("t2h.h", "t2h_eval.h", "t2h_inst.h"):
        assert not any("t2h_interp" in name for name in declared_symbols(header))
    others = list(_lib.SIGNATURES) + list(evaluator.SIGNATURES) + list(instances.SIGNATURES)
    assert not any("t2h_interp" in name for name in others)
    assert _lib.ABI_VERSION == 20 == lib.t2h_abi_version()
    assert any(h.endswith("t2h_interp.h") for h in build.PUBLIC_HEADERS)
    text = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "t2h_interp.h")).read()
    for name, value in (("TILE", interpolate.TILE), ("CHUNK", interpolate.CHUNK), ("MAX_K", interpolate.MAX_K),
                        ("CELL_POINTS", interpolate.CELL_POINTS), ("TABLE_COLS", interpolate.TABLE_COLS)):
        assert f"#define T2H_INTERP_{name} {value} " in text, name
    assert interpolate.CHUNK * 20 <= 64 * 1024                    # the LDS a workgroup gets without opting in


def test_interp_entries_reject_bad_arguments_without_a_gpu():
    from tomosar2height_amd import interpolate
    lib = interpolate.load()
    n = None
    buf = np.zeros(1 << 16, np.float64)                   # host memory: valid-looking, aligned, never launched on
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    big = 1 << 40
    grid = lambda **kw: tuple({**dict(u=p, off=p, M=50, xmin=1.0, ymin=2.0, h=1.5, gx=4, gy=5, res=1.0, ny=7, nx=9), **kw}.values())
    bad_grids = [grid(u=n), grid(off=n), grid(u=p + 4), grid(off=p + 2), grid(M=0), grid(xmin=float("nan")), grid(ymin=float("inf")),
                 grid(h=0.0), grid(h=float("inf")), grid(gx=0), grid(gy=-1), grid(gx=1 << 16, gy=1 << 16), grid(res=0.0),
                 grid(res=-1.0), grid(res=float("nan")), grid(ny=0), grid(nx=0), grid(ny=1 << 16, nx=1 << 16)]
    cases = {
        # (points, N, table, ws, ws_bytes, stream)
        "t2h_interp_bounds": [(n, 9, p, p, big, n), (p, 9, n, p, big, n), (p, 9, p, n, big, n), (p, 0, p, p, big, n),
                              (p, 1 << 31, p, p, big, n), (p + 4, 9, p, p, big, n)],
        # (points, N, table, unique, cell_offsets, ws, ws_bytes, stream)
        "t2h_interp_index": [(n, 9, p, p, p, p, big, n), (p, 9, n, p, p, p, big, n), (p, 9, p, n, p, p, big, n),
                             (p, 9, p, p, n, p, big, n), (p, 9, p, p, p, n, big, n), (p, 0, p, p, p, p, big, n),
                             (p, 1 << 31, p, p, p, p, big, n), (p, 9, p, p + 4, p, p, big, n), (p, 9, p, p, p + 2, p, big, n)],
        # (grid..., k, d2, idx, stream)
        "t2h_interp_knn": [g + (8, p, p, n) for g in bad_grids] + [grid() + (8, n, p, n), grid() + (8, p, n, n),
                                                                     grid() + (0, p, p, n), grid() + (9, p, p, n),
                                                                     grid(M=5) + (6, p, p, n), grid() + (8, p, p + 2, n)],
        # (grid..., out, stream)
        "t2h_interp_nearest": [g + (p, n) for g in bad_grids] + [grid() + (n, n), grid() + (p + 4, n)],
        # (grid..., k, out, stream)
        "t2h_interp_idw": [g + (8, p, n) for g in bad_grids] + [grid() + (8, n, n), grid() + (0, p, n), grid() + (9, p, n),
                                                                  grid(M=7) + (8, p, n)],
    }
    launching = [k for k, (res, _a) in interpolate.SIGNATURES.items() if res is interpolate._i]
    assert sorted(cases) == sorted(launching)
    for name, rows in cases.items():
        for args in rows:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert len(lib.t2h_last_error_string()) > 8
    for query in ("t2h_interp_max_cells", "t2h_interp_bounds_workspace_bytes", "t2h_interp_index_workspace_bytes"):
        assert getattr(lib, query)(0) == 0 and getattr(lib, query)(-3) == 0 and getattr(lib, query)(1 << 31) == 0, query
        assert getattr(lib, query)(1) > 0
    assert lib.t2h_interp_max_cells(3221) == 3221 // 2 + 8
    need = lib.t2h_interp_bounds_workspace_bytes(3221)
    assert need == 40 * 1024 and lib.t2h_interp_bounds(p, 3221, p, p, need - 1, n) == -3
    assert b"workspace" in lib.t2h_last_error_string()
    need = lib.t2h_interp_index_workspace_bytes(3221)
    assert need >= 52 * 3221 and lib.t2h_interp_index(p, 3221, p, p, p, p, need - 1, n) == -3
    assert b"workspace" in lib.t2h_last_error_string()
    # linear in the points: the documented constants bound a five-million-point cloud's workspace
    N = 5_000_000
    assert lib.t2h_interp_index_workspace_bytes(N) <= 52 * N + 4 * (N // 2 + 9) + 4 * (N // 1024 + 2) + 6 * 256


def test_interpolation_has_no_cpu_path_and_refuses_bad_requests():
    import tomosar2height_amd
    from tomosar2height_amd import CloudIndex, grid_knn, idw_dsm, interpolate, linear_dsm, nearest_dsm
    assert tomosar2height_amd.CloudIndex is interpolate.CloudIndex and tomosar2height_amd.idw_dsm is interpolate.idw_dsm
    host = torch.zeros(12, 3, dtype=torch.float64)
    for fn in (CloudIndex, nearest_dsm, idw_dsm):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(host)
    with pytest.raises(TypeError, match="float64"):
        CloudIndex(torch.zeros(12, 3, dtype=torch.int32))
    with pytest.raises(TypeError, match="float64"):
        CloudIndex(torch.zeros(12, 3, dtype=torch.float16))
    with pytest.raises(TypeError, match="torch tensor"):
        CloudIndex(np.zeros((12, 3)))
    for shape in ((12, 2), (12,), (0, 3), (2, 12, 3)):
        with pytest.raises(ValueError, match=r"\[N, 3\]"):
            CloudIndex(torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError, match="power"):
        idw_dsm(host, power=3)                                    # refused before the cloud is looked at
    with pytest.raises(TypeError, match="CloudIndex"):
        grid_knn(host)
    with pytest.raises(NotImplementedError, match=r"interpolate_bilinear\.py.*DESIGN\.md section 7"):
        linear_dsm(host)
    ix = CloudIndex.__new__(CloudIndex)                           # the host-side arithmetic of an index, without a device
    ix.bounds, ix.n_unique = (392000.0, 392070.3, 5820000.0, 5820045.7), 5
    assert ix.grid_shape() == (46, 71) and ix.grid_shape(0.5) == (92, 141) and ix.grid_shape(2.0) == (23, 36)
    ix.bounds = (1.0, 4.0, 2.0, 2.0)
    assert ix.grid_shape() == (0, 3)                              # ymin == ymax: an empty raster
    for res in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="resolution"):
            ix.grid_shape(res)
    for k in (0, 9, 2.5):
        with pytest.raises(ValueError, match="k = "):
            interpolate._check_k(ix, k, "idw_dsm")
    with pytest.raises(ValueError, match="5 distinct"):
        interpolate._check_k(ix, 6, "idw_dsm")
