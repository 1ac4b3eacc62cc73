"""CPU (no GPU needed): the numpy restatement of the Delaunay-linear baseline (tests/tin_ref.py) reproduces the fixture made
with scipy's griddata / Delaunay.find_simplex on shifted coordinates (tests/golden/make_golden_tin.py), and the boundary of
include/t2h_tin.h holds without a device."""
import numpy as np
import pytest
import torch

import tin_ref
from conftest import load_golden
from abi_ref import declared_symbols

CASES = ("tiny", "mid", "fine", "clustered", "strip", "on_node")
SHAPES = {"tiny": (10, 12), "mid": (40, 48), "fine": (80, 96), "clustered": (64, 64), "strip": (6, 80), "on_node": (40, 48)}
EXCLUSION_CAP = 0.005       # ambiguous nodes (finite in the reference, smallest |lambda| below 2^-30) a test may leave out


def fixture_case(name):
    g = load_golden("tin_baseline")
    c = {k: g[f"{name}_{k}"] for k in ("points", "dsm", "tri", "ambiguous")}
    c["resolution"] = float(g[f"{name}_resolution"])
    c["unique"] = tin_ref.unique_cloud(c["points"])
    c["units_bound"] = float(g["units_bound"])
    finite = ~np.isnan(c["dsm"])
    assert c["ambiguous"].sum() <= EXCLUSION_CAP * finite.sum() and not (c["ambiguous"] & ~finite).any()
    return c


def test_fixture_records_what_the_generator_asserted():
    g = load_golden("tin_baseline")
    assert [str(n) for n in g["cases"]] == list(CASES)
    assert float(g["units_bound"]) == 16.0                        # next power of two at or above 4 x 2.34 units measured
    for name in CASES:
        assert int(g[f"{name}_coplanar"]) == 0 and bool(g[f"{name}_general_position"])
        assert float(g[f"{name}_ambiguous_share"]) <= EXCLUSION_CAP
        assert int(g[f"{name}_coplanar_raw"]) > 0                 # what Qhull drops on the raw UTM coordinates
        assert g[f"{name}_dsm"].shape == SHAPES[name] and float(g[f"{name}_units"]) * 4 <= 16.0
        nan = np.isnan(g[f"{name}_dsm"]).mean()
        assert 0.015 < nan < 0.25, (name, nan)
        d = g[f"{name}_points"][:, :2] - (389000.0, 5819000.0)
        assert (d >= 0).all() and (d < 256).all() and np.array_equal(d * 65536, np.round(d * 65536))
    assert int(g["on_node_ambiguous"].sum()) == 3 and sum(int(g[f"{n}_ambiguous"].sum()) for n in CASES) == 3


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    """The restatement evaluated on find_simplex's triangles: NaN mask equal, raster within ``units_bound`` units of 2^-52 *
    max|z| of the node's three vertices of griddata's (measured by the generator: tiny 0.86, mid 1.52, fine 2.03, clustered
    2.34, strip 1.67, on_node 1.60), barycentric coordinates inside [0, 1] up to rounding and summing to 1."""
    c = fixture_case(name)
    u, tri, res = c["unique"], c["tri"], c["resolution"]
    assert len(u) < len(c["points"])                              # duplicated (X, Y) carry other heights
    qx, qy = tin_ref.nodes(u, res)
    assert (len(qy), len(qx)) == c["dsm"].shape == SHAPES[name]
    lam = tin_ref.barycentric(u, tri, res)
    dsm = tin_ref.linear(u, tri, res)
    assert np.array_equal(np.isnan(dsm), np.isnan(c["dsm"])) and np.array_equal(np.isnan(dsm), tri[..., 0] < 0)
    ok = ~np.isnan(dsm)
    assert lam[ok].min() > -2.0 ** -30 and np.abs(lam[ok].sum(-1) - 1).max() < 2.0 ** -40
    gap = tin_ref.units(dsm, c["dsm"], u, tri)[ok & ~c["ambiguous"]].max()
    print(name, "restatement vs griddata:", gap, "units; bound", c["units_bound"])
    assert gap <= c["units_bound"]
    assert (tri[ok][:, 0] < tri[ok][:, 1]).all() and (tri[ok][:, 1] < tri[ok][:, 2]).all()


def test_brute_force_agrees_with_the_fixture_on_the_small_case():
    c = fixture_case("tiny")
    tri, count = tin_ref.brute_force(c["unique"], c["resolution"])
    inside = c["tri"][..., 0] >= 0
    assert np.array_equal(tri, c["tri"]) and not c["ambiguous"].any()
    assert (count[inside] == 1).all() and (count[~inside] == 0).all()
    assert tin_ref.linear(c["unique"], tri).tobytes() == tin_ref.linear(c["unique"], c["tri"]).tobytes()


def test_brute_force_and_barycentric_on_a_known_square():
    """Four points, one diagonal: (0, 0), (2, 0), (0, 2), (2.5, 2.5); node (1, 1) lies on the edge (2, 0)-(0, 2) of both
    triangles, node (0, 0) on a point."""
    u = np.array([[0.0, 0.0, 1.0], [0.0, 2.0, 3.0], [2.0, 0.0, 5.0], [2.5, 2.5, 9.0]]) + [10.0, 20.0, 0.0]
    tri, count = tin_ref.brute_force(u)
    assert tri.shape == (3, 3, 3) and count[1, 1] == 2 and count[0, 0] == 1 and tri[0, 0].tolist() == [0, 1, 2]
    dsm = tin_ref.linear(u, tri)
    assert dsm[0, 0] == 1.0 and dsm[1, 1] == 4.0 and dsm[0, 1] == 3.0 and abs(dsm[2, 2] - (4.0 + 10.0 / 3.0)) < 1e-12
    lam = tin_ref.barycentric(u, tri)
    assert lam[0, 0].tolist() == [1.0, 0.0, 0.0] and lam[1, 1, 0] == 0.0
    sets = tin_ref.vertex_sets(u, tri)
    assert sets[0, 0].tolist() == [[10.0, 20.0], [10.0, 22.0], [12.0, 20.0]]


def test_tin_header_matches_signatures_and_library():
    from tomosar2height_amd import _lib, cloud_instances, evaluator, instances, interpolate
    from tomosar2height_amd.csrc import build
    declared = declared_symbols("t2h_tin.h")
    assert declared == sorted(interpolate.TIN_SIGNATURES) and len(declared) == 4
    assert all(name.startswith("t2h_tin_") for name in declared)
    lib = interpolate.load()
    for name in declared:
        fn = getattr(lib, name)
        sig = interpolate.TIN_SIGNATURES[name]
        assert (fn.restype, list(fn.argtypes)) == (sig[0], sig[1]), name
    for header in ("t2h.h", "t2h_eval.h", "t2h_inst.h", "t2h_interp.h", "t2h_cloud.h"):
        assert not any("t2h_tin" in name for name in declared_symbols(header))
    others = (list(_lib.SIGNATURES) + list(evaluator.SIGNATURES) + list(instances.SIGNATURES) + list(interpolate.SIGNATURES) +
              list(cloud_instances.SIGNATURES))
    assert not any("t2h_tin" in name for name in others)
    assert _lib.ABI_VERSION == 20 == lib.t2h_abi_version()
    assert any(h.endswith("t2h_tin.h") for h in build.PUBLIC_HEADERS)
    assert any(s.endswith("dsm_tin.hip") for s in build.sources())
    text = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "t2h_tin.h")).read()
    for name, value in (("DIRECTIONS", interpolate.TIN_DIRECTIONS), ("MAX_PIVOTS", interpolate.TIN_MAX_PIVOTS),
                        ("STATUS_COLS", interpolate.TIN_STATUS_COLS)):
        assert f"#define T2H_TIN_{name} {value} " in text, name
    assert interpolate.TIN_MAX_PIVOTS == 64


def test_tin_entries_reject_bad_arguments_without_a_gpu():
    from tomosar2height_amd import interpolate
    lib = interpolate.load()
    n = None
    buf = np.zeros(1 << 16, np.float64)                   # host memory: valid-looking, aligned, never launched on
    p = buf.ctypes.data + (-buf.ctypes.data % 16)
    big, nan, inf = 1 << 40, float("nan"), float("inf")
    grid = lambda **kw: tuple({**dict(u=p, off=p, M=50, xmin=1.0, ymin=2.0, h=1.5, gx=4, gy=5, res=1.0, ny=7, nx=9), **kw}.values())
    bad_grids = [grid(u=n), grid(off=n), grid(u=p + 4), grid(off=p + 2), grid(M=2), grid(xmin=nan), grid(ymin=inf), grid(h=0.0),
                 grid(h=inf), grid(gx=0), grid(gy=-1), grid(gx=1 << 16, gy=1 << 16), grid(res=0.0), grid(res=-1.0), grid(res=nan),
                 grid(ny=0), grid(nx=0), grid(ny=1 << 16, nx=1 << 16)]
    cases = {
        # (unique, M, xmin, ymin, hull, status, ws, ws_bytes, stream)
        "t2h_tin_hull": [(n, 9, 1.0, 2.0, p, p, p, big, n), (p, 9, 1.0, 2.0, n, p, p, big, n), (p, 9, 1.0, 2.0, p, n, p, big, n),
                         (p, 9, 1.0, 2.0, p, p, n, big, n), (p, 0, 1.0, 2.0, p, p, p, big, n), (p, (1 << 30) + 1, 1.0, 2.0, p, p, p, big, n),
                         (p + 4, 9, 1.0, 2.0, p, p, p, big, n), (p, 9, 1.0, 2.0, p + 2, p, p, big, n), (p, 9, nan, 2.0, p, p, p, big, n),
                         (p, 9, 1.0, inf, p, p, p, big, n)],
        # (grid..., hull, n_hull, tri, bary, status, stream)
        "t2h_tin_simplex": [g + (p, 5, p, p, p, n) for g in bad_grids] + [grid() + (n, 5, p, p, p, n), grid() + (p, 5, n, p, p, n),
                                                                          grid() + (p, 5, p, n, p, n), grid() + (p, 5, p, p, n, n),
                                                                          grid() + (p, 2, p, p, p, n), grid() + (p, 51, p, p, p, n),
                                                                          grid() + (p, 5, p + 2, p, p, n), grid() + (p, 5, p, p + 4, p, n)],
        # (grid..., hull, n_hull, out, status, stream)
        "t2h_tin_linear": [g + (p, 5, p, p, n) for g in bad_grids] + [grid() + (n, 5, p, p, n), grid() + (p, 5, n, p, n),
                                                                      grid() + (p, 5, p, n, n), grid() + (p, 2, p, p, n),
                                                                      grid() + (p, 5, p + 4, p, n), grid() + (p + 2, 5, p, p, n)],
    }
    launching = [k for k, (res, _a) in interpolate.TIN_SIGNATURES.items() if res is interpolate._i]
    assert sorted(cases) == sorted(launching)
    for name, rows in cases.items():
        for args in rows:
            assert getattr(lib, name)(*args) == -1, (name, args)
            assert len(lib.t2h_last_error_string()) > 8
    q = lib.t2h_tin_hull_workspace_bytes
    assert q(0) == 0 and q(-3) == 0 and q((1 << 30) + 1) == 0 and q(1) > 0
    need = q(3221)
    assert need >= 4 * 4096 and lib.t2h_tin_hull(p, 3221, 1.0, 2.0, p, p, p, need - 1, n) == -3
    assert b"workspace" in lib.t2h_last_error_string()
    M = 3_200_000                                                 # the documented constants bound a Berlin chunk's workspace
    assert q(M) <= 8 * M + (8 + 4) * 256 * 16 + 512 + 5 * 256


def test_delaunay_baseline_has_no_cpu_path_and_linear_dsm_still_raises():
    import tomosar2height_amd
    from tomosar2height_amd import delaunay_dsm, grid_simplex, interpolate, linear_dsm
    assert tomosar2height_amd.delaunay_dsm is interpolate.delaunay_dsm and tomosar2height_amd.grid_simplex is interpolate.grid_simplex
    assert "delaunay_dsm" in tomosar2height_amd.__all__ and "grid_simplex" in tomosar2height_amd.__all__
    host = torch.zeros(12, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        delaunay_dsm(host)
    with pytest.raises(RuntimeError, match="no CPU path"):
        delaunay_dsm(host, 0.5, return_status=True)
    with pytest.raises(TypeError, match="CloudIndex"):
        grid_simplex(host)
    with pytest.raises(TypeError, match="torch tensor"):
        delaunay_dsm(np.zeros((12, 3)))
    with pytest.raises(TypeError, match="float64"):
        delaunay_dsm(torch.zeros(12, 3, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match=r"interpolate_bilinear\.py.*delaunay_dsm.*DESIGN\.md section 7"):
        linear_dsm(host)
