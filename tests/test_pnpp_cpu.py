"""CPU (no GPU needed): the numpy restatement of the PointNet++ point stages (tests/pnpp_ref.py) reproduces the fixture made
from the reference's own modules in float32 and float64 (tests/golden/make_golden_pnpp.py), and the encoder's parameters keep
the reference's names and shapes."""
import numpy as np
import pytest
import torch

import pnpp_ref
from abi_ref import declared_symbols
from conftest import load_golden

UNAMBIGUOUS = ("n700", "n1536b2", "n300")
INDEX_KEYS = ("sa1_fps", "sa2_fps", "sa1_idx", "sa2_idx", "fp2_idx", "fp1_idx")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("pnpp_encoder")
    return _cache["g"]


def restated(name):
    """The restatement of every cloud of a case, computed once and shared."""
    if name not in _cache:
        from tomosar2height_amd import TomoSAR2Height
        g = golden()
        if "enc" not in _cache:
            _cache["enc"] = pnpp_ref.init_pnpp_(TomoSAR2Height(pnpp_ref.model_cfg("alto", g)), seed=41).eval().point_encoder
        pts = g[f"{name}_points"]
        _cache[name] = [pnpp_ref.encoder_points(_cache["enc"], pts[b], g[f"{name}_start1"][b], g[f"{name}_start2"][b])
                        for b in range(pts.shape[0])]
    return _cache[name]


def test_fixture_records_what_the_generator_asserted():
    g = golden()
    assert [str(c) for c in g["cases"]] == ["n700", "n1536b2", "n300", "dup1024", "n700u"]
    for name, n, b in (("n700", 700, 1), ("n1536b2", 1536, 2), ("n300", 300, 1), ("dup1024", 1024, 1), ("n700u", 700, 1)):
        pts = g[f"{name}_points"]
        assert pts.shape == (b, n, 3) and pts.dtype == np.float32
        assert (pts[..., :2] > 0).all() and (pts[..., :2] < 1).all() and (pts[..., 2] >= 0).all() and (pts[..., 2] < 0.6).all()
        assert bool(g[f"{name}_unambiguous"]) == (name != "dup1024")
        assert np.array_equal(g[f"{name}_sa1_fps"][:, 0], g[f"{name}_start1"])
        assert np.array_equal(g[f"{name}_sa2_fps"][:, 0], g[f"{name}_start2"])
        for k in ("l3_points", "l2_points", "l1_points", "l0_points", "plane", "out", "heights"):
            assert 0 < float(g[f"{name}_{k}_dev"]) < 1e-4 * np.abs(g[f"{name}_{k}"]).max()
        for k in ("l1_points", "l0_points", "fp1_w", "fp2_w", "fp1_rows", "fp2_rows"):      # measured off the coincident rows
            assert 0 < float(g[f"{name}_{k}_dev"]) <= float(g[f"{name}_{k}_dev_all"])
    dup = g["dup1024_points"][0]
    assert np.unique(dup, axis=0).shape[0] == 1024 - 64
    assert str(g["n700u_unet_type"]) == "unet" and str(g["n700_unet_type"]) == "alto"


@pytest.mark.parametrize("name", UNAMBIGUOUS)
def test_three_nn_weights_and_rows_with_the_coincident_rows_left_out_of_ref32(name):
    """The restatement's 3-NN weights and interpolated rows from the reference's own source features: within tolerance of ref64
    on all rows, of ref32 on the non-coincident rows.  The excluded rows are exactly those with float64 d2_min < 1e-12: at most
    S per cloud and level, counted here."""
    g = golden()
    pts = g[f"{name}_points"]
    for b in range(pts.shape[0]):
        l1 = pts[b][g[f"{name}_sa1_fps"][b]]
        l2 = l1[g[f"{name}_sa2_fps"][b]]
        for level, targets, sources, feats, s_max in (("fp1", pts[b], l1, g[f"{name}_l1_points"][b], 512),
                                                      ("fp2", l1, l2, g[f"{name}_l2_points"][b], 128)):
            idx, w, _ = pnpp_ref.three_nn(targets, sources)
            mask = pnpp_ref.check_three_nn(g, name, level, b, w, pnpp_ref.interpolate(feats, idx, w))
            assert np.array_equal(mask, pnpp_ref.coincident(targets, sources))
            distinct_sources = np.unique(sources, axis=0).shape[0]
            assert distinct_sources <= int(mask.sum()) and (int(mask.sum()) <= s_max or name == "n300"), (name, level, int(mask.sum()))
        assert int(g[f"{name}_fp1_coincident"][b].sum()) == min(512, pts.shape[1])
        # (n300's l1 repeats point 0 in 212 slots: as targets of fp2 every copy coincides with the source that is point 0)
        assert int(g[f"{name}_fp2_coincident"][b].sum()) == (128 if name != "n300" else int(pnpp_ref.coincident(l1, l2).sum()))


@pytest.mark.parametrize("name", UNAMBIGUOUS)
def test_restatement_reproduces_the_reference_indices(name):
    g = golden()
    for b, r in enumerate(restated(name)):
        for k in INDEX_KEYS:
            got, want = r[k], g[f"{name}_{k}"][b]
            if name == "n300" and k == "fp1_idx":
                # below npoint the centroids repeat point 0 (212 slots): equal distances among its copies, which the reference's
                # sort orders arbitrarily and this library by slot -- compared through the cloud points the slots denote
                got, want = r["sa1_fps"][got], r["sa1_fps"][want]
            assert np.array_equal(got, want), (name, b, k)


@pytest.mark.parametrize("name", UNAMBIGUOUS)
def test_restatement_reproduces_the_reference_features(name):
    """Within 4 x max|ref32 - ref64| of the float64 reference (the restatement's products are numpy's float32 sums)."""
    g = golden()
    for key in ("l3_points", "l2_points", "l1_points", "l0_points"):
        want, tol = pnpp_ref.ref64(g, name, key)
        for b, r in enumerate(restated(name)):
            err = np.abs(r[key].astype(np.float64) - want[b]).max()
            print(f"{name}[{b}] {key}: max err {err:.3g}, tolerance {tol:.3g}")
            assert err <= tol, (name, b, key, err, tol)


def test_tie_rules_on_the_duplicates_cloud():
    """Equal maxima of FPS and equal 3-NN distances go to the lowest index; duplicates inside a ball keep index order."""
    g = golden()
    pts = g["dup1024_points"][0]
    r = restated("dup1024")[0]
    fps = r["sa1_fps"]
    assert len(set(fps.tolist())) == 512                                    # 960 distinct points: no distance reaches 0
    _, inverse = np.unique(pts, axis=0, return_inverse=True)
    first_of = {}
    for i, u in enumerate(inverse.reshape(-1)):
        first_of.setdefault(int(u), i)
    start = int(g["dup1024_start1"][0])
    assert all(first_of[int(inverse.reshape(-1)[i])] == i for i in fps if i != start)      # of two copies FPS takes the first
    l1 = pts[fps]
    idx, w, dd = pnpp_ref.three_nn(pts, l1)
    assert (np.diff(dd, axis=1) >= 0).all()
    ties = dd[:, 0] == dd[:, 1]
    assert (idx[ties, 0] < idx[ties, 1]).all()
    ball = r["sa1_idx"]
    for s in range(0, 512, 37):
        row = ball[s]
        n_in = len(set(row.tolist()))
        assert (np.diff(row[:n_in]) > 0).all() and (row[n_in:] == row[0]).all()


def test_fps_below_npoint_repeats_centroids_as_the_reference():
    g = golden()
    fps = restated("n300")[0]["sa1_fps"]
    assert sorted(set(fps[:300].tolist())) == list(range(300)) and (fps[300:] == 0).all()
    assert np.array_equal(fps, g["n300_sa1_fps"][0])


def test_state_dict_keys_and_shapes_are_the_references():
    from tomosar2height_amd.encoder import encoder_dict
    g = golden()
    enc = encoder_dict["pointnet_plus_plus"](**pnpp_ref.model_cfg("alto", g).model.encoder_kwargs, dim=3)
    sd = enc.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_keys"]]
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g["state_shapes"]]
    assert "sa1.mlp_bns.0.num_batches_tracked" in sd and tuple(sd["sa1.mlp_convs.0.weight"].shape) == (64, 6, 1, 1)
    with pytest.raises(NotImplementedError, match="BatchNorm batch statistics"):
        enc.train()(torch.zeros(1, 8, 3))
    with pytest.raises(RuntimeError, match="cuda device"):
        enc.eval()(torch.zeros(1, 8, 3))


def test_header_declares_exactly_the_typed_entry_points():
    from tomosar2height_amd import _lib, pointops
    from tomosar2height_amd.csrc import build
    header = [h for h in build.PUBLIC_HEADERS if h.endswith("t2h_pnpp.h")][0]
    assert sorted(pointops.SIGNATURES) == declared_symbols(header)
    assert not set(pointops.SIGNATURES) & set(_lib.SIGNATURES)
    assert any(h.endswith("t2h_pnpp.h") for h in build.PUBLIC_HEADERS)
    assert pointops.FPS_ONE_WG_MAX == 2048 and "#define T2H_FPS_ONE_WG_MAX 2048" in open(
        [h for h in build.PUBLIC_HEADERS if h.endswith("t2h_pnpp.h")][0]).read()
