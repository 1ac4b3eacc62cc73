"""CPU (no GPU needed): the BatchNorm batch-statistics entries of include/t2h_pnpp.h and their typing, the opt-in switch of the
PointNet++ encoder, and the numpy restatement tests/pnpp_bn_ref.py against float64 ``torch.nn.functional.batch_norm``."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

import pnpp_bn_ref as ref
from abi_ref import declared_symbols

BN_ENTRIES = ("t2h_bn_col_stats", "t2h_bn_apply_relu", "t2h_bn_running_update", "t2h_bn_bwd_reduce", "t2h_bn_bwd_apply")


def header_text():
    from tomosar2height_amd.csrc import build
    return open([h for h in build.PUBLIC_HEADERS if h.endswith("t2h_pnpp.h")][0]).read()


def test_header_declares_the_batchnorm_entries_with_the_typed_arguments():
    from tomosar2height_amd import pointops
    from tomosar2height_amd.csrc import build
    header = [h for h in build.PUBLIC_HEADERS if h.endswith("t2h_pnpp.h")][0]
    assert set(BN_ENTRIES) <= set(declared_symbols(header)) and set(BN_ENTRIES) <= set(pointops.SIGNATURES)
    text = re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "t2h_stream_t": ctypes.c_void_p}
    for name in BN_ENTRIES:
        args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        want = [ctypes.c_void_p if "*" in a else ctype[a.split()[-2]] for a in args]
        assert pointops.SIGNATURES[name] == (ctypes.c_int, want), name
    assert f"#define T2H_BN_SLAB {pointops.BN_SLAB}" in header_text() and ref.SLAB == pointops.BN_SLAB
    assert f"#define T2H_BN_WAVES {ref.WAVES}" in header_text()


def test_switch_defaults_to_off_and_is_a_plain_attribute():
    from tomosar2height_amd.encoder.pointnetpp import PointNetFeaturePropagation, PointNetPlusPlus, PointNetSetAbstraction
    sig = inspect.signature(PointNetPlusPlus.__init__)
    assert sig.parameters["batch_statistics"].default is False and list(sig.parameters)[-1] == "batch_statistics"
    kw = dict(feature_dim=32, plane_resolution=16, unet_type="unet", unet_kwargs={"depth": 2, "start_filts": 8})
    off, on = PointNetPlusPlus(**kw), PointNetPlusPlus(**kw, batch_statistics=True)
    for enc, flag in ((off, False), (on, True)):
        assert enc.batch_statistics is flag
        assert [getattr(enc, s).batch_statistics for s in ("sa1", "sa2", "sa3", "fp3", "fp2", "fp1")] == [flag] * 6
    assert list(off.state_dict()) == list(on.state_dict())
    assert [tuple(v.shape) for v in off.state_dict().values()] == [tuple(v.shape) for v in on.state_dict().values()]
    assert not any("batch_statistics" in k for k, _ in list(on.named_buffers()) + list(on.named_parameters()))
    fp = PointNetFeaturePropagation(in_channel=8, mlp=[8, 8])
    sa = PointNetSetAbstraction(npoint=16, radius=0.4, nsample=8, in_channel=6, mlp=[8, 8], group_all=False)
    assert fp.batch_statistics is False and sa.batch_statistics is False
    fp.batch_statistics = True
    assert fp.batch_statistics is True and "batch_statistics" not in fp.state_dict() and fp.wants_batch_stats()
    assert not fp.eval().wants_batch_stats()


def test_default_encoder_still_raises_under_train_and_says_how_to_switch():
    from tomosar2height_amd.encoder.pointnetpp import PointNetFeaturePropagation, PointNetPlusPlus, PointNetSetAbstraction
    enc = PointNetPlusPlus(feature_dim=32, plane_resolution=16, unet_type="unet", unet_kwargs={"depth": 2, "start_filts": 8})
    with pytest.raises(NotImplementedError, match="BatchNorm batch statistics.*batch_statistics=True"):
        enc.train()(torch.rand(1, 50, 3))
    sa = PointNetSetAbstraction(npoint=16, radius=0.4, nsample=8, in_channel=6, mlp=[8, 8], group_all=False)
    with pytest.raises(NotImplementedError, match="BatchNorm batch statistics.*batch_statistics"):
        sa.train().forward_rows(torch.rand(1, 50, 3), torch.rand(1, 50, 3))
    fp = PointNetFeaturePropagation(in_channel=8, mlp=[8, 8])
    with pytest.raises(NotImplementedError, match="BatchNorm batch statistics.*batch_statistics"):
        fp.train().forward_rows(torch.rand(1, 40, 3), torch.rand(1, 5, 3), None, torch.rand(1, 5, 8))


def test_one_value_per_channel_raises_torchs_message():
    from tomosar2height_amd import pointops
    with pytest.raises(ValueError) as ours:
        pointops._bn_rows_count(1, 8)
    with pytest.raises(ValueError) as torchs:
        torch.nn.functional.batch_norm(torch.zeros(1, 8), None, None, training=True)
    assert str(ours.value) == str(torchs.value)


@pytest.mark.parametrize("m,c", ((2, 4), (65, 5), (255, 3), (256, 4), (257, 4), (785, 7)))
def test_restatement_agrees_with_float64_torch_batch_norm(m, c):
    rng = np.random.default_rng(m * 31 + c)
    z = (rng.standard_normal((m, c + 3)) * rng.uniform(0.5, 3, c + 3) + rng.uniform(-2, 2, c + 3)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
    gy = rng.standard_normal((m, c)).astype(np.float32)
    eps, mom = 1e-5, 0.1
    # float64 torch, forward and backward
    zt = torch.tensor(z[:, :c], dtype=torch.float64, requires_grad=True)
    gt, bt = torch.tensor(gamma, dtype=torch.float64, requires_grad=True), torch.tensor(beta, dtype=torch.float64, requires_grad=True)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    yt = torch.relu(torch.nn.functional.batch_norm(zt, rm, rv, gt, bt, training=True, momentum=mom, eps=eps))
    yt.backward(torch.tensor(gy, dtype=torch.float64))
    # the float64 helpers of the restatement are torch's
    y64, mean64, var64 = ref.batch_norm64(z[:, :c], gamma, beta, eps)
    assert np.allclose(y64, yt.detach().numpy(), rtol=1e-12, atol=1e-12)
    dz64, dg64, db64 = ref.batch_norm_bwd64(gy, z[:, :c], gamma.astype(np.float64), eps, y=y64)
    assert np.allclose(dz64, zt.grad.numpy(), rtol=1e-10, atol=1e-12)
    assert np.allclose(dg64, gt.grad.numpy(), rtol=1e-10, atol=1e-12) and np.allclose(db64, bt.grad.numpy(), rtol=1e-10, atol=1e-12)
    # the float32 restatement: statistics within the any-order bounds, the rest within float32 roundings of float64
    mean, var, rstd = ref.col_stats(z, c, eps)
    assert mean.dtype == var.dtype == rstd.dtype == np.float32
    (m64, mb), (v64, vb) = ref.col_stats64(z, c, mean)
    assert (np.abs(mean - m64) <= mb).all() and (np.abs(var - v64) <= vb).all()
    assert np.allclose(m64, mean64, rtol=1e-12, atol=1e-12) and np.allclose(v64, var64, rtol=1e-5, atol=1e-9)
    y = ref.apply_relu(z, c, mean, rstd, gamma, beta, c + 3)
    assert not y[:, c:].any() and np.allclose(y[:, :c], y64, rtol=1e-4, atol=1e-4)
    nrm, nrv = ref.running_update(mean, var, m, mom, np.zeros(c, np.float32), np.ones(c, np.float32))
    assert np.allclose(nrm, rm.numpy(), rtol=1e-5, atol=1e-6) and np.allclose(nrv, rv.numpy(), rtol=1e-4, atol=1e-6)
    dbeta, dgamma = ref.bwd_reduce(gy, y, z, c, mean, rstd, True)
    scale = np.abs(gy).sum(0)
    assert (np.abs(dbeta - db64) <= 1e-5 * scale).all() and (np.abs(dgamma - dg64) <= 1e-4 * scale * np.abs(z).max()).all()
    dz = ref.bwd_apply(gy, y, z, c, mean, rstd, gamma, dbeta, dgamma, True, c + 1)
    assert not dz[:, c:].any() and np.allclose(dz[:, :c], dz64, rtol=1e-3, atol=1e-4 * np.abs(dz64).max() + 1e-5)
    # relu = 0 leaves the gradient unmasked
    db0, _ = ref.bwd_reduce(gy, None, z, c, mean, rstd, False)
    assert np.allclose(db0, gy.astype(np.float64).sum(0), rtol=0, atol=1e-5 * scale.max())
