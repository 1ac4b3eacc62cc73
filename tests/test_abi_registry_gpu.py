"""GPU: an operator whose first t2h call of the process crosses into another header's entries works without anybody having
loaded that header by hand (the registry of ``_lib.declare``), and the PointNet++ stage's folded layers, now on ``_lib.Derived``,
are the float64 expression's bytes and are refilled when a source changes."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LABEL_CHILD = (
    "import numpy as np, torch\n"
    "import inst_ref\n"
    "from tomosar2height_amd.instances import label_components\n"
    "mask = np.zeros((8, 8), np.int32)\n"
    "mask[0, 0] = 3; mask[1, 1] = 3; mask[0, 5:8] = 1; mask[3:6, 2] = 9; mask[5, 3:6] = 9; mask[7, 7] = 2; mask[7, 0] = -4\n"
    "labels, K = label_components(torch.from_numpy(mask).to('cuda:0'))\n"          # int32: goes through t2h_eval_predicate
    "want, want_k = inst_ref.label(mask)\n"
    "assert K == want_k == 5, (K, want_k)\n"
    "assert labels.dtype == torch.int32 and labels.cpu().numpy().tobytes() == want.tobytes(), labels\n"
    "print('child ok')\n")

MEDIANS_CHILD = (
    "import numpy as np, torch\n"
    "import cloud_inst_ref\n"
    "from tomosar2height_amd.cloud_instances import point_medians\n"
    "rng = np.random.default_rng(16)\n"
    "z = np.round(rng.standard_normal(16) * 8) / 4\n"
    "lab = np.array([1, 2, 1, 1, 2, 0, 2, 1, 2, 2, 1, 0, 2, 1, 2, 1], np.int32)\n"
    "counts, med = point_medians(torch.from_numpy(z).to('cuda:0'), torch.from_numpy(lab).to('cuda:0'), 2)\n"
    "want_counts, want = cloud_inst_ref.point_medians(z, lab, 2)\n"
    "assert want_counts.tolist() == [7, 7]\n"
    "assert counts.dtype == torch.int32 and counts.cpu().numpy().tobytes() == want_counts.tobytes(), counts\n"
    "assert med.dtype == torch.float64 and cloud_inst_ref.same_floats(med.cpu().numpy(), want), (med, want)\n"
    "print('child ok')\n")


def test_first_call_of_a_process_crosses_headers():
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    for code in (LABEL_CHILD, MEDIANS_CHILD):            # one after the other; the first failure ends the test
        out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "child ok" in out.stdout, f"exit {out.returncode}\n{out.stdout}{out.stderr}"


def test_folded_layers_are_the_float64_expression_and_follow_their_sources():
    from tomosar2height_amd.encoder.pointnetpp import PointNetSetAbstraction
    torch.manual_seed(6)
    sa = PointNetSetAbstraction(npoint=4, radius=0.5, nsample=4, in_channel=6, mlp=[8, 8], group_all=False)
    with torch.no_grad():
        for bn in sa.mlp_bns:
            bn.weight.copy_(torch.rand(8) + 0.5), bn.bias.copy_(torch.randn(8))
            bn.running_mean.copy_(torch.randn(8)), bn.running_var.copy_(torch.rand(8) + 0.25)
    sa = sa.eval().to("cuda:0")

    def expected():
        layers = []
        for conv, bn in zip(sa.mlp_convs, sa.mlp_bns):
            w, b, gamma, beta, mean, var = (t.detach().cpu().numpy().astype(np.float64) for t in (
                conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var))
            s = gamma / np.sqrt(var + bn.eps)
            w = w.reshape(w.shape[0], -1) * s[:, None]
            wp = np.zeros((w.shape[0], (w.shape[1] + 3) // 4 * 4), np.float32)
            wp[:, :w.shape[1]] = w.astype(np.float32)
            layers.append((wp, ((b - mean) * s + beta).astype(np.float32)))
        return layers

    def same(got, want):
        assert len(got) == len(want) == 2
        for (w, b), (ww, wb) in zip(got, want):
            assert w.dtype == b.dtype == torch.float32 and w.is_contiguous() and b.is_contiguous()
            assert tuple(w.shape) == ww.shape == (8, 8) and tuple(b.shape) == wb.shape == (8,)
            assert w.cpu().numpy().tobytes() == ww.tobytes() and b.cpu().numpy().tobytes() == wb.tobytes()

    first = sa.folded()
    want = expected()
    assert not want[0][0][:, 6:].any() and want[0][0][:, :6].all()                # in_channel 6 padded to rows of 8
    same(first, want)
    again = sa.folded()
    assert again is first and all(a is b for x, y in zip(again, first) for a, b in zip(x, y))
    assert "_fold" in sa.__dict__ and not any("_fold" in k for k in sa.state_dict())
    sa.mlp_bns[1].running_var.add_(1)
    second = sa.folded()
    assert second is not first and all(a is not b for x, y in zip(second, first) for a, b in zip(x, y))
    changed = expected()
    same(second, changed)
    assert changed[0][1].tobytes() == want[0][1].tobytes() and changed[1][1].tobytes() != want[1][1].tobytes()
    assert sa.folded() is second
