"""float64 restatement of the fused point-trunk backward that uses the SAME ReLU masks and arg-max bits as the kernels (so no
mask can flip); shared by test_hip_trunk.py and test_scratch_guard_gpu.py."""
import torch


def fused_backward_float64(tile, params, nets, hrs, winners, cats, g_out):
    """``params``: fc_pos (w, b), five tensors per block, fc_c (w, b); the rest as ``mlp._trunk_forward_fused(want_x_full=True)``
    returns them.  Returns the gradient of every entry of ``params``, in that order."""
    d = torch.float64
    nb = (len(params) - 4) // 5
    w = [p.to(d) for p in params]
    want = [None] * len(params)
    go = g_out.to(d)
    out_last = nets[-1].to(d)
    want[-2], want[-1] = go.t() @ torch.relu(out_last), go.sum(0)
    g = (go @ w[-2]) * (out_last > 0)
    cell = tile.cell.long()
    uniq, inv = torch.unique_consecutive(cell, return_inverse=True)
    for i in range(nb - 1, -1, -1):
        w0, b0, w1, b1, ws = w[2 + 5 * i: 7 + 5 * i]
        x, hr = cats[i].to(d), hrs[i].to(d)
        dhr = (g @ w1) * (hr > 0)
        want[2 + 5 * i: 7 + 5 * i] = [dhr.t() @ torch.relu(x), dhr.sum(0), g.t() @ hr, g.sum(0), g.t() @ x]
        dx = g @ ws + (dhr @ w0) * (x > 0)
        if i > 0:
            sums = torch.zeros(len(uniq), 32, dtype=d, device=dx.device).index_add_(0, inv, dx[:, 32:])
            bits = winners[i - 1]
            mask = torch.stack([(bits[:, ch // 4] >> (ch % 4)) & 1 for ch in range(32)], 1).to(d)
            g = dx[:, :32] + mask * sums[inv]
        else:
            want[0], want[1] = dx.t() @ tile.pts.to(d), dx.sum(0)
    return want
