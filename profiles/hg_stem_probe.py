"""What does training the hourglass encoder's stem cost?  ("Training the stem")

    python profiles/hg_stem_probe.py [--out FILE, default profiles/hg_stem_probe.txt] [--size 512] [--repeats 10] [--warmup 3]

HGFilter(3, 256, 2, 4), norm='group', on one image [1, 3, size, size], forward + backward of sum(out * cotangent), for
hg_down = 'ave_pool' and 'conv128', HIP events around whole steps after a warm-up, the three forms alternating:

    stem on      trainable=True, stem_gradients=True, every parameter trains (the image needs no gradient)
    stem frozen  trainable=True with conv1 (conv128: everything up to down_conv2) frozen: the path without the switch
    plain torch  tests/hg_ref.py in float32 under autograd on the same device (MIOpen / ATen), every parameter trains

Then t2h_hg_conv_s2_dgrad / _wgrad alone at conv1's and down_conv2's shapes (`--inner` launches back to back between two events)
beside torch's own conv2d backward for the same shapes (``torch.autograd.grad`` of the input / of weight and bias).  Every step
runs under a time limit and the script stops at the first step that fails.  No time is asserted anywhere.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from hg_probe import event_ms, fmt, step  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hg_stem_probe.txt"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--limit", type=int, default=180, help="seconds per step")
    args = ap.parse_args()

    import hg_ref
    from tomosar2height_amd import grid
    from tomosar2height_amd.encoder import hourglass as hg
    dev = torch.device("cuda:0")
    n = args.size
    image = (torch.rand(1, 3, n, n, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    cot = torch.randn(1, 256, n // 4, n // 4, generator=torch.Generator().manual_seed(4)).to(dev)
    lines = [f"hourglass stem probe: HGFilter(3, 256, 2, 4, 'group') on [1, 3, {n}, {n}], forward + backward; conv precision {grid.CONV_PRECISION}",
             f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}, HIP events"]

    for hg_down in ("ave_pool", "conv128"):
        on = hg_ref.init_hg_(hg.HGFilter(3, 256, 2, 4, hg_down=hg_down, trainable=True, stem_gradients=True)).to(dev)
        off = hg_ref.init_hg_(hg.HGFilter(3, 256, 2, 4, hg_down=hg_down, trainable=True)).to(dev)
        for name in ("conv1",) if hg_down == "ave_pool" else ("conv1", "bn1", "conv2", "down_conv2"):
            getattr(off, name).requires_grad_(False)
        params = {k: v.clone().requires_grad_(True) for k, v in hg_ref.params_of(on, torch.float32, dev).items() if v.is_floating_point()}
        kw = dict(num_hourglass=2, num_stack=4, hg_down=hg_down)

        def hip_step(net):
            net.zero_grad(set_to_none=True)
            (net(image) * cot).sum().backward()

        def torch_step():
            for p in params.values():
                p.grad = None
            (hg_ref.hg_filter(image, params, **kw) * cot).sum().backward()

        forms = (("stem on (this change)", lambda: hip_step(on)), ("stem frozen (the path without the switch)", lambda: hip_step(off)),
                 ("plain torch, float32", torch_step))
        with step(f"{hg_down} warm-up", args.limit):
            for _ in range(args.warmup):
                for _, fn in forms:
                    fn()
            torch.cuda.synchronize()
        times = {name: [] for name, _ in forms}
        with step(f"{hg_down} steps", args.limit):
            for _ in range(args.repeats):                     # alternating: all see the same neighbours on the machine
                for name, fn in forms:
                    times[name].append(event_ms(fn))
        lines.append(f"hg_down='{hg_down}':")
        for name, _ in forms:
            lines.append(f"  {name:44s}: {fmt(times[name])}")
        lines.append(f"  stem on - stem frozen (medians): {statistics.median(times[forms[0][0]]) - statistics.median(times[forms[1][0]]):+.3f} ms; "
                     f"plain torch / stem on: {statistics.median(times[forms[2][0]]) / statistics.median(times[forms[0][0]]):.2f}")
        del on, off, params

    lines.append(f"the two adjoint kernels alone ({args.inner} launches back to back per sample, {args.repeats} samples), beside torch's conv2d backward:")
    for what, cin, cout, k, pad, h in (("conv1 7x7 3->64", 3, 64, 7, 3, n), ("down_conv2 3x3 128->128", 128, 128, 3, 1, n // 2)):
        g = torch.Generator().manual_seed(k)
        x = torch.randn(1, cin, h, h, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        weight = (torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5).to(dev)
        bias = torch.zeros(cout, device=dev)
        wk = weight.permute(2, 3, 1, 0).contiguous()
        oh = (h + 2 * pad - k) // 2 + 1
        gy = torch.randn(1, cout, oh, oh, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
        xt, wt, bt = x.clone().requires_grad_(True), weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        flops = 2 * k * k * cin * cout * oh * oh
        rows = (
            (f"t2h_hg_conv_s2_dgrad {what}, {oh}^2 outputs", lambda: hg.conv_s2_dgrad(gy, wk, h, h, k, pad)),
            (f"torch conv2d backward, input  {what}", lambda: torch.autograd.grad(F.conv2d(xt, wt, bt, stride=2, padding=pad), xt, gy)),
            (f"t2h_hg_conv_s2_wgrad {what}, {oh}^2 outputs", lambda: hg.conv_s2_wgrad(x, gy, k, pad)),
            (f"torch conv2d backward, weight {what}", lambda: torch.autograd.grad(F.conv2d(xt, wt, bt, stride=2, padding=pad), (wt, bt), gy)),
            (f"torch conv2d forward alone    {what}", lambda: F.conv2d(xt, wt, bt, stride=2, padding=pad)),
        )
        for name, fn in rows:
            with step(name, args.limit):
                fn()
                ms = [event_ms(fn, args.inner) for _ in range(args.repeats)]
            lines.append(f"  {name:58s}: {fmt(ms)}  {flops / statistics.median(ms) / 1e9:7.2f} TFLOP/s of the {flops / 1e9:.2f} GFLOP")
    lines.append("  (torch's backward rows include the forward they differentiate: subtract the 'forward alone' row)")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
