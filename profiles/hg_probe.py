"""What does the hourglass image encoder cost at the Berlin image's size, and what do its own kernels achieve?  

    python profiles/hg_probe.py [--out FILE, default profiles/r13_hourglass.txt] [--size 512] [--repeats 10] [--warmup 3]

HGFilter(in_channel=3, feature_dim=32), constructor defaults otherwise (group norm, average pool, 4 stacks of depth 2), on one
image [1, 3, size, size] (512: one image of BASELINE.json configs[2]).  HIP events around whole forwards after a warm-up, the HIP
path and the plain-torch baseline alternating; the baseline is tests/hg_ref.py's restatement in float32 on the same device
(MIOpen / ATen kernels) with the same parameters.  Then, per entry point of include/t2h_hg.h, (a) its calls within one forward
(events around every call: small planes are launch-bound) and (b) the largest call of the forward alone, `--inner` launches back
to back between two events: algorithmic bytes over time against the 8 TB/s HBM figure bench.py uses.  Every step runs under a
time limit (an alarm) and the script stops at the first step that fails.  No time is asserted anywhere.
"""
import argparse
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GBS = 8000.0          # as bench.py


class step:
    def __init__(self, name, limit):
        self.name, self.limit = name, limit

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._late)
        signal.alarm(self.limit)

    def _late(self, *a):
        raise TimeoutError(f"step '{self.name}' exceeded {self.limit} s")

    def __exit__(self, kind, exc, tb):
        signal.alarm(0)
        if kind is not None:
            print(f"FAILED at step '{self.name}': {kind.__name__}: {exc}", flush=True)
            sys.exit(1)


def event_ms(fn, inner=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def fmt(ms):
    return f"median {statistics.median(ms):9.3f} ms, min {min(ms):9.3f} ms, max {max(ms):9.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_hourglass.txt"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    args = ap.parse_args()

    import hg_ref
    from tomosar2height_amd import _lib, grid
    from tomosar2height_amd.encoder import hourglass as hg
    dev = torch.device("cuda:0")
    enc = hg_ref.init_hg_(hg.HGFilter(in_channel=3, feature_dim=32)).to(dev).eval()
    base = hg_ref.TorchHGFilter(enc, torch.float32, dev)
    image = (torch.rand(1, 3, args.size, args.size, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    lines = [f"hourglass encoder probe: image [1, 3, {args.size}, {args.size}], in_channel 3, feature_dim 32, group norm, ave_pool, "
             f"4 stacks of depth 2; conv precision {grid.CONV_PRECISION}",
             f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}, HIP events"]

    with torch.no_grad():
        with step("warm-up", args.limit):
            for _ in range(args.warmup):
                out, ref = enc(image), base(image)
            torch.cuda.synchronize()
        lines.append(f"max |HIP - torch baseline| of the output: {float((out - ref).abs().max()):.3g} (max |output| {float(ref.abs().max()):.3g})")
        ours, theirs = [], []
        with step("forwards", args.limit):
            for _ in range(args.repeats):                     # alternating: both see the same neighbours on the machine
                ours.append(event_ms(lambda: enc(image)))
                theirs.append(event_ms(lambda: base(image)))
        lines.append(f"{'HGFilter forward, HIP kernels':46s}: {fmt(ours)}")
        lines.append(f"{'HGFilter forward, plain torch (float32)':46s}: {fmt(theirs)}")
        lines.append(f"ratio of the medians (torch / HIP): {statistics.median(theirs) / statistics.median(ours):.2f}")

        with step("per entry point", args.limit):
            with _lib.KernelTimeline() as tl:
                enc(image)
            torch.cuda.synchronize()
            summary = tl.summary()
        total = sum(d["ms"] for d in summary.values())
        lines.append(f"one forward, events around every entry-point call ({sum(d['calls'] for d in summary.values())} calls, {total:.3f} ms in all):")
        for name, d in sorted(summary.items(), key=lambda kv: -kv[1]["ms"]):
            gbs = d["bytes"] / d["ms"] / 1e6 if d["ms"] > 0 else 0.0
            mine = "*" if name.startswith("t2h_hg_") else " "
            lines.append(f"  {mine} {name:40s} {d['calls']:4d} calls {d['ms']:9.3f} ms {gbs:9.1f} GB/s ({100 * gbs / HBM_PEAK_GBS:5.1f} % of 8 TB/s)")
        lines.append("  (* = the entry points of include/t2h_hg.h)")

        # the largest call of each new kernel in this forward, alone
        q, h = args.size // 2, args.size // 4
        stem_in = image.contiguous(memory_format=torch.channels_last)
        w_stem = enc.conv1.weight.detach().permute(2, 3, 1, 0).contiguous()
        x64 = torch.randn(1, 64, q, q, device=dev).contiguous(memory_format=torch.channels_last)
        x128 = torch.randn(1, 128, q, q, device=dev).contiguous(memory_format=torch.channels_last)
        x256 = torch.randn(1, 256, h, h, device=dev).contiguous(memory_format=torch.channels_last)
        parts = [torch.randn(1, c, h, h, device=dev).contiguous(memory_format=torch.channels_last) for c in (128, 64, 64)]
        gn, st = enc.bn1, hg.group_norm_stats(x64, 32, 1e-5)
        alone = [
            (f"t2h_hg_conv_s2_fwd 7x7 3->64 on {args.size}^2", lambda: hg.conv_s2(stem_in, w_stem, enc.conv1.bias, 7, 3),
             4 * (stem_in.numel() + 64 * q * q + w_stem.numel())),
            (f"t2h_hg_groupnorm_stats C=64 on {q}^2", lambda: hg.group_norm_stats(x64, 32, 1e-5), 4 * x64.numel()),
            (f"t2h_hg_norm_apply C=64 on {q}^2", lambda: hg.norm_apply(x64, st, gn.weight, gn.bias, 32, True), 8 * x64.numel()),
            (f"t2h_hg_groupnorm_stats C=256 on {h}^2", lambda: hg.group_norm_stats(x256, 32, 1e-5), 4 * x256.numel()),
            (f"t2h_hg_avgpool2x2 C=128 on {q}^2", lambda: hg.avgpool2x2(x128), 5 * x128.numel()),
            (f"t2h_hg_block_tail C=256 on {h}^2", lambda: hg.block_tail(parts[0], parts[1], parts[2], x256), 12 * x256.numel()),
        ]
        lines.append(f"largest call of each new kernel alone ({args.inner} launches back to back per sample, {args.repeats} samples):")
        for name, fn, nbytes in alone:
            with step(name, args.limit):
                fn()
                ms = [event_ms(fn, args.inner) for _ in range(args.repeats)]
            gbs = nbytes / statistics.median(ms) / 1e6
            lines.append(f"  {name:46s}: {fmt(ms)}  {gbs:8.1f} GB/s ({100 * gbs / HBM_PEAK_GBS:5.1f} % of 8 TB/s)")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
