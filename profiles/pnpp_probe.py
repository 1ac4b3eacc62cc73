"""What does the PointNet++ encoder cost at the Berlin tile's size, and where does the time go?  

    python profiles/pnpp_probe.py [--out FILE, default profiles/r12_pnpp.txt] [--points 131072] [--repeats 10] [--warmup 3]
    python profiles/pnpp_probe.py --reference          # on a host that holds the reference tree: its encoder forward on the CPU
    python profiles/pnpp_probe.py --batch-statistics   # train() with BatchNorm batch statistics: forward, forward + backward
                                                       # (default --out profiles/pnpp_train_probe.txt)

N = 131 072, B = 1, plane resolution 256, ALTO depth 5, feature_dim 32.  HIP events around every stage of the point side on its
real inputs and around the whole encoder forward, after a warm-up; the launches of one forward.  Every step runs under a time
limit (``--limit`` seconds, an alarm) and the script stops at the first step that fails or runs out of time.  The comparison
point is the reference's own encoder forward at the same size on the host CPU, taken once through the fixture generator's import
path (``--reference``); both modes keep the other's lines in the output file.  No time is asserted anywhere.
"""
import argparse
import os
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KW = dict(feature_dim=32, dim=3, unet_type="alto", unet_kwargs=dict(depth=5, merge_mode="concat", start_filts=32), plane_resolution=256)
HOST_TAG = "host reference"


def cloud(n):
    g = torch.Generator().manual_seed(5)
    xy = torch.rand(1, n, 2, generator=g).clamp(2.0 ** -20, 1 - 2.0 ** -20)
    return torch.cat([xy, torch.rand(1, n, 1, generator=g) * 0.6], 2).float().contiguous()


class step:
    """``with step(name, limit):`` -- an alarm around one step; any failure ends the script."""

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


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return out, ms


def fmt(ms):
    return f"median {statistics.median(ms):9.3f} ms, min {min(ms):9.3f} ms, max {max(ms):9.3f} ms"


def write(path, lines, keep_host):
    """Replace this mode's lines of the file, keep the other mode's."""
    old = open(path).read().splitlines() if os.path.exists(path) else []
    kept = [ln for ln in old if ln.startswith(HOST_TAG) == keep_host]
    text = "\n".join(lines + kept if keep_host else kept + lines)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")
    print(text)


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from ref_import import import_reference
    import_reference()
    from tomosar2height.encoder.pointnetpp import PointNetPlusPlus
    torch.manual_seed(0)
    enc = PointNetPlusPlus(**KW).eval()
    pts = cloud(args.points)
    with step("reference forward", args.limit), torch.no_grad():
        t0 = time.perf_counter()
        enc(pts)
        sec = time.perf_counter() - t0
    if not os.path.exists(args.out):
        write(args.out, [f"PointNet++ encoder probe: N = {args.points}, B = 1, resolution 256, ALTO depth 5",
                         "device: not measured"], keep_host=True)
    write(args.out, [f"{HOST_TAG}: encoder forward of the reference on this host's CPU ({torch.get_num_threads()} threads, float32, "
                     f"one run): {sec * 1e3:.0f} ms"], keep_host=False)


def device(args):
    from tomosar2height_amd import _lib, pointops
    from tomosar2height_amd.encoder.pointnetpp import PointNetPlusPlus
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = PointNetPlusPlus(**KW).to(dev).eval()
    enc.set_channels_last(True)
    enc.fps_start = 0
    pts = cloud(args.points).to(dev)
    n, lines, rows = args.points, [], []

    def stage(name, fn):
        with step(name, args.limit):
            out, ms = timed(fn, args.warmup, args.repeats)
        rows.append(f"{name:44s}: {fmt(ms)}")
        print(rows[-1], flush=True)
        return out

    with torch.no_grad():
        fps1 = stage(f"sa1 FPS ({pointops.fps_launches(n, 512)} launches)", lambda: pointops.farthest_point_sample(pts, 512, 0))
        l1 = pointops.index_points(pts, fps1).contiguous()
        idx1 = stage("sa1 ball query (r 0.2, 32)", lambda: pointops.query_ball_point(0.2, 32, pts, l1))
        rows1 = stage("sa1 grouped rows [16384, 8]", lambda: pointops.group_rows(pts, l1, pts, idx1, 8))
        feat1 = stage("sa1 layers 8 -> 64 -> 64 -> 128", lambda: enc.sa1._chain(rows1))
        p1 = stage("sa1 grouped max", lambda: pointops.group_max_rows(feat1, 32)).view(1, 512, 128)
        (l2, p2) = stage("sa2 whole (FPS in one launch)", lambda: enc.sa2.forward_rows(l1, p1, 0))
        (l3, p3) = stage("sa3 whole (group_all)", lambda: enc.sa3.forward_rows(l2, p2))
        q2 = stage("fp3 whole (S = 1)", lambda: enc.fp3.forward_rows(l2, l3, p2, p3))
        q1 = stage("fp2 whole", lambda: enc.fp2.forward_rows(l1, l2, p1, q2))
        stage(f"fp1 3-NN + interpolation [{n}, 128]", lambda: pointops.three_nn_interpolate(pts, l1, q1))
        stage("fp1 whole", lambda: enc.fp1.forward_rows(pts, l1, None, q1))
        stage("point side (sa1 .. fp1)", lambda: enc.point_features(pts))
        stage("encoder forward (index, points, plane, ALTO)", lambda: enc(pts))
        calls = {}
        real = _lib.call

        def counting(name, *a, **kw):
            calls[name] = calls.get(name, 0) + 1
            return real(name, *a, **kw)

        with step("launch census", args.limit):
            _lib.call = counting
            try:
                enc(pts)
            finally:
                _lib.call = real
    expand = {"t2h_fps": None, "t2h_three_nn_interp": None}
    launches = sum(v for k, v in calls.items() if k not in expand)
    launches += pointops.fps_launches(n, 512) + pointops.fps_launches(512, 128) + 1 + 2 + 2          # fp3: one launch, fp2 / fp1: two
    lines = [f"PointNet++ encoder probe: N = {n}, B = 1, resolution 256, ALTO depth 5",
             f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}, HIP events"] + rows
    lines += [f"entry-point calls per forward         : {sum(calls.values())} ({calls.get('t2h_linear_fwd', 0)} t2h_linear_fwd among them)",
              f"launches per forward                   : {launches} (FPS expanded: {pointops.fps_launches(n, 512)} + "
              f"{pointops.fps_launches(512, 128)}; 3-NN: 1 + 2 + 2; every other entry point counted as one)"]
    write(args.out, lines, keep_host=True)


def batch_statistics(args):
    """The encoder under train() with the opt-in batch statistics: forward under no_grad, forward with the graph, and forward +
    backward of L = sum(plane), every parameter of the encoder requiring a gradient."""
    from tomosar2height_amd.encoder.pointnetpp import PointNetPlusPlus
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = PointNetPlusPlus(**KW, batch_statistics=True).to(dev).train()
    enc.set_channels_last(True)
    enc.fps_start = 0
    pts = cloud(args.points).to(dev)
    rows = []

    def stage(name, fn):
        with step(name, args.limit):
            _, ms = timed(fn, args.warmup, args.repeats)
        rows.append(f"{name:52s}: {fmt(ms)}")
        print(rows[-1], flush=True)

    def no_grad():
        with torch.no_grad():
            return enc(pts)["xy"]

    def fwd_bwd():
        enc.zero_grad(set_to_none=True)
        enc(pts)["xy"].sum().backward()

    stage("train() forward, no_grad (statistics + updates)", no_grad)
    stage("train() forward with the autograd graph", lambda: enc(pts)["xy"])
    stage("train() forward + backward", fwd_bwd)
    enc.eval()
    stage("eval() forward, no_grad (folded, for comparison)", no_grad)
    lines = [f"PointNet++ encoder, BatchNorm batch statistics: N = {args.points}, B = 1, resolution 256, ALTO depth 5",
             f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}, HIP events"] + rows
    write(args.out, lines, keep_host=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", type=int, default=131072)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--reference", action="store_true", help="time the reference's encoder forward on the host CPU instead")
    ap.add_argument("--batch-statistics", action="store_true", help="time the encoder under train() with batch statistics instead")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "pnpp_train_probe.txt" if args.batch_statistics else "r12_pnpp.txt")
    if args.batch_statistics:
        batch_statistics(args)
    else:
        reference(args) if args.reference else device(args)


if __name__ == "__main__":
    main()
