"""Is the device DSM evaluator launch-bound, and is it ahead of the host path?  

    python profiles/dsm_eval_probe.py [--out FILE] [--repeats 20] [--warmup 3]

Shape: the Berlin test chunk, 1660 x 1990, with the seven Berlin classes from a synthetic footprint.  HIP-event timing of
``DSMEvaluator.eval`` (events around the whole call, and per entry point through ``_lib.KernelTimeline``), wall-clock of the
same call, and the numpy restatement (tests/eval_ref.py) on this host with the mosaic already in host memory plus the copy a
user of the host path pays first.  Bytes are the algorithmic ones: 10 B per pixel and pass (8 B residual + 2 B class bits), 17
passes (sums + 2 rounds x 8 digit passes), plus the residual launch.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import eval_ref  # noqa: E402
from tomosar2height_amd import DSMEvaluator, _lib, evaluator  # noqa: E402


def berlin_case(seed=21, H=1660, W=1990):
    rng = np.random.default_rng(seed)
    type_plane = np.zeros((H, W), np.uint8)
    for _ in range(900):
        y, x, h, w = rng.integers(0, H - 40), rng.integers(0, W - 40), rng.integers(6, 40), rng.integers(6, 40)
        type_plane[y:y + h, x:x + w] = rng.integers(1, 3)
    building = (type_plane > 0).astype(np.uint8)
    gt = (rng.standard_normal((H, W)) * 6 + 20).astype(np.float32) * (1 + building)
    target = gt.astype(np.float64) + rng.standard_normal((H, W)) * 1.7 + 0.3 * building
    target[rng.random((H, W)) < 0.01] = np.nan
    return target, gt, {"building": building, "type": type_plane}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    target, gt, other = berlin_case()
    n = target.size
    t0 = time.perf_counter()
    ev = DSMEvaluator(torch.from_numpy(gt).to(dev), bounds=(0.0, 0.0), other_masks={k: torch.from_numpy(v).to(dev) for k, v in other.items()})
    torch.cuda.synchronize()
    construct_ms = (time.perf_counter() - t0) * 1e3
    tgt = torch.from_numpy(target).to(dev)
    for _ in range(args.warmup):
        stats, _ = ev.eval(tgt)
    ev_ms, wall_ms = [], []
    for _ in range(args.repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        ev.eval(tgt)
        e.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(s.elapsed_time(e))
    with _lib.KernelTimeline() as tl:
        for _ in range(args.repeats):
            ev.eval(tgt)
        torch.cuda.synchronize()
    per_entry = {k: v["ms"] / v["calls"] for k, v in tl.summary().items()}

    t0 = time.perf_counter()
    host_target = tgt.cpu().numpy()
    copy_ms = (time.perf_counter() - t0) * 1e3
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want, _ = eval_ref.evaluate(host_target, gt, None, other)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    eval_ref.assert_stats(stats, want)

    med = statistics.median(ev_ms)
    stats_ms = per_entry["t2h_eval_stats"]
    pass_bytes = 17 * 10 * n
    all_bytes = pass_bytes + n * (8 + 4 + 2 + 8 + 2)
    lines = [
        f"DSM evaluator probe: {target.shape[0]} x {target.shape[1]} = {n} px, classes {ev.class_names}",
        f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}",
        f"eval(), HIP events around the call : median {med:.3f} ms, min {min(ev_ms):.3f} ms, max {max(ev_ms):.3f} ms",
        f"eval(), wall clock incl. the table copy: median {statistics.median(wall_ms):.3f} ms, min {min(wall_ms):.3f} ms",
        f"per entry point (events, mean)      : " + ", ".join(f"{k} {v:.3f} ms" for k, v in sorted(per_entry.items())),
        f"device launches per eval()           : {evaluator.LAUNCHES_PER_EVAL} (+ 1 device-to-host copy of {len(ev.class_names) * 64} B)",
        f"t2h_eval_stats per launch            : {stats_ms / (evaluator.LAUNCHES_PER_EVAL - 1) * 1e3:.1f} us over {evaluator.LAUNCHES_PER_EVAL - 1} launches",
        f"algorithmic bytes                    : {all_bytes / 1e6:.1f} MB per eval ({pass_bytes / 17 / 1e6:.1f} MB per pass)",
        f"achieved                             : {all_bytes / med / 1e6:.1f} GB/s over the call, {pass_bytes / stats_ms / 1e6:.1f} GB/s inside t2h_eval_stats",
        f"evaluator construction (once)        : {construct_ms:.1f} ms wall (class bits, 4 dilations, first-call overheads included)",
        f"numpy restatement on this host       : median {statistics.median(host_ms):.1f} ms, min {min(host_ms):.1f} ms (+ {copy_ms:.1f} ms to copy the mosaic to the host)",
        f"ratio host / device (wall)           : {statistics.median(host_ms) / statistics.median(wall_ms):.1f} x",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
