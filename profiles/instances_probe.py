"""Are the device building-wise metrics launch-bound, and how far ahead of the host path are they?  

    python profiles/instances_probe.py [--out FILE] [--repeats 20] [--warmup 3]

Shape: the Berlin test chunk, 1660 x 1990, with a synthetic footprint of a few thousand buildings (rectangles, L-shapes, salt).
HIP-event timing of the window's first use (labels + ground-truth medians, a fresh ``BuildingEvaluator`` each repeat) and of the
``eval`` that follows it, per entry point through ``_lib.KernelTimeline``, and the numpy restatement (tests/inst_ref.py) on this
host with the mosaic already in host memory.  Bytes are the algorithmic ones of DESIGN section 4.5.
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

import inst_ref  # noqa: E402
from tomosar2height_amd import BuildingEvaluator, _lib, instances  # noqa: E402


def berlin_case(seed=22, H=1660, W=1990):
    rng = np.random.default_rng(seed)
    mask = np.zeros((H, W), np.uint8)
    for i in range(2500):
        y, x, h, w = rng.integers(0, H - 60), rng.integers(0, W - 60), rng.integers(6, 50), rng.integers(6, 50)
        mask[y:y + h, x:x + w] = 1
        if i % 3 == 0:
            mask[y + h // 2:y + h, x + w // 2:x + w] = 0
    mask[rng.random((H, W)) < 0.002] = 1
    gt = ((rng.standard_normal((H, W)) * 3 + 15) * mask).astype(np.float32)
    pred = gt.astype(np.float64) + rng.standard_normal((H, W)) * 1.7 + 0.3
    return pred, gt, mask


def timed(fn, repeats):
    ev_ms, wall_ms = [], []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        ev_ms.append(s.elapsed_time(e))
    return out, ev_ms, wall_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pred, gt, mask = berlin_case()
    H, W = mask.shape
    n = mask.size
    mask_d, gt_d, pred_d = (torch.from_numpy(a).to(dev) for a in (mask, gt, pred))

    def construct():
        ev = BuildingEvaluator(mask_d, gt_d, bounds=(0.0, 0.0))
        ev.buildings(0, 0, H, W)
        return ev

    for _ in range(args.warmup):
        ev = construct()
        metrics, rec = ev.eval(pred_d)
    ev, con_ms, con_wall = timed(construct, args.repeats)
    (metrics, rec), ev_ms, ev_wall = timed(lambda: ev.eval(pred_d), args.repeats)
    with _lib.KernelTimeline() as tl:
        for _ in range(args.repeats):
            construct().eval(pred_d)
        torch.cuda.synchronize()
    per_entry = {k: v["ms"] / v["calls"] for k, v in tl.summary().items()}

    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        want, labels, counts, pm, gm = inst_ref.evaluate(pred, gt, mask)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    inst_ref.assert_metrics(metrics, want)
    assert rec["labels"].cpu().numpy().tobytes() == labels.tobytes()
    K, members = int(counts.size), int(counts.sum())
    large = int((counts > instances.SMALL_MAX).sum())

    label_bytes = n * (1 + 4) + 3 * 8 * members + n * (4 + 4) + n * 4 + n * 8     # tile pass, merge (edges only: bounded by this),
    #                                                                              flatten, rank, relabel
    med_bytes = n * 4 + n * (4 + 8) + members * 8 + members * 4 + 4 * 8 * int(counts[counts > instances.SMALL_MAX].sum())
    lines = [
        f"building-wise metrics probe: {H} x {W} = {n} px, {K} buildings, {members} member pixels, sizes {int(counts.min())} .. "
        f"{int(counts.max())}, {large} above {instances.SMALL_MAX}",
        f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}",
        f"first use of a window (labels + gt medians), HIP events: median {statistics.median(con_ms):.3f} ms, min {min(con_ms):.3f}, "
        f"max {max(con_ms):.3f}; wall clock incl. the 4-byte copy of K: median {statistics.median(con_wall):.3f} ms",
        f"eval() after it (pred medians + metrics), HIP events  : median {statistics.median(ev_ms):.3f} ms, min {min(ev_ms):.3f}, "
        f"max {max(ev_ms):.3f}; wall clock incl. the table copy: median {statistics.median(ev_wall):.3f} ms",
        "per entry point (events, mean)      : " + ", ".join(f"{k} {v:.3f} ms" for k, v in sorted(per_entry.items())),
        f"device launches                      : label {instances.LAUNCHES_PER_LABEL}, medians {instances.LAUNCHES_PER_MEDIANS}, "
        f"eval {instances.LAUNCHES_PER_EVAL} (+ 1 device-to-host copy of 64 B)",
        f"per launch                           : label {per_entry['t2h_inst_label'] / instances.LAUNCHES_PER_LABEL * 1e3:.1f} us, "
        f"medians {per_entry['t2h_inst_medians'] / instances.LAUNCHES_PER_MEDIANS * 1e3:.1f} us",
        f"algorithmic bytes                    : label {label_bytes / 1e6:.1f} MB, medians of one plane {med_bytes / 1e6:.1f} MB",
        f"achieved                             : label {label_bytes / per_entry['t2h_inst_label'] / 1e6:.1f} GB/s, "
        f"medians {med_bytes / per_entry['t2h_inst_medians'] / 1e6:.1f} GB/s",
        f"numpy restatement on this host       : median {statistics.median(host_ms):.1f} ms, min {min(host_ms):.1f} ms "
        f"(labels by row runs, medians by one lexsort; the reference's per-building np.where loop is slower still)",
        f"ratio host / device (first use + eval, wall): "
        f"{statistics.median(host_ms) / (statistics.median(con_wall) + statistics.median(ev_wall)):.1f} x",
        f"metrics                              : {metrics}",
    ]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
