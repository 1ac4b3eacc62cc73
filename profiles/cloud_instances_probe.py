"""How long do the device point-cloud building-wise metrics take, and how far ahead of the host path are they?  (DESIGN.md
section 4.7)

    python profiles/cloud_instances_probe.py [--out FILE] [--repeats 20] [--warmup 3]

Shape: the Berlin test chunk's raster, 1660 x 1990 at 1 m, with the synthetic footprint of instances_probe.py and a synthetic
cloud of about 3.2 M float64 points (uniform over the raster plus a margin, unordered).  HIP-event timing of the three entry
points (assign, medians, metrics) through ``_lib.KernelTimeline`` and of a whole ``eval`` on an evaluator whose labels and
raster medians are cached, and the vectorised numpy restatement (tests/cloud_inst_ref.py) on this host with the cloud
already in host memory.  Bytes are the algorithmic ones of DESIGN section 4.7.
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
sys.path.insert(0, os.path.join(ROOT, "profiles"))

import cloud_inst_ref  # noqa: E402
from instances_probe import berlin_case, timed  # noqa: E402
from tomosar2height_amd import CloudBuildingEvaluator, _lib, cloud_instances  # noqa: E402


def cloud_case(H, W, transform, n_points=3_200_000, seed=23):
    rng = np.random.default_rng(seed)
    col = rng.random(n_points) * (W + 20) - 10
    row = rng.random(n_points) * (H + 20) - 10
    a, b, c, d, e, f = transform
    x, y = col * a + row * b + c, col * d + row * e + f
    z = 35 + rng.standard_normal(n_points) * 6
    return np.round(np.stack([x, y, z], 1) * 1000.0) / 1000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _, ndsm, mask = berlin_case()
    H, W = mask.shape
    rng = np.random.default_rng(24)
    dtm = (30 + rng.standard_normal((H, W)) * 0.3).astype(np.float32)
    transform = (1.0, 0.0, 392000.0, 0.0, -1.0, 5820000.0 + H)
    pts = cloud_case(H, W, transform)
    N = pts.shape[0]
    mask_d, dtm_d, ndsm_d, pts_d = (torch.from_numpy(a).to(dev) for a in (mask, dtm, ndsm, pts))
    ev = CloudBuildingEvaluator(mask_d, dtm_d, ndsm_d, transform)
    ev.buildings()

    for _ in range(args.warmup):
        metrics, rec = ev.eval(pts_d, mode="all")
    (metrics, rec), ev_ms, ev_wall = timed(lambda: ev.eval(pts_d, mode="all"), args.repeats)
    with _lib.KernelTimeline() as tl:
        for _ in range(args.repeats):
            ev.eval(pts_d, mode="all")
        torch.cuda.synchronize()
    per_entry = {k: v["ms"] / v["calls"] for k, v in tl.summary().items()}

    labels = rec["labels"].cpu().numpy()
    K = int(rec["counts"].numel())
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        point_label, _ = cloud_inst_ref.assign(pts, labels, transform)
        counts, pred_med = cloud_inst_ref.point_medians(pts[:, 2], point_label, K)
        want, _ = cloud_inst_ref.metrics(pred_med, rec["dtm_median"].cpu().numpy(), rec["ndsm_median"].cpu().numpy(), counts, "all")
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert rec["point_label"].cpu().numpy().tobytes() == point_label.tobytes()
    assert rec["counts"].cpu().numpy().tobytes() == counts.tobytes()
    assert cloud_inst_ref.same_floats(rec["pred_median"].cpu().numpy(), pred_med)
    assert metrics["MedAE-B"] == want["MedAE-B"] and abs(metrics["MAE-B"] - want["MAE-B"]) <= 1e-12 * want["MAE-B"]
    members = int(counts.sum())
    large = int((counts > cloud_instances.SMALL_MAX).sum())
    in_large = int(counts[counts > cloud_instances.SMALL_MAX].sum())

    assign_bytes = N * (24 + 4 + 4)
    med_bytes = N * 4 + N * (4 + 8) + members * 12 + members * 8 + 8 * 12 * in_large
    t_assign, t_med, t_met = (per_entry[k] for k in ("t2h_cloud_assign", "t2h_cloud_medians", "t2h_cloud_metrics"))
    lines = [
        f"point-cloud building-wise metrics probe: raster {H} x {W}, {N} points, {K} buildings, {members} points on buildings, "
        f"segment sizes {int(counts.min())} .. {int(counts.max())}, {large} above {cloud_instances.SMALL_MAX} holding {in_large}",
        f"device: {torch.cuda.get_device_name(0)}; warm-up {args.warmup}, repeats {args.repeats}",
        f"eval() on cached buildings (assign + medians + metrics), HIP events: median {statistics.median(ev_ms):.3f} ms, "
        f"min {min(ev_ms):.3f}, max {max(ev_ms):.3f}; wall clock incl. the table copy: median {statistics.median(ev_wall):.3f} ms",
        "per entry point (events, mean)      : " + ", ".join(f"{k} {v:.3f} ms" for k, v in sorted(per_entry.items())),
        f"device launches                      : assign {cloud_instances.LAUNCHES_PER_ASSIGN}, medians "
        f"{cloud_instances.LAUNCHES_PER_MEDIANS}, eval {cloud_instances.LAUNCHES_PER_EVAL} (+ 1 device-to-host copy of 64 B)",
        f"per launch                           : medians {t_med / cloud_instances.LAUNCHES_PER_MEDIANS * 1e3:.1f} us",
        f"algorithmic bytes                    : assign {assign_bytes / 1e6:.1f} MB, medians {med_bytes / 1e6:.1f} MB",
        f"achieved                             : assign {assign_bytes / t_assign / 1e6:.1f} GB/s, medians "
        f"{med_bytes / t_med / 1e6:.1f} GB/s, metrics {t_met * 1e3:.1f} us for {K} buildings",
        f"numpy restatement on this host       : median {statistics.median(host_ms):.1f} ms, min {min(host_ms):.1f} ms "
        f"(one lexsort; the reference's per-point Python loop is slower still)",
        f"ratio host / device (eval, wall)     : {statistics.median(host_ms) / statistics.median(ev_wall):.1f} x",
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
