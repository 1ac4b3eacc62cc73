"""Numpy restatement of the reference's building-wise evaluation (scripts/evaluator_instance.py:15-57) for the tests of
tomosar2height_amd.instances.  numpy only: neither skimage nor scipy is assumed.  Pinned to the reference by
tests/golden/building_instances.npz (test_instances_cpu.py)."""
import math

import numpy as np


def label(mask, connectivity=2):
    """``(labels int32, K)``: components of ``mask != 0``, 0 for background, 1..K in raster order of each component's first
    pixel -- skimage.measure.label's and scipy.ndimage.label's numbering.  Two passes over the row RUNS of the mask: runs of
    consecutive rows that touch (connectivity 2: also diagonally) are united under the smaller run index."""
    m = np.asarray(mask) != 0
    R, C = m.shape
    edge = np.diff(np.pad(m, ((0, 0), (1, 1))).astype(np.int8), axis=1)
    row, start = np.nonzero(edge == 1)                       # row-major, hence runs in raster order of their first pixel
    end = np.nonzero(edge == -1)[1]
    n_runs = row.size
    labels = np.zeros((R, C), np.int32)
    if n_runs == 0:
        return labels, 0
    parent = list(range(n_runs))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    first = np.searchsorted(row, np.arange(R + 1)).tolist()  # runs of row r: first[r] .. first[r + 1]
    s, e = start.tolist(), end.tolist()
    reach = 1 if connectivity == 2 else 0
    for r in range(1, R):
        a, a1, b, b1 = first[r - 1], first[r], first[r], first[r + 1]
        while a < a1 and b < b1:
            if s[a] < e[b] + reach and s[b] < e[a] + reach:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if e[a] < e[b]:
                a += 1
            else:
                b += 1
    root = np.array([find(i) for i in range(n_runs)])
    is_root = root == np.arange(n_runs)
    number = np.cumsum(is_root)                              # 1-based rank of a root among the roots
    labels[m] = np.repeat(number[root], end - start).astype(np.int32)
    return labels, int(is_root.sum())


def segment_medians(values, labels, K):
    """``(counts int32 [K], medians float32 [K])``: np.median(values32[labels == k]) for k = 1..K by ONE lexsort.  The median
    is (s[(n-1)/2] + s[n/2]) / 2 in float64, rounded once to float32; NaN for a segment with a NaN (numpy's rule) or no pixel."""
    v = np.asarray(values).astype(np.float32).ravel()
    lab = np.asarray(labels).ravel()
    member = (lab >= 1) & (lab <= K)
    v, lab = v[member], lab[member]
    order = np.lexsort((v, lab))                             # by label, then by value; NaNs last inside a label
    sv = v[order].astype(np.float64)
    counts = np.bincount(lab, minlength=K + 1)[1:K + 1]
    off = np.concatenate(([0], np.cumsum(counts)[:-1])) if K else np.zeros(0, np.int64)
    med = np.full(K, np.nan, np.float32)
    ok = counts > 0
    o, c = off[ok], counts[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        mid = ((sv[o + (c - 1) // 2] + sv[o + c // 2]) / 2.0 + 0.0).astype(np.float32)     # (+ 0.0: -0 to +0, as np.mean)
    mid[np.isnan(sv[o + c - 1])] = np.nan
    med[ok] = mid
    return counts.astype(np.int32), med


def middle(values):
    v = np.sort(np.asarray(values, dtype=np.float64))
    n = v.size
    return float((v[(n - 1) // 2] + v[n // 2]) / 2.0)


def metrics(pred_med, gt_med):
    """The aggregates of evaluator_instance.py:48-55 in float64 over the buildings whose two medians are finite."""
    p, g = np.asarray(pred_med, dtype=np.float64), np.asarray(gt_med, dtype=np.float64)
    valid = np.isfinite(p) & np.isfinite(g)
    d = np.abs(p[valid] - g[valid])
    n = int(d.size)
    out = {"RMSE-B": None, "MAE-B": None, "MedAE-B": None, "max_abs": None, "n_buildings": int(p.size), "n_valid": n,
           "n_nan": int(p.size) - n}
    if n:
        out.update({"RMSE-B": math.sqrt(math.fsum(d * d) / n), "MAE-B": math.fsum(d) / n, "MedAE-B": middle(d),
                    "max_abs": float(d.max())})
    return out


def evaluate(pred, gt, mask, connectivity=2):
    """(metrics, labels, counts, pred medians, gt medians) for three planes of one shape."""
    labels, K = label(mask, connectivity)
    counts, pm = segment_medians(pred, labels, K)
    _, gm = segment_medians(gt, labels, K)
    return metrics(pm, gm), labels, counts, pm, gm


def same_floats(got, want):
    """Byte for byte, except that any NaN equals any NaN (numpy keeps an input NaN's payload, the device writes the default)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    bits = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(bits)[~nan], want.view(bits)[~nan]))


def assert_metrics(got, want, rtol=1e-12):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key, w in want.items():
        g = got[key]
        if w is None or isinstance(w, int):
            assert g == w and type(g) is type(w), (key, g, w)
        else:
            assert isinstance(g, float) and (g == w or abs(g - w) <= rtol * abs(w)), (key, g, w)
