"""Numpy restatement of the reference's DSM evaluation (evaluator.py:14-99, utils/dilate_mask.py) for the tests of
tomosar2height_amd.evaluator.  numpy only: scipy is not assumed.  Pinned to the reference by tests/golden/dsm_evaluator.npz
(test_evaluator_cpu.py)."""
import math

import numpy as np

STAT_KEYS = ("max", "min", "MAE", "RMSE", "abs_median", "median", "n_pixel", "NMAD")


def dilate(mask, iterations=1):
    """scipy.ndimage.binary_dilation defaults: cross element, border value 0, ``iterations`` times -- by shifted ORs."""
    m = np.asarray(mask).astype(bool)
    for _ in range(iterations):
        out = m.copy()
        out[1:, :] |= m[:-1, :]
        out[:-1, :] |= m[1:, :]
        out[:, 1:] |= m[:, :-1]
        out[:, :-1] |= m[:, 1:]
        m = out
    return m


def class_masks(other_masks):
    """The reference's ``other_mask`` dict, in its insertion order (evaluator.py:27-51)."""
    out = {}
    other_masks = other_masks or {}
    if "building" in other_masks:
        out["building"] = dilate(np.asarray(other_masks["building"]).astype(bool), 2)
        out["terrain"] = ~out["building"]
    if "type" in other_masks:
        t = np.asarray(other_masks["type"])
        out["non_building"] = t == 0
        out["residential"] = dilate(t == 1, 2)
        out["non_residential"] = dilate(t == 2, 2)
        out["building_combined"] = dilate(t > 0, 2)
    for key, m in other_masks.items():
        if key not in ("building", "type"):
            out[key] = np.asarray(m).astype(bool)
    return out


def middle(values):
    """s[(n-1)/2] for odd n, (s[n/2-1] + s[n/2]) / 2 for even n."""
    v = np.asarray(values, dtype=np.float64)
    n = v.size
    s = np.partition(v, sorted({(n - 1) // 2, n // 2}))      # the two middle ranks in their sorted places: an exact selection
    return float(s[(n - 1) // 2]) if n % 2 else float((s[n // 2 - 1] + s[n // 2]) / 2.0)


def statistics(residual):
    r = np.asarray(residual, dtype=np.float64)
    if r.size == 0:
        return dict.fromkeys(STAT_KEYS)
    med = middle(r)
    with np.errstate(over="ignore"):                        # r * r of 1e300 is inf, here as in the reference
        sq = r * r
    return {"max": float(r.max()), "min": float(r.min()), "MAE": math.fsum(np.abs(r)) / r.size,
            "RMSE": math.sqrt(math.fsum(sq) / r.size), "abs_median": middle(np.abs(r)), "median": med, "n_pixel": int(r.size),
            "NMAD": 1.4826 * middle(np.abs(r - med))}


def evaluate(target, gt, gt_mask=None, other_masks=None, t_row=0, l_col=0):
    """(stats, diff) of evaluator.py:53-80 for a window that lies inside the ground truth."""
    target = np.asarray(target)
    H, W = target.shape
    gt = np.asarray(gt)
    assert 0 <= t_row and 0 <= l_col and t_row + H <= gt.shape[0] and l_col + W <= gt.shape[1]
    win = (slice(t_row, t_row + H), slice(l_col, l_col + W))
    gm = np.ones(gt.shape, bool) if gt_mask is None else np.asarray(gt_mask).astype(bool)
    gm = gm[win]
    with np.errstate(invalid="ignore", over="ignore"):
        residual = target.astype(np.float64) - gt[win].astype(np.float64)
    ok = ~np.isnan(residual)
    stats = {"overall": statistics(residual[gm & ok])}
    for name, m in class_masks(other_masks).items():
        stats[name] = statistics(residual[gm & m[win] & ok])
    diff = np.where(gm, residual, np.nan)
    return stats, diff


def assert_stats(got, want, exact_sums=False):
    """The issue's tolerances: order statistics, extrema, counts and Nones equal (-0.0 == 0.0); MAE / RMSE to rtol 1e-12."""
    assert list(got) == list(want), (list(got), list(want))
    for name in want:
        g, w = got[name], want[name]
        assert set(g) == set(STAT_KEYS), (name, g)
        for key in STAT_KEYS:
            if w[key] is None:
                assert g[key] is None, (name, key, g[key])
                continue
            assert g[key] is not None, (name, key)
            if key == "n_pixel":
                assert isinstance(g[key], int) and g[key] == w[key], (name, key, g[key], w[key])
            elif key in ("MAE", "RMSE") and not exact_sums:
                assert isinstance(g[key], float), (name, key, type(g[key]))
                assert g[key] == w[key] or abs(g[key] - w[key]) <= 1e-12 * abs(w[key]), (name, key, g[key], w[key])
            else:
                assert isinstance(g[key], float), (name, key, type(g[key]))
                assert g[key] == w[key], (name, key, g[key], w[key])


def assert_diff(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
