"""numpy restatement of the interpolation baselines (tomosar2height_amd.interpolate): brute force, float64, no k-d tree.

``unique_cloud`` is ``df.groupby(['X', 'Y']).max()`` (rows in X, then Y order); ``knn`` orders the candidates of every grid
node by (d2, X, Y) with ``d2 = dx * dx + dy * dy`` (two products, one sum) -- in the unique cloud's own order that is "smaller
index first", which a stable sort gives -- and also says, per node, whether ranks k and k + 1 tie (the k-d tree of the
reference may then return either); ``idw`` has the device's fixed order: ``s`` = sequential sum of the weights in rank order,
result = sequential sum of ``(w / s) * z``.
"""
import math

import numpy as np


def unique_cloud(points):
    """[M, 3]: one row per distinct (X, Y) with the largest Z, sorted by X, then Y."""
    p = np.asarray(points, np.float64)
    order = np.lexsort((-p[:, 2], p[:, 1], p[:, 0]))
    s = p[order]
    first = np.r_[True, (s[1:, 0] != s[:-1, 0]) | (s[1:, 1] != s[:-1, 1])]
    return np.ascontiguousarray(s[first])


def grid(unique, resolution=1.0):
    """``(gx [nx], gy [ny], (xmin, ymin))``: node coordinates ``i * res + min``, the maximum excluded."""
    xmin, xmax = unique[:, 0].min(), unique[:, 0].max()
    ymin, ymax = unique[:, 1].min(), unique[:, 1].max()
    nx, ny = int(math.ceil((xmax - xmin) / resolution)), int(math.ceil((ymax - ymin) / resolution))
    return np.arange(nx) * resolution + xmin, np.arange(ny) * resolution + ymin, (xmin, ymin)


def knn(unique, resolution=1.0, k=8):
    """``(d2 [ny, nx, k], idx [ny, nx, k] int32 into unique, tie [ny, nx] bool)``; ``tie`` = ranks k and k + 1 are at the same
    distance (False where the cloud has only k points)."""
    u = np.asarray(unique, np.float64)
    assert len(u) >= k
    xs, ys, _ = grid(u, resolution)
    ny, nx = len(ys), len(xs)
    d2 = np.empty((ny, nx, k))
    idx = np.empty((ny, nx, k), np.int32)
    tie = np.zeros((ny, nx), bool)
    for j in range(ny):
        dy = u[None, :, 1] - ys[j]
        dx = u[None, :, 0] - xs[:, None]
        dd = dx * dx + dy * dy                                    # [nx, M]
        order = np.argsort(dd, axis=1, kind="stable")             # unique is in (X, Y) order: stable = the tie rule
        top = order[:, :k]
        d2[j] = np.take_along_axis(dd, top, 1)
        idx[j] = top
        if len(u) > k:
            tie[j] = np.take_along_axis(dd, order[:, k:k + 1], 1)[:, 0] == d2[j, :, k - 1]
    return d2, idx, tie


def nearest(unique, resolution=1.0):
    d2, idx, tie = knn(unique, resolution, 1)
    return np.asarray(unique)[idx[..., 0], 2], tie


def idw(unique, resolution=1.0, k=8):
    d2, idx, tie = knn(unique, resolution, k)
    z = np.asarray(unique)[idx, 2]
    dist = np.sqrt(d2)
    with np.errstate(divide="ignore"):
        w = np.where(dist == 0, 1.0, 1.0 / (dist * dist))
    s = w[..., 0].copy()
    for m in range(1, k):
        s = s + w[..., m]
    out = (w[..., 0] / s) * z[..., 0]
    for m in range(1, k):
        out = out + (w[..., m] / s) * z[..., m]
    return out, tie


def idw_bound(z):
    """32 * 2^-53 * max|z|: five roundings per term, seven additions of terms that sum to at most max|z|, doubled for the
    reference's pairwise order."""
    return 32.0 * 2.0 ** -53 * float(np.abs(z).max())


def rows_as_set(a):
    """The rows of an [n, 3] float64 array as sorted bytes: equal as sets of rows <=> equal here (for distinct rows)."""
    a = np.ascontiguousarray(a, np.float64)
    return sorted(r.tobytes() for r in a)
