"""numpy restatement of the Delaunay-linear baseline (tomosar2height_amd.interpolate.delaunay_dsm / grid_simplex), float64.

Everything works on SHIFTED coordinates, ``X - xmin`` and ``Y - ymin`` (each rounded once), as the device does: ``shifted`` for
the cloud, ``nodes`` for the raster (node i = ``(i * res + xmin) - xmin``).  ``barycentric`` evaluates, for a given table of
triangles (rows a <= b <= c of the cloud), ``cross(b - q, c - q) / cross(b - a, c - a)``, ``cross(c - q, a - q) / ...``,
``cross(a - q, b - q) / ...`` with ``cross(u, v) = u.x * v.y - u.y * v.x`` -- numpy rounds every difference, product and
quotient once, in the written order -- and ``linear`` the heights ``(l0 * z_a + l1 * z_b) + l2 * z_c``.  ``brute_force`` finds
the triangles themselves for a small cloud: of all triples that contain a node, the one whose circumcircle holds no other
point beyond the error bound of the in-circle determinant.
"""
import itertools
import math

import numpy as np

from interp_ref import unique_cloud  # noqa: F401  (the group-by restatement, shared with the other baselines)

EPS = 2.0 ** -53
ICC_ERR = (10.0 + 96.0 * EPS) * EPS                              # Shewchuk 1997, first-stage bound of the in-circle test


def shifted(unique):
    """``(P [M, 2], (xmin, ymin))``: the cloud's (X, Y) minus its minimum."""
    u = np.asarray(unique, np.float64)
    origin = (u[:, 0].min(), u[:, 1].min())
    return np.c_[u[:, 0] - origin[0], u[:, 1] - origin[1]], origin


def nodes(unique, resolution=1.0):
    """``(qx [nx], qy [ny])`` shifted node coordinates of the raster of ``unique`` (maximum excluded)."""
    u = np.asarray(unique, np.float64)
    xmin, xmax, ymin, ymax = u[:, 0].min(), u[:, 0].max(), u[:, 1].min(), u[:, 1].max()
    nx, ny = int(math.ceil((xmax - xmin) / resolution)), int(math.ceil((ymax - ymin) / resolution))
    return (np.arange(nx) * resolution + xmin) - xmin, (np.arange(ny) * resolution + ymin) - ymin


def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def barycentric(unique, tri, resolution=1.0):
    """``bary [ny, nx, 3]`` for ``tri [ny, nx, 3]`` (rows of ``unique``, -1 = no triangle -> NaN)."""
    P, _ = shifted(unique)
    qx, qy = nodes(unique, resolution)
    tri = np.asarray(tri, np.int64)
    assert tri.shape == (len(qy), len(qx), 3)
    ok = tri[..., 0] >= 0
    t = np.where(ok[..., None], tri, 0)
    a, b, c = P[t[..., 0]], P[t[..., 1]], P[t[..., 2]]
    QX, QY = np.broadcast_to(qx[None, :], ok.shape), np.broadcast_to(qy[:, None], ok.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        area = _cross(b[..., 0] - a[..., 0], b[..., 1] - a[..., 1], c[..., 0] - a[..., 0], c[..., 1] - a[..., 1])
        l0 = _cross(b[..., 0] - QX, b[..., 1] - QY, c[..., 0] - QX, c[..., 1] - QY) / area
        l1 = _cross(c[..., 0] - QX, c[..., 1] - QY, a[..., 0] - QX, a[..., 1] - QY) / area
        l2 = _cross(a[..., 0] - QX, a[..., 1] - QY, b[..., 0] - QX, b[..., 1] - QY) / area
    out = np.stack([l0, l1, l2], -1)
    out[~ok] = np.nan
    return out


def linear(unique, tri, resolution=1.0):
    """``dsm [ny, nx]``: the heights over ``tri``, NaN where there is no triangle."""
    u = np.asarray(unique, np.float64)
    lam = barycentric(u, tri, resolution)
    t = np.where(np.asarray(tri) >= 0, tri, 0).astype(np.int64)
    z = u[:, 2][t]
    out = (lam[..., 0] * z[..., 0] + lam[..., 1] * z[..., 1]) + lam[..., 2] * z[..., 2]
    out[np.asarray(tri)[..., 0] < 0] = np.nan
    return out


def units(got, want, unique, tri):
    """|got - want| in units of 2^-52 * max|z| of every node's three vertices (NaN where there is no triangle)."""
    t = np.where(np.asarray(tri) >= 0, tri, 0).astype(np.int64)
    zmax = np.abs(np.asarray(unique)[:, 2][t]).max(-1)
    with np.errstate(invalid="ignore"):
        return np.abs(got - want) / (2.0 ** -52 * zmax)


def incircle(a, b, c, p):
    """``(det, bound)`` of p [n, 2] against the counter-clockwise triangle (a, b, c): det > bound <=> strictly inside."""
    adx, ady, bdx, bdy, cdx, cdy = a[0] - p[:, 0], a[1] - p[:, 1], b[0] - p[:, 0], b[1] - p[:, 1], c[0] - p[:, 0], c[1] - p[:, 1]
    bdxcdy, cdxbdy, alift = bdx * cdy, cdx * bdy, adx * adx + ady * ady
    cdxady, adxcdy, blift = cdx * ady, adx * cdy, bdx * bdx + bdy * bdy
    adxbdy, bdxady, clift = adx * bdy, bdx * ady, cdx * cdx + cdy * cdy
    det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady)
    perm = (abs(bdxcdy) + abs(cdxbdy)) * alift + (abs(cdxady) + abs(adxcdy)) * blift + (abs(adxbdy) + abs(bdxady)) * clift
    return det, ICC_ERR * perm


def brute_force(unique, resolution=1.0):
    """``(tri [ny, nx, 3] int32 ascending, n_candidates [ny, nx])`` for a cloud of up to about 60 points: every triple with an
    area and an empty circumcircle is a Delaunay triangle; a node takes the one that contains it (on an edge counts).
    ``n_candidates`` is how many contain it: 1 in general position and off the edges, 0 outside the hull."""
    P, _ = shifted(unique)
    M = len(P)
    assert M <= 64
    qx, qy = nodes(unique, resolution)
    tris = []
    for i, j, k in itertools.combinations(range(M), 3):
        a, b, c = P[i], P[j], P[k]
        area = _cross(b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1])
        if area == 0:
            continue
        if area < 0:
            b, c = c, b
        det, bound = incircle(a, b, c, P)
        det[[i, j, k]] = 0.0
        if not (det > bound).any():
            tris.append((i, j, k))
    tris = np.array(tris, np.int64)
    a, b, c = P[tris[:, 0]], P[tris[:, 1]], P[tris[:, 2]]
    area = _cross(b[:, 0] - a[:, 0], b[:, 1] - a[:, 1], c[:, 0] - a[:, 0], c[:, 1] - a[:, 1])
    sign = np.sign(area)
    out = np.full((len(qy), len(qx), 3), -1, np.int32)
    count = np.zeros((len(qy), len(qx)), np.int32)
    for jj, y in enumerate(qy):
        for ii, x in enumerate(qx):
            w0 = _cross(b[:, 0] - x, b[:, 1] - y, c[:, 0] - x, c[:, 1] - y) * sign
            w1 = _cross(c[:, 0] - x, c[:, 1] - y, a[:, 0] - x, a[:, 1] - y) * sign
            w2 = _cross(a[:, 0] - x, a[:, 1] - y, b[:, 0] - x, b[:, 1] - y) * sign
            hit = np.flatnonzero((w0 >= 0) & (w1 >= 0) & (w2 >= 0))
            count[jj, ii] = len(hit)
            if len(hit):
                out[jj, ii] = tris[hit[0]]
    return out, count


def vertex_sets(unique, tri):
    """The triangles as sorted coordinate triples [ny, nx, 3, 2] (NaN where -1): equal <=> the same three points, whatever
    order the two clouds' rows are in."""
    u = np.asarray(unique, np.float64)
    tri = np.asarray(tri, np.int64)
    xy = u[:, :2][np.where(tri >= 0, tri, 0)]                    # [ny, nx, 3, 2]
    order = np.lexsort((xy[..., 1], xy[..., 0]), axis=-1)
    xy = np.take_along_axis(xy, order[..., None], axis=-2)
    xy[tri[..., 0] < 0] = np.nan
    return xy
