"""The resamplers of csrc/bicubic.hip, csrc/raster.hip and csrc/grid_fused.hip restated in float64 as 1-D interpolation matrices,
their derived error bars, and the cases of tests/test_resample_cpu.py and tests/test_resample_gpu.py.

Formulas.  Every resampler here is separable.  An output index o of an axis reads the source coordinate r(o) = s o with
s = (n_in - 1) / (n_out - 1) (align_corners=True; s = 0 when n_out = 1); a point p of the samplers reads r = p (n_in - 1).  With
f = floor(r), t = r - f the taps f - 1 .. f + 2 weigh cc2(t + 1), cc1(t), cc1(1 - t), cc2(2 - t) (bicubic, ATen's cubic convolution,
A = -0.75: cc1(x) = ((A + 2) x - (A + 3)) x x + 1 on [0, 1], cc2(x) = ((A x - 5 A) x + 8 A) x - 4 A on [1, 2]) or the taps f, f + 1
weigh 1 - t, t (bilinear).  A tap outside [0, n_in - 1] is clamped to the border pixel, and its weight ADDS into that pixel's entry:
row o of the matrix ``Ay [n_out, n_in]`` is the weight of every source pixel in output o.  Then

    forward  = Ay . X . Ax^T          adjoint = Ay^T . G . Ax

and for the point samplers the rows are per point: out[n, c] = sum_pq Wy[n, p] Wx[n, q] plane[c, p, q], and the adjoint scatters
g[n, c] Wy[n, p] Wx[n, q].  'nearest' clips r to [0, n_in - 1] and rounds half to even (grid_sampler_2d's nearbyint).

Bars.  u = 2^-24 (``U``), gamma_n = n u / (1 - n u).  The bar of an element has three parts, evaluated elementwise in float64; the
first two bound the entrywise error of the weights the kernel computes, |Ay_computed - Ay| <= D, the third the rounded sums.

1.  Source coordinate.  The resamplers form r^ = fl(fl(s) o): two roundings, |r^ - r| <= (2 u + u^2) r.  The samplers form
    r^ = fl(p (n_in - 1)) from the float32 p and the exact integer: one rounding, |r^ - r| <= u |r|.  f^ = floor(r^) and
    t^ = r^ - f^ are exact.  As a function of the coordinate the weight of source offset d = r - j is W(d), continuous, piecewise
    cubic, with |W'| <= max|cc1'| = 1.35 (cc1' = 3.75 x^2 - 4.5 x, extreme at x = 0.6) on the inner taps and <= max|cc2'| = 0.75
    (cc2' = A (3 x - 4)(x - 2), extreme at x = 1) on the outer taps; for bilinear |W'| = 1.  So every tap's weight moves by at most
    Lip |r^ - r|.  When [r - e, r + e] contains an integer the kernel may use the neighbouring window: the bound then takes all the
    taps of both windows with Lip = 1.35.  ``T`` counts, per source pixel, the taps (of that possibly widened window) that clamp
    to it; part 1 is Lip e T.
2.  The coefficients in float32.  Arguments: t^ is exact; 1 - t^ rounds by <= u / 2, t^ + 1 and 2 - t^ (in [1, 2]) by <= u, which the
    Lipschitz constants turn into 0.675 u and 0.75 u.  Horner forms, every operation rounded once (a fused multiply-add rounds
    less), absolute errors accumulated with the exact ranges of the intermediates:
      cc1 on [0, 1]:  1.25 x [<= 1.25 u]; - 2.25, in [-2.25, -1] [3.5 u]; . x, |.| <= 2.25 [5.75 u]; . x, |.| <= 1 [6.75 u];
                      + 1, in [0, 1] [7.75 u]; with the argument 8.43 u:                                             E1 = 9 u
      cc2 on [1, 2]:  -0.75 x, |.| <= 1.5 [1.5 u]; + 3.75, in [2.25, 3] [4.5 u]; . x, |.| <= 4.5 [13.5 u]; - 6, in [-3, -1.5]
                      [16.5 u]; . x, |.| <= 3.12 [36.12 u]; + 3, in [-0.112, 0] [36.24 u]; with the argument 36.99 u: E2 = 37 u
    that is 4 u and 8.3 u times the largest intermediate (2.25 and 4.5).  Bilinear: l1 = t^ is exact, l0 = fl(1 - t^) is off by
    <= u / 2; E = u / 2 is taken for both taps.
    D = Lip e T + E (E placed on the taps like the weights), P = |A| + D bounds the computed weights in absolute value.
3.  The rounded sums.  n rounded operations on the path of any term, in any order, stay within gamma_n sum|terms|.  Forward
    bicubic: 16 products plus 4 + 4 (the row sums' and the column sum's products and additions), n = 24, and 25 with an addend.
    Forward bilinear: 4 products plus 2 + 2, n = 8, and 9 with an addend.  Gather adjoints: element (p, q) collects
    m = my[p] mx[q] terms, my the column sum of T; summing up to four coefficients into one weight per axis, two products and the
    m additions make n = m + 8.  Atomic scatters (samplers): m = sum_n Ty[n, p] Tx[n, q] additions in any order and two
    products, n = m + 2; 'nearest' adds the m values of a pixel with no product, n = m.

    forward bar  = (Py |X| Px^T - |Ay| |X| |Ax|^T) + gamma_n (Py |X| Px^T + |addend|)
    adjoint bar  = (Py^T |G| Px - |Ay|^T |G| |Ax|) + gamma_n (Py^T |G| Px)              (n elementwise)

Every function takes ``u``: with u = 2^-53 the same bars hold for a float64 implementation of the same operations, which is how
the restatement itself is checked against ``F.interpolate`` and ``F.grid_sample`` in float64 (tests/test_resample_cpu.py).
"""
import zlib

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
A = -0.75
LIP = {"cubic": (0.75, 1.35, 1.35, 0.75), "linear": (1.0, 1.0)}
EVAL = {"cubic": (37.0, 9.0, 9.0, 37.0), "linear": (0.5, 0.5)}          # in units of u
FIRST = {"cubic": -1, "linear": 0}                                      # first tap relative to floor(r)

# (h, w, H, W): every plane pair of the upsample tests; B = 2 and C in CHANNELS
SHAPES = (
    (1, 1, 2, 2), (1, 2, 2, 4), (2, 1, 4, 2), (2, 2, 4, 4),          # fewer than four pixels: every tap clamped somewhere
    (3, 5, 6, 10), (4, 4, 4, 4), (5, 3, 9, 5),                       # rectangular x 2; H == h (scale 1); scale exactly 1 / 2
    (7, 3, 19, 5),
    (9, 6, 3, 2), (5, 7, 1, 1), (2, 3, 1, 6),                        # H < h (scale above 1); H == 1 (scale 0)
    (16, 16, 40, 32),
    (33, 17, 66, 34),
)
B = 2
CHANNELS = (1, 5, 70)
BILINEAR_NHWC_CHANNELS = (4, 12, 68)        # t2h_upsample_bilinear_nhwc_* takes C % 4 == 0 only (include/t2h.h)
N_POINTS = 37
# (r, C, dim, N)
POINT_CASES = tuple((r, c, dim, N_POINTS) for r in (1, 2, 3, 5, 9, 16) for c in CHANNELS for dim in (2, 3)) + ((5, 5, 3, 0),)
TIES = {5: ((0.125, 0.625), (0.375, 0.875), (0.625, 0.125), (0.875, 0.375)),
        9: ((1 / 16, 9 / 16), (3 / 16, 15 / 16), (7 / 16, 5 / 16), (11 / 16, 13 / 16))}
OUTSIDE = ((-0.3, 0.2), (1.4, 1.0))
BELOW_ONE = float(np.float32(1.0) - np.float32(2.0 ** -24))


def gamma(n, u=U):
    n = np.asarray(n, np.float64)
    assert float(n.max(initial=0.0)) * u < 0.01
    return n * u / (1.0 - n * u)


def cc1(x, a=A):
    return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0


def cc2(x, a=A):
    return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a


def tap_weights(t, kind, a=A):
    """[len(t), taps] weights of the taps FIRST[kind] .. relative to floor(r), from the fraction t in [0, 1)."""
    if kind == "cubic":
        return np.stack([cc2(t + 1.0, a), cc1(t, a), cc1(1.0 - t, a), cc2(2.0 - t, a)], axis=1)
    return np.stack([1.0 - t, t], axis=1)


def source_coords(n_in, n_out, align_corners=True):
    o = np.arange(n_out, dtype=np.float64)
    if align_corners:
        return o * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    return (o + 0.5) * (n_in / n_out) - 0.5          # (the mutant: ATen's half-pixel index, unclamped as for cubic)


def rows(src, n_in, kind, a=A, clamp=True):
    """Dense float64 [len(src), n_in]: row i holds the weight of every source pixel at the source coordinate src[i]."""
    src = np.asarray(src, np.float64)
    f = np.floor(src)
    w = tap_weights(src - f, kind, a)
    m = np.zeros((src.shape[0], n_in))
    for k in range(w.shape[1]):
        tap = f.astype(np.int64) + FIRST[kind] + k
        inside = (tap >= 0) & (tap <= n_in - 1)
        keep = np.ones_like(inside) if clamp else inside          # (clamp=False: the zero-padding mutant)
        np.add.at(m, (np.nonzero(keep)[0], np.clip(tap, 0, n_in - 1)[keep]), w[keep, k])
    return m


def cubic_matrix(n_in, n_out, a=A, clamp=True, align_corners=True):
    return rows(source_coords(n_in, n_out, align_corners), n_in, "cubic", a, clamp)


def bilinear_matrix(n_in, n_out):
    return rows(source_coords(n_in, n_out), n_in, "linear")


def rows_bound(src, n_in, kind, rel, u=U):
    """(P, T) of the module docstring for coordinates known to |r^ - r| <= rel |r|: P [len(src), n_in] bounds the absolute value
    of every weight the float32 code can compute, T counts the taps that reach each pixel."""
    src = np.asarray(src, np.float64)
    e = rel * np.abs(src)
    lo, hi = np.floor(src - e).astype(np.int64), np.floor(src + e).astype(np.int64)
    taps = len(LIP[kind])
    d = np.zeros((src.shape[0], n_in))
    t = np.zeros((src.shape[0], n_in))
    for i in range(src.shape[0]):
        for k, tap in enumerate(range(lo[i] + FIRST[kind], hi[i] + FIRST[kind] + taps)):
            same = lo[i] == hi[i]
            lip = LIP[kind][k] if same else max(LIP[kind])
            ev = EVAL[kind][k] if same else max(EVAL[kind])
            p = min(max(tap, 0), n_in - 1)
            d[i, p] += lip * e[i] + ev * u
            t[i, p] += 1.0
    return np.abs(rows(src, n_in, kind)) + d, t


def matrix_bound(n_in, n_out, kind, u=U):
    return rows_bound(source_coords(n_in, n_out), n_in, kind, 2.0 * u + u * u, u)


# ------------------------------------------------------------------------------------------------ plane resamplers
def upsample(x, ay, ax):
    """[B, C, h, w] -> [B, C, H, W]: Ay . X . Ax^T per plane."""
    return ay @ np.asarray(x, np.float64) @ ax.T


def upsample_adjoint(g, ay, ax):
    """[B, C, H, W] -> [B, C, h, w]: Ay^T . G . Ax per plane."""
    return ay.T @ np.asarray(g, np.float64) @ ax


def upsample_abs(x, ay, ax):
    return upsample(np.abs(np.asarray(x, np.float64)), np.abs(ay), np.abs(ax))


def upsample_adjoint_abs(g, ay, ax):
    return upsample_adjoint(np.abs(np.asarray(g, np.float64)), np.abs(ay), np.abs(ax))


FORWARD_TERMS = {"cubic": 24, "linear": 8}


def upsample_bar(x, shape, kind, addend=None, u=U):
    h, w, hh, ww = shape
    (py, _), (px, _) = matrix_bound(h, hh, kind, u), matrix_bound(w, ww, kind, u)
    exact = upsample_abs(x, rows(source_coords(h, hh), h, kind), rows(source_coords(w, ww), w, kind))
    reach = upsample_abs(x, py, px)
    if addend is None:
        return (reach - exact) + gamma(FORWARD_TERMS[kind], u) * reach
    return (reach - exact) + gamma(FORWARD_TERMS[kind] + 1, u) * (reach + np.abs(np.asarray(addend, np.float64)))


def upsample_adjoint_bar(g, shape, kind, u=U):
    h, w, hh, ww = shape
    (py, ty), (px, tx) = matrix_bound(h, hh, kind, u), matrix_bound(w, ww, kind, u)
    exact = upsample_adjoint_abs(g, rows(source_coords(h, hh), h, kind), rows(source_coords(w, ww), w, kind))
    reach = upsample_adjoint_abs(g, py, px)
    m = np.outer(ty.sum(axis=0), tx.sum(axis=0))
    return (reach - exact) + gamma(m + 8, u) * reach


def adjoint_window_short(ay):
    """The mutant of a gather window one pixel short at its far end: every source pixel loses its last contributing output."""
    out = ay.copy()
    for p in range(ay.shape[1]):
        hit = np.nonzero(ay[:, p])[0]
        if hit.size:
            out[hit[-1], p] = 0.0
    return out


# ------------------------------------------------------------------------------------------------ point samplers
def point_coords(pts, r, swap=False):
    """(x, y) float64 [B, N] pixel coordinates of float32 points [B, N, dim]: p (r - 1), exact in float64."""
    assert pts.dtype == np.float32
    p = pts.astype(np.float64) * (r - 1)
    return (p[..., 1], p[..., 0]) if swap else (p[..., 0], p[..., 1])


def _point_rows(pts, r, make):
    sx, sy = point_coords(pts, r)
    return [(make(sy[b]), make(sx[b])) for b in range(pts.shape[0])]


def sample_bicubic(plane, pts, a=A, clamp=True, swap=False):
    """plane [B, C, r, r], pts float32 [B, N, dim] -> [B, N, C] float64."""
    plane = np.asarray(plane, np.float64)
    r = plane.shape[2]
    sx, sy = point_coords(pts, r, swap)
    return np.stack([np.einsum("np,nq,cpq->nc", rows(sy[b], r, "cubic", a, clamp), rows(sx[b], r, "cubic", a, clamp), plane[b])
                     for b in range(plane.shape[0])])


def sample_bicubic_adjoint(g, pts, r):
    """g [B, N, C] -> plane gradient [B, C, r, r] float64."""
    g = np.asarray(g, np.float64)
    return np.stack([np.einsum("np,nq,nc->cpq", wy, wx, g[b]) for b, (wy, wx) in
                     enumerate(_point_rows(pts, r, lambda s: rows(s, r, "cubic")))])


def sample_bicubic_bar(plane, pts, u=U):
    plane = np.abs(np.asarray(plane, np.float64))
    r = plane.shape[2]
    exact = _point_rows(pts, r, lambda s: np.abs(rows(s, r, "cubic")))
    bound = _point_rows(pts, r, lambda s: rows_bound(s, r, "cubic", u, u)[0])
    out = []
    for b in range(plane.shape[0]):
        reach = np.einsum("np,nq,cpq->nc", bound[b][0], bound[b][1], plane[b])
        out.append((reach - np.einsum("np,nq,cpq->nc", exact[b][0], exact[b][1], plane[b])) + gamma(24, u) * reach)
    return np.stack(out)


def sample_bicubic_adjoint_bar(g, pts, r, u=U):
    """(bar [B, C, r, r], additions into every plane element [B, r, r])."""
    g = np.abs(np.asarray(g, np.float64))
    exact = _point_rows(pts, r, lambda s: np.abs(rows(s, r, "cubic")))
    bound = _point_rows(pts, r, lambda s: rows_bound(s, r, "cubic", u, u))
    bars, counts = [], []
    for b in range(g.shape[0]):
        (py, ty), (px, tx) = bound[b]
        reach = np.einsum("np,nq,nc->cpq", py, px, g[b])
        m = np.einsum("np,nq->pq", ty, tx)
        bars.append((reach - np.einsum("np,nq,nc->cpq", exact[b][0], exact[b][1], g[b])) + gamma(m + 2, u)[None] * reach)
        counts.append(m)
    return np.stack(bars), np.stack(counts)


def nearest_index(pts, r, ties="even", clip=True, swap=False):
    """(iy, ix, inside) int64 / bool [B, N]: the pixel 'nearest' selects.  ``ties='away'`` and ``clip=False`` are the mutants; without
    the clip an index outside the plane reads zero (``inside`` False) the way zero padding would."""
    sx, sy = point_coords(pts, r, swap)
    out = []
    for s in (sy, sx):
        if clip:
            s = np.clip(s, 0.0, r - 1.0)
        out.append((np.rint(s) if ties == "even" else np.sign(s) * np.floor(np.abs(s) + 0.5)).astype(np.int64))
    inside = (out[0] >= 0) & (out[0] <= r - 1) & (out[1] >= 0) & (out[1] <= r - 1)
    return np.clip(out[0], 0, r - 1), np.clip(out[1], 0, r - 1), inside


def sample_nearest(plane, pts, **mutant):
    """plane [B, C, r, r] -> [B, N, C], the selected elements themselves (dtype kept)."""
    plane = np.asarray(plane)
    iy, ix, inside = nearest_index(pts, plane.shape[2], **mutant)
    return np.stack([plane[b][:, iy[b], ix[b]].T * inside[b][:, None].astype(plane.dtype) for b in range(plane.shape[0])])


def sample_nearest_adjoint(g, pts, r):
    """(plane gradient [B, C, r, r] float64, sum|terms| of the same shape, points per pixel [B, r, r])."""
    g = np.asarray(g, np.float64)
    iy, ix, _ = nearest_index(pts, r)
    b_n, n, c = g.shape
    grad, mag, count = np.zeros((b_n, c, r, r)), np.zeros((b_n, c, r, r)), np.zeros((b_n, r, r))
    for b in range(b_n):
        for i in range(n):
            grad[b, :, iy[b, i], ix[b, i]] += g[b, i]
            mag[b, :, iy[b, i], ix[b, i]] += np.abs(g[b, i])
            count[b, iy[b, i], ix[b, i]] += 1
    return grad, mag, count


def is_tie(pts, r):
    """[B, N, 2] bool: the coordinate p (r - 1), clipped, lies exactly half way between two pixels."""
    sx, sy = point_coords(pts, r)
    s = np.clip(np.stack([sx, sy], axis=-1), 0.0, r - 1.0)
    return s - np.floor(s) == 0.5


# ------------------------------------------------------------------------------------------------ cases
def _rng(key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def case(shape, channels):
    """(x [B, C, h, w], g [B, C, H, W], addend [B, C, H, W]) float32 of an upsample shape, seeded by the shape."""
    h, w, hh, ww = shape
    rng = _rng(("upsample", shape, channels))
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((B, channels, h, w), (B, channels, hh, ww), (B, channels, hh, ww)))


def points(r, dim, n):
    """float32 [B, n, dim]: the four corners, pixel centres, the exact ties of r = 5 and r = 9, two points outside [0, 1], 1 - 2^-24,
    odd multiples of 2^-8 (p (r - 1) is exact in float32 for every r here and never a tie) and uniform points of [-0.1, 1.1]; the
    second sample holds the same list in another order with other random points.  Columns past the second are not coordinates."""
    rng = _rng(("points", r, dim, n))
    if n == 0:
        return np.zeros((B, 0, dim), np.float32)
    q = max(r - 1, 1)
    fixed = [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)]
    fixed += [(min(i, q) / q, min(j, q) / q) for i, j in ((1, 1), (1, 2), (2, 1), (q - 1, q - 1))]
    fixed += [p for key in sorted(TIES) for p in TIES[key]]
    fixed += list(OUTSIDE) + [(BELOW_ONE, BELOW_ONE), (BELOW_ONE, 0.0)]
    out = np.zeros((B, n, dim), np.float32)
    for b in range(B):
        dyadic = (2 * rng.integers(0, 128, size=(8, 2)) + 1) / 256.0
        free = rng.uniform(-0.1, 1.1, size=(n - len(fixed) - 8, 2))
        xy = np.concatenate([np.asarray(fixed, np.float64), dyadic, free]).astype(np.float32)
        out[b, :, :2] = xy if b == 0 else xy[rng.permutation(n)]
        out[b, :, 2:] = rng.uniform(0.0, 1.0, size=(n, dim - 2)).astype(np.float32)
    return out


def point_case(case_):
    """(plane [B, C, r, r], pts [B, N, dim], g [B, N, C]) float32 of a POINT_CASES entry."""
    r, c, dim, n = case_
    rng = _rng(("point-case", case_))
    plane = rng.standard_normal((B, c, r, r)).astype(np.float32)
    return plane, points(r, dim, n), rng.standard_normal((B, n, c)).astype(np.float32)


def worst_ratio(got, want, bar):
    """max |got - want| / bar over the elements (0 / 0 counts as 0; anything above a zero bar as inf)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bar)
    return float(np.nanmax(ratio)) if not np.isnan(err).any() else float("inf")
