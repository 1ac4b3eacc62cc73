// Per-node state and predicates of the Delaunay-linear baseline (csrc/dsm_tin.hip).  Plain C++ that
// compiles for the host as well, so the search can be stepped through on a CPU build.  Everything here works on SHIFTED
// coordinates (X - xmin, Y - ymin); products and sums are separate roundings (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define T2H_TIN_HD __host__ __device__ inline
#else
#define T2H_TIN_HD inline
#endif

namespace t2h {

// (10 + 96 eps) eps and (3 + 16 eps) eps with eps = 2^-53: the first-stage bounds of Shewchuk's in-circle and orientation
// predicates ("Adaptive Precision Floating-Point Arithmetic and Fast Robust Geometric Predicates", 1997, section 4): a
// determinant evaluated as below, differences included, is off by at most the bound times its permanent.
constexpr double kTinEps = 0x1p-53;
constexpr double kTinIccErr = (10.0 + 96.0 * kTinEps) * kTinEps;
constexpr double kTinCcwErr = (3.0 + 16.0 * kTinEps) * kTinEps;

// cross(a - o, b - o): positive where o, a, b turn left
T2H_TIN_HD double tin_cross(double ox, double oy, double ax, double ay, double bx, double by) {
    return (ax - ox) * (by - oy) - (ay - oy) * (bx - ox);
}

// the in-circle determinant of p against the counter-clockwise triangle (a, b, c), positive inside; true where it exceeds its
// error bound: p is then strictly inside the circumcircle in exact arithmetic.  An exactly cocircular p never is.
T2H_TIN_HD bool tin_incircle(double ax, double ay, double bx, double by, double cx, double cy, double px, double py, double *det) {
    const double adx = ax - px, ady = ay - py, bdx = bx - px, bdy = by - py, cdx = cx - px, cdy = cy - py;
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy, alift = adx * adx + ady * ady;
    const double cdxady = cdx * ady, adxcdy = adx * cdy, blift = bdx * bdx + bdy * bdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady, clift = cdx * cdx + cdy * cdy;
    const double d = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady);
    const double permanent = (fabs(bdxcdy) + fabs(cdxbdy)) * alift + (fabs(cdxady) + fabs(adxcdy)) * blift +
                             (fabs(adxbdy) + fabs(bdxady)) * clift;
    *det = d;
    return d > kTinIccErr * permanent;
}

// What one raster node carries through the search.  Before `have`: the wedge of directions seen from q -- r is its clockwise
// end, l its counter-clockwise end, opening below 180 degrees (`flat`: exactly 180, q on the segment r l), `on` a point that
// coincides with q.  After: a counter-clockwise triangle (a, b, c) that contains q.  The wedge lives in the slots of a and b.
struct TinNode {
    double qx, qy;
    double ax, ay, bx, by, cx, cy;
    int ia, ib, ic;
    int n;              // points in the wedge (0, 1, 2 = two or more)
    int on;             // row of a point equal to q, or -1
    bool flat, have;
};

T2H_TIN_HD void tin_node_init(TinNode &s, double qx, double qy) {
    s.qx = qx; s.qy = qy;
    s.ax = s.ay = s.bx = s.by = s.cx = s.cy = 0.0;
    s.ia = s.ib = s.ic = -1;
    s.n = 0; s.on = -1; s.flat = false; s.have = false;
}

T2H_TIN_HD void tin_set(TinNode &s, double ax, double ay, int ia, double bx, double by, int ib, double cx, double cy, int ic) {
    s.ax = ax; s.ay = ay; s.ia = ia; s.bx = bx; s.by = by; s.ib = ib; s.cx = cx; s.cy = cy; s.ic = ic;
    s.have = true;
}

// Offer p to a node that has no triangle yet.  The first three points whose hull contains q make the triangle.
T2H_TIN_HD void tin_wedge(TinNode &s, double px, double py, int id) {
    const double qx = s.qx, qy = s.qy;
    if (px == qx && py == qy) {
        s.on = id;
    } else if (s.n == 0) {
        s.ax = s.bx = px; s.ay = s.by = py; s.ia = s.ib = id; s.n = 1;
    } else {
        const double cr = tin_cross(qx, qy, s.ax, s.ay, px, py), cl = tin_cross(qx, qy, s.bx, s.by, px, py);
        if (s.flat) {                                            // q lies on the segment r l: any point off that line closes it
            if (cr > 0.0) tin_set(s, s.ax, s.ay, s.ia, px, py, id, s.bx, s.by, s.ib);
            else if (cr < 0.0) tin_set(s, s.ax, s.ay, s.ia, s.bx, s.by, s.ib, px, py, id);
            return;
        }
        if (cr == 0.0 && cl == 0.0) {                            // on the line of a wedge without opening
            const double dot = (s.ax - qx) * (px - qx) + (s.ay - qy) * (py - qy);
            if (dot < 0.0) { s.bx = px; s.by = py; s.ib = id; s.flat = true; s.n = 2; }
        } else if (cr <= 0.0 && cl >= 0.0) {                     // in the opposite cone: r, l, p surround q
            tin_set(s, s.ax, s.ay, s.ia, s.bx, s.by, s.ib, px, py, id);
            return;
        } else if (cr > 0.0 && cl > 0.0) {                       // beyond l
            s.bx = px; s.by = py; s.ib = id; s.n = 2;
        } else if (cr < 0.0 && cl < 0.0) {                       // beyond r
            s.ax = px; s.ay = py; s.ia = id; s.n = 2;
        }
    }
    // q is itself a point of the cloud: with two directions that open, (q, r, l) is a triangle that has q as a corner
    if (s.on >= 0 && s.n == 2 && !s.flat && tin_cross(qx, qy, s.ax, s.ay, s.bx, s.by) > 0.0)
        tin_set(s, qx, qy, s.on, s.ax, s.ay, s.ia, s.bx, s.by, s.ib);
}

// Bring p (strictly inside the circumcircle) into the triangle: of (p, b, c), (a, p, c), (a, b, p) the one that still contains
// q and has an area.  With u_x = cross(x - p, q - p): (p, b, c) holds q where u_b >= 0 >= u_c, and cyclically.  A candidate for
// which both hold strictly is preferred (q on an edge of the old triangle leaves two).  False where rounding left none.
T2H_TIN_HD bool tin_pivot(TinNode &s, double px, double py, int id) {
    const double ua = tin_cross(px, py, s.ax, s.ay, s.qx, s.qy), ub = tin_cross(px, py, s.bx, s.by, s.qx, s.qy),
                 uc = tin_cross(px, py, s.cx, s.cy, s.qx, s.qy);
    const bool area_a = tin_cross(px, py, s.bx, s.by, s.cx, s.cy) > 0.0, area_b = tin_cross(s.ax, s.ay, px, py, s.cx, s.cy) > 0.0,
               area_c = tin_cross(s.ax, s.ay, s.bx, s.by, px, py) > 0.0;
    const bool ka = area_a && ub >= 0.0 && uc <= 0.0, kb = area_b && uc >= 0.0 && ua <= 0.0, kc = area_c && ua >= 0.0 && ub <= 0.0;
    int pick = -1;
    if (ka && ub > 0.0 && uc < 0.0) pick = 0;
    else if (kb && uc > 0.0 && ua < 0.0) pick = 1;
    else if (kc && ua > 0.0 && ub < 0.0) pick = 2;
    else if (ka) pick = 0;
    else if (kb) pick = 1;
    else if (kc) pick = 2;
    if (pick < 0) return false;
    if (pick == 0) { s.ax = px; s.ay = py; s.ia = id; }
    else if (pick == 1) { s.bx = px; s.by = py; s.ib = id; }
    else { s.cx = px; s.cy = py; s.ic = id; }
    return true;
}

// Offer p during the ring walk: the wedge first, afterwards a pivot on every point found inside the circumcircle.  Returns
// 1 where it pivoted.
T2H_TIN_HD int tin_offer(TinNode &s, double px, double py, int id) {
    if (!s.have) { tin_wedge(s, px, py, id); return 0; }
    if (id == s.ia || id == s.ib || id == s.ic) return 0;
    double det;
    if (!tin_incircle(s.ax, s.ay, s.bx, s.by, s.cx, s.cy, px, py, &det)) return 0;
    return tin_pivot(s, px, py, id) ? 1 : 0;
}

// (2 R)^2 of the circumcircle: every point inside it is within 2 R of q.  Infinite for a triangle without area.
T2H_TIN_HD double tin_diameter2(const TinNode &s) {
    const double cr = tin_cross(s.ax, s.ay, s.bx, s.by, s.cx, s.cy);
    const double ab = (s.bx - s.ax) * (s.bx - s.ax) + (s.by - s.ay) * (s.by - s.ay);
    const double bc = (s.cx - s.bx) * (s.cx - s.bx) + (s.cy - s.by) * (s.cy - s.by);
    const double ca = (s.ax - s.cx) * (s.ax - s.cx) + (s.ay - s.cy) * (s.ay - s.cy);
    return cr > 0.0 ? ab * bc * ca / (cr * cr) : INFINITY;
}

// A box (x0, x1, y0, y1) that holds the circumcircle, widened by 2^-20 of its radius; false where the triangle is too thin for
// the centre to be placed that well (sine of its sharpest angle below about 2^-24): the caller then scans every cell.
T2H_TIN_HD bool tin_circle_box(const TinNode &s, double *x0, double *x1, double *y0, double *y1) {
    const double bax = s.bx - s.ax, bay = s.by - s.ay, cax = s.cx - s.ax, cay = s.cy - s.ay;
    const double bl = bax * bax + bay * bay, cl = cax * cax + cay * cay, cr = bax * cay - bay * cax;
    if (!(cr * cr > 0x1p-48 * bl * cl)) return false;
    const double d = 2.0 * cr, ux = (cay * bl - bay * cl) / d, uy = (bax * cl - cax * bl) / d;
    const double r = sqrt(ux * ux + uy * uy) * (1.0 + 0x1p-20);
    if (!isfinite(r)) return false;
    *x0 = s.ax + ux - r; *x1 = s.ax + ux + r; *y0 = s.ay + uy - r; *y1 = s.ay + uy + r;
    return true;
}

// The triangle's rows in ascending order (a <= b <= c afterwards; orientation is no longer counter-clockwise)
T2H_TIN_HD void tin_sort_rows(TinNode &s) {
#define T2H_TIN_SWAP(X, Y)                                                                                                    \
    if (s.i##X > s.i##Y) {                                                                                                    \
        const int ti = s.i##X; s.i##X = s.i##Y; s.i##Y = ti;                                                                  \
        double t = s.X##x; s.X##x = s.Y##x; s.Y##x = t;                                                                       \
        t = s.X##y; s.X##y = s.Y##y; s.Y##y = t;                                                                              \
    }
    T2H_TIN_SWAP(a, b) T2H_TIN_SWAP(b, c) T2H_TIN_SWAP(a, b)
#undef T2H_TIN_SWAP
}

// lambda_0 = cross(b - q, c - q) / cross(b - a, c - a), lambda_1 = cross(c - q, a - q) / the same, lambda_2 = cross(a - q, b - q)
// / the same: each difference, product and quotient rounded once, in this order
T2H_TIN_HD void tin_bary(const TinNode &s, double *l0, double *l1, double *l2) {
    const double area = tin_cross(s.ax, s.ay, s.bx, s.by, s.cx, s.cy);
    *l0 = tin_cross(s.qx, s.qy, s.bx, s.by, s.cx, s.cy) / area;
    *l1 = tin_cross(s.qx, s.qy, s.cx, s.cy, s.ax, s.ay) / area;
    *l2 = tin_cross(s.qx, s.qy, s.ax, s.ay, s.bx, s.by) / area;
}

}  // namespace t2h
