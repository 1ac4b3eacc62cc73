/* t2h_tin.h -- C ABI of the Delaunay-linear baseline in libt2h_hip.so (csrc/dsm_tin.hip): the convex hull of the unique cloud
 * of t2h_interp_index, and for every node of a regular grid the one Delaunay triangle of that cloud which contains it, with
 * its barycentric coordinates or the height interpolated over it -- scipy.interpolate.griddata(method='linear') of the
 * reference's scripts/interpolate_bilinear.py, on the cloud shifted to its (xmin, ymin).  No triangulation is built: the
 * triangle of a node is found by a local search over the cell index.
 *
 * Same conventions as t2h.h and t2h_interp.h: device pointers owned by the caller, no allocation, no state, stream-ordered
 * calls, 0 or a negative T2H_ERR_* code, every argument validated before any launch.  The entries live in the same library
 * but are typed by tomosar2height_amd/interpolate.py (its own TIN_SIGNATURES table); T2H_ABI_VERSION is unchanged.
 *
 * Every predicate is evaluated on SHIFTED coordinates (X - xmin, Y - ymin), each rounded once, in float64 without fused
 * multiply-add.
 */
#ifndef T2H_TIN_H_
#define T2H_TIN_H_

#include "t2h_interp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2H_TIN_DIRECTIONS 16      /* fan of directions whose extreme points make the polygon of the hull's first filter */
#define T2H_TIN_MAX_PIVOTS 64      /* pivots of one node's verification before it gives up (counted in the status) */
#define T2H_TIN_STATUS_COLS 8      /* int32 words of a status table */
/* hull status: */
#define T2H_TIN_HULL_COUNT 0       /* vertices of the hull */
#define T2H_TIN_HULL_DEGENERATE 1  /* 1: fewer than 3 distinct points, or all on one line (hull holds nothing then) */
#define T2H_TIN_HULL_SURVIVORS 2   /* points the polygon filter left for the sort */
/* search status: */
#define T2H_TIN_CAPPED 0           /* nodes that reached T2H_TIN_MAX_PIVOTS, or whose pivot found no triangle to go to */
#define T2H_TIN_UNRESOLVED 1       /* nodes inside the hull for which no three points around them were found (NaN, -1) */
#define T2H_TIN_PIVOTS 2           /* pivots of the verification, all nodes */
#define T2H_TIN_WALK_PIVOTS 3      /* pivots during the ring walk, all nodes */

/* 8 * M bytes (the survivors, padded to a power of two) + the partial extremes + 512: 0 for an M the entry would refuse. */
size_t t2h_tin_hull_workspace_bytes(int64_t M);

/* The convex hull of unique [M, 3] (rows of t2h_interp_index; M >= 1), counter-clockwise from its smallest (X, Y), points on
 * an edge left out: hull [M + 1] int32 receives status[T2H_TIN_HULL_COUNT] rows of `unique` (the rest is scratch),
 * status [T2H_TIN_STATUS_COLS] int32 the table above.  Extremes along T2H_TIN_DIRECTIONS directions give an inscribed
 * polygon; points strictly inside it (beyond the error bound of the orientation) are discarded; one workgroup sorts the rest
 * by (X, Y) and runs a monotone chain on them.  The result does not depend on scheduling: two runs give the same bytes. */
int t2h_tin_hull(const double *unique, int M, double xmin, double ymin, int32_t *hull, int32_t *status, void *workspace,
                 size_t workspace_bytes, t2h_stream_t stream);

/* The two search entries share their first arguments with t2h_interp_knn (the unique cloud, its cell offsets, M >= 3, the cell
 * grid, the raster) followed by the hull (n_hull >= 3 rows of `unique`, as t2h_tin_hull left them).  One workgroup per tile of
 * 16 x 16 nodes, one node per thread.  A node q = (i * res + xmin) - xmin, likewise y, is OUTSIDE where the cross product
 * (h1 - h0) x (q - h0) of some hull edge is negative (on an edge counts as inside).  Inside, the search returns the triangle
 * (a, b, c) of cloud points that contains q and whose circumcircle holds no other point strictly inside -- strictly: the
 * in-circle determinant must exceed its float64 error bound, an exactly cocircular point does not count.
 * status [T2H_TIN_STATUS_COLS] int32 is cleared and filled as above.
 *
 * t2h_tin_simplex: tri [ny, nx, 3] int32 = the triangle's rows of `unique` in ascending order (-1 outside the hull) and
 * bary [ny, nx, 3] float64 = for those rows a, b, c in that order
 *   cross(b - q, c - q) / cross(b - a, c - a), cross(c - q, a - q) / cross(b - a, c - a), cross(a - q, b - q) / cross(b - a, c - a)
 * with cross(u, v) = u.x * v.y - u.y * v.x, every difference, product and quotient rounded once (NaN outside the hull). */
int t2h_tin_simplex(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                    int gy, double res, int ny, int nx, const int32_t *hull, int n_hull, int32_t *tri, double *bary,
                    int32_t *status, t2h_stream_t stream);

/* out [ny, nx] float64 = (bary_0 * Z_a + bary_1 * Z_b) + bary_2 * Z_c of the same search, NaN outside the hull: griddata's
 * fill_value.  Replaces scripts/interpolate_bilinear.py:33-38 on shifted coordinates. */
int t2h_tin_linear(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                   int gy, double res, int ny, int nx, const int32_t *hull, int n_hull, double *out, int32_t *status,
                   t2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2H_TIN_H_ */
