/* t2h_interp.h -- C ABI of the device interpolation baselines in libt2h_hip.so (csrc/dsm_interp.hip): bounds of a float64
 * cloud, a uniform cell index with the z-max de-duplication of equal (X, Y), exact k nearest neighbours of every node of a
 * regular grid, and the nearest / inverse-distance-weighted rasters of the reference's scripts/interpolate_nearest.py and
 * scripts/interpolate_idw.py.
 *
 * Same conventions as t2h.h, t2h_eval.h and t2h_inst.h: device pointers owned by the caller, no allocation, no state,
 * stream-ordered calls, 0 or a negative T2H_ERR_* code, every argument validated before any launch.  The entries live in the
 * same library but are typed by tomosar2height_amd/interpolate.py (its own SIGNATURES table); T2H_ABI_VERSION is unchanged.
 *
 * Points are rows of (X, Y, Z) float64.  A point's index is an int32: 1 <= N <= 2^31 - 1.
 */
#ifndef T2H_INTERP_H_
#define T2H_INTERP_H_

#include "t2h.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2H_INTERP_TILE 16         /* edge of the square pixel tile one workgroup searches (one pixel per thread) */
#define T2H_INTERP_CHUNK 2048      /* points staged in LDS at a time: 16 B of coordinates + 4 B of index each = 40 KB */
#define T2H_INTERP_MAX_K 8         /* neighbours kept in registers per pixel */
#define T2H_INTERP_CELL_POINTS 4   /* the cell edge h aims at this many INPUT points per cell on average */
#define T2H_INTERP_TABLE_COLS 16   /* xmin, xmax, ymin, ymax, n_nonfinite, h, gx, gy, M, 0 ... (all as doubles) */

/* Cells the index of an N-point cloud can have at most, N / 2 + 8 (0 for an N the entries refuse): cell_offsets holds one
 * more int32 than this. */
int64_t t2h_interp_max_cells(int64_t N);

/* 40 * 1024 bytes of partial rows. */
size_t t2h_interp_bounds_workspace_bytes(int64_t N);

/* table[0..4] = min X, max X, min Y, max Y over the rows whose three values are all finite, and the number of rows that
 * have a non-finite value (such rows are left out of everything below).  table[5..7] = the cell grid derived from them:
 *   h  = max( sqrt(T2H_INTERP_CELL_POINTS * (xmax - xmin) * (ymax - ymin) / N),
 *             2 * T2H_INTERP_CELL_POINTS * max(xmax - xmin, ymax - ymin) / N ),   1 where that is 0,
 *   gx = floor((xmax - xmin) / h) + 1, gy likewise: gx * gy <= t2h_interp_max_cells(N) (h is doubled until it holds).
 * table[8..15] = 0.  Min and max do not depend on order: two runs give the same bytes. */
int t2h_interp_bounds(const double *points, int64_t N, double *table, void *workspace, size_t workspace_bytes,
                      t2h_stream_t stream);

/* 52 * N bytes of point copies and scan positions + 4 bytes per possible cell + scan partials, each part rounded up to 256.
 * 0 for an N the entry would refuse. */
size_t t2h_interp_index_workspace_bytes(int64_t N);

/* The index of the cloud over the cell grid of `table` (as t2h_interp_bounds left it, read on the device).
 * Point (X, Y) belongs to cell (min(floor((X - xmin) / h), gx - 1), min(floor((Y - ymin) / h), gy - 1)): points on xmax or
 * ymax are clamped into the last cell.  Cells are numbered row-major, cy * gx + cx.  Inside a cell the points are ordered
 * by (X, Y, -Z) and every run of equal (X, Y) collapses to its first element: the reference's
 * df.groupby(['X', 'Y']).max().  unique [N, 3] float64 receives the M surviving rows in cell-major order (rows M .. N - 1 are
 * not written), cell_offsets [t2h_interp_max_cells(N) + 1] int32 the start of every cell in it (cells past gx * gy - 1 start
 * at M), table[8] = M.  The result does not depend on scheduling: two runs give the same bytes. */
int t2h_interp_index(const double *points, int64_t N, double *table, double *unique, int32_t *cell_offsets, void *workspace,
                     size_t workspace_bytes, t2h_stream_t stream);

/* The three grid entries share their first arguments: the unique cloud and cell offsets of t2h_interp_index, M, the cell
 * grid (xmin, ymin, h, gx, gy: the values of the table, now passed from the host), the raster (node (j, i) at
 * (i * res + xmin, j * res + ymin), ny rows by nx columns, 1 <= ny * nx <= 2^31 - 1) and 1 <= k <= min(M, T2H_INTERP_MAX_K).
 * Candidates are ordered by (d2, X, Y) ascending with d2 = dx * dx + dy * dy (two products, one sum, no fused multiply-add).
 * One workgroup per tile of 16 x 16 nodes; neighbour lists live in registers.
 *
 * t2h_interp_knn: d2 [ny, nx, k] float64 and idx [ny, nx, k] int32 (rows of unique). */
int t2h_interp_knn(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                   int gy, double res, int ny, int nx, int k, double *d2, int32_t *idx, t2h_stream_t stream);

/* out [ny, nx] float64 = Z of the nearest unique point.  Replaces scripts/interpolate_nearest.py:32-36. */
int t2h_interp_nearest(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                       int gy, double res, int ny, int nx, double *out, t2h_stream_t stream);

/* out [ny, nx] float64 = inverse-distance weighting (power 2) over the k nearest: dist = sqrt(d2); w = 1 where dist == 0,
 * else 1 / (dist * dist); s = the sum of w in rank order; out = the sum of (w / s) * Z in rank order.  Correctly rounded
 * sqrt and divisions.  Replaces scripts/interpolate_idw.py:9-27. */
int t2h_interp_idw(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                   int gy, double res, int ny, int nx, int k, double *out, t2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2H_INTERP_H_ */
