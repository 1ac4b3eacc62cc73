/* t2h_cloud.h -- C ABI of the device point-cloud building-wise metrics in libt2h_hip.so (csrc/dsm_cloud.hip): the label of
 * the pixel under every point of a raw cloud, the exact float64 median z of every building's points, and the RMSE-B / MAE-B /
 * MedAE-B aggregates of the reference's scripts/evaluator_instance.py:139-291 (evaluate_cloud_valid_only, evaluate_cloud_all).
 *
 * Same conventions as t2h.h and t2h_inst.h: device pointers owned by the caller, no allocation, no state, stream-ordered
 * calls, 0 or a negative T2H_ERR_* code, every argument validated before any launch.  The entries live in the same library
 * but are typed by tomosar2height_amd/cloud_instances.py (its own SIGNATURES table); T2H_ABI_VERSION is unchanged.
 *
 * Point counts and pixel counts are limited to 2^31 - 1.  Strides are in elements (doubles).
 */
#ifndef T2H_CLOUD_H_
#define T2H_CLOUD_H_

#include "t2h.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2H_CLOUD_TINY_MAX 64     /* segments up to this size: one wave each, ranked in registers */
#define T2H_CLOUD_SMALL_MAX 2048  /* segments up to this size: one workgroup each, sorted in 16 KB of LDS; above: radix select */
#define T2H_CLOUD_TABLE_COLS 8    /* n_valid, n_nan, sum |d|, sum d^2, median |d|, max |d|, n_covered, n_bad (all as doubles) */
#define T2H_CLOUD_MODE_VALID_ONLY 0  /* evaluate_cloud_valid_only: a building without points (or with a NaN) is dropped */
#define T2H_CLOUD_MODE_ALL 1         /* evaluate_cloud_all: np.nan_to_num on the height first, so such a building counts as 0 */

/* point_label[i] = labels[row, col] of the pixel under point i = (x, y) = (points[i * stride], points[i * stride + 1]):
 *   fx = (x * ra + y * rb) + rc,  fy = (x * rd + y * re) + rf      (every product and sum rounded on its own, in this order)
 *   col = clip(floor(fx), 0, C - 1),  row = clip(floor(fy), 0, R - 1)
 * (ra .. rf) are the coefficients of the INVERSE raster transform (world -> pixel).  The clip is applied in float64 before the
 * conversion to an integer: a point outside the raster lands on the border pixel, however far away it is.  A point whose x or y
 * is not finite, or whose fx or fy is a NaN (inf - inf), gets label 0 and is counted into *n_bad (device int32, overwritten).
 * labels [R, C] int32, contiguous; N = 0 is valid (only *n_bad = 0 is written); stride >= 2.
 * Replaces scripts/evaluator_instance.py:155-164 (associate_points_with_buildings). */
int t2h_cloud_assign(const double *points, int64_t N, int64_t stride, double ra, double rb, double rc, double rd, double re,
                     double rf, const int32_t *labels, int R, int C, int32_t *point_label, int32_t *n_bad, t2h_stream_t stream);

/* N points, K labels.  Linear in N and K: 256 + 12 * K + 8 * ceil(K / 1024) bytes of per-label tables, 12 * N bytes of
 * compacted (label, key) pairs, and (32 + 2 048) bytes for each of the at most N / (T2H_CLOUD_SMALL_MAX + 1) + 1 segments that
 * can be large (about 1 byte per point), each part rounded up to 256.  0 for a shape the entry would refuse. */
size_t t2h_cloud_medians_workspace_bytes(int64_t N, int K);

/* counts[k-1] = |{point_label == k}| and medians[k-1] = np.median(z[point_label == k]) for k = 1..K in float64, where
 * z[i] = z[i * stride] (stride >= 1; column 2 of a point list is z = points + 2).  Labels outside 1..K are background.  The
 * median is the exact order statistic on 64-bit keys: s[n/2] for odd n, (s[n/2 - 1] + s[n/2]) / 2 for even n, then + 0.0
 * (a zero median is +0, as numpy's mean has it); a segment that contains a NaN gives NaN, as does an empty one (count 0).
 * The result does not depend on the order of the points or on scheduling: two runs give the same bytes.  N = 0 is valid.
 * Replaces scripts/evaluator_instance.py:193-199. */
int t2h_cloud_medians(const double *z, int64_t stride, const int32_t *point_label, int64_t N, int K, int32_t *counts,
                      double *medians, void *workspace, size_t workspace_bytes, t2h_stream_t stream);

/* Over the K buildings: height[k] = pred_med[k] - (double)dtm_med[k] (written as it is, before any NaN handling), then
 *   mode T2H_CLOUD_MODE_VALID_ONLY: a building whose height or ref_med is a NaN is left out;
 *   mode T2H_CLOUD_MODE_ALL: h = np.nan_to_num(height) (NaN -> 0, +-inf -> +-DBL_MAX); a building whose ref_med is a NaN is
 *   left out;
 * d = (double)ref_med - h and table = { n_valid, n_nan = K - n_valid, sum |d|, sum d^2, median |d|, max |d|,
 * n_covered = |{counts > 0}|, n_bad = *n_bad (the device int32 of t2h_cloud_assign; may be null: 0) }.  One workgroup: float64
 * partial sums per thread in a fixed order, then a fixed tree; the median is an exact radix select.  K = 0 gives a zero table
 * (but for n_bad).
 * Replaces scripts/evaluator_instance.py:204-221 and 267-284. */
int t2h_cloud_metrics(const double *pred_med, const float *dtm_med, const float *ref_med, const int32_t *counts, int K, int mode,
                      const int32_t *n_bad, double *height, double *table, t2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2H_CLOUD_H_ */
