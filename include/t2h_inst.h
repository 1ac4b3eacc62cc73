/* t2h_inst.h -- C ABI of the device building-instance metrics in libt2h_hip.so (csrc/dsm_instances.hip): connected-component
 * labels of a footprint mask, exact per-component medians of a plane, and the RMSE-B / MAE-B / MedAE-B aggregates of the
 * reference's scripts/evaluator_instance.py:15-57.
 *
 * Same conventions as t2h.h and t2h_eval.h: device pointers owned by the caller, no allocation, no state, stream-ordered
 * calls, 0 or a negative T2H_ERR_* code, every argument validated before any launch.  The entries live in the same library
 * but are typed by tomosar2height_amd/instances.py (its own SIGNATURES table); T2H_ABI_VERSION is unchanged.
 *
 * Planes are row-major.  Pixel counts are limited to 2^31 - 1: a pixel's linear index is an int32, as a label is.
 */
#ifndef T2H_INST_H_
#define T2H_INST_H_

#include "t2h.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2H_INST_TILE 32         /* edge of the square tile one workgroup labels in LDS */
#define T2H_INST_TINY_MAX 64     /* segments up to this size: one wave each, ranked in registers */
#define T2H_INST_SMALL_MAX 2048  /* segments up to this size: one workgroup each, sorted in LDS; above: radix select */
#define T2H_INST_TABLE_COLS 8    /* n_valid, n_nan, sum |d|, sum d^2, median |d|, max |d|, 0, 0 (all as doubles) */

/* 4 * R * C bytes (the flattened parent plane) + 4 bytes per 1 024 pixels (scan partials), each rounded up to 256.
 * 0 for a shape the entry would refuse. */
size_t t2h_inst_label_workspace_bytes(int R, int C);

/* Connected components of the foreground (mask != 0) of the [R, C] window of a byte plane with row pitch ld >= C.
 * connectivity 1 = 4 neighbours, 2 = 8 neighbours (skimage.measure.label(mask, connectivity=2), the reference's).
 * labels [R, C] int32, contiguous: 0 for background, 1..K numbered in raster order of each component's first pixel
 * (the numbering of skimage and of scipy.ndimage.label); *n_labels = K, written on the device.  The result does not
 * depend on scheduling: two runs give the same bytes.
 * Replaces scripts/evaluator_instance.py:42. */
int t2h_inst_label(const uint8_t *mask, int ld, int R, int C, int connectivity, int32_t *labels, int32_t *n_labels,
                   void *workspace, size_t workspace_bytes, t2h_stream_t stream);

/* n = H * W pixels, K labels.  Linear in n and K: 256 + 12 * K + 8 * ceil(K / 1024) bytes of per-label tables, 8 * n
 * bytes of compacted (label, key) pairs, and (24 + 2 048) bytes for each of the at most n / (T2H_INST_SMALL_MAX + 1) + 1
 * segments that can be large (about 1 byte per pixel), each part rounded up to 256.  0 for a shape the entry would refuse. */
size_t t2h_inst_medians_workspace_bytes(int64_t n, int K);

/* counts[k-1] = |{labels == k}| and medians[k-1] = np.median(values32[labels == k]) for k = 1..K, where values32 is the
 * [H, W] window (row pitch ld >= W, in elements) of a float32 plane (is_f64 = 0) or of a float64 plane rounded to float32
 * (is_f64 = 1: what the reference's GeoTIFF round trip does, utils/io_raster.py:189).  labels [H, W] int32, contiguous;
 * values outside 1..K are background.  The median is the exact order statistic (s[(n-1)/2] + s[n/2]) / 2, formed in
 * float64 and rounded once to float32 (a zero median is +0, as numpy's mean has it); a segment that contains a NaN gives
 * NaN, as does an empty one.
 * Nothing here is raster-specific: any plane of values with a plane of labels will do.
 * Replaces scripts/evaluator_instance.py:15-27 (compute_median_height_per_building). */
int t2h_inst_medians(const void *values, int is_f64, int ld, int H, int W, const int32_t *labels, int K, int32_t *counts,
                     float *medians, void *workspace, size_t workspace_bytes, t2h_stream_t stream);

/* Over the K pairs of medians, d = (double)pred_med - (double)gt_med where both are finite:
 * table = { n_valid, n_nan = K - n_valid, sum |d|, sum d^2, median |d|, max |d|, 0, 0 }.  One workgroup: float64 partial
 * sums per thread in a fixed order, then a fixed tree; the median is an exact radix select.  K = 0 gives a zero table.
 * Replaces scripts/evaluator_instance.py:48-55. */
int t2h_inst_metrics(const float *pred_med, const float *gt_med, int K, double *table, t2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2H_INST_H_ */
