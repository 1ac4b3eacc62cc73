/* t2h_eval.h -- C ABI of the device DSM evaluator in libt2h_hip.so (csrc/dsm_eval.hip): the masked multi-class
 * residual statistics of the reference's test path (evaluator.py:14-99, utils/dilate_mask.py), with exact medians.
 *
 * Same conventions as t2h.h: device pointers owned by the caller, no allocation, no state, stream-ordered calls, 0 or a
 * negative T2H_ERR_* code, every argument validated before any launch.  The entries live in the same library but are
 * typed by tomosar2height_amd/evaluator.py (its own SIGNATURES table), not by _lib.SIGNATURES; T2H_ABI_VERSION is
 * unchanged.
 *
 * Planes are row-major and contiguous.  Mask planes are one byte per pixel (0 = false, anything else = true); the class
 * plane is one uint16 per pixel: bit 0 = 'overall' (= gt_mask), bit c = gt_mask & mask of class c, at most
 * T2H_EVAL_MAX_CLASSES bits.
 */
#ifndef T2H_EVAL_H_
#define T2H_EVAL_H_

#include "t2h.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2H_EVAL_MAX_CLASSES 16
#define T2H_EVAL_TABLE_COLS 8 /* n (int64 bits), min, max, sum|r|, sum r^2, median, abs_median, median|r - median| */

/* element kinds of t2h_eval_predicate's source plane */
#define T2H_EVAL_U8 0
#define T2H_EVAL_I16 1
#define T2H_EVAL_I32 2
#define T2H_EVAL_I64 3
#define T2H_EVAL_F32 4
#define T2H_EVAL_F64 5
/* predicates */
#define T2H_EVAL_NONZERO 0 /* .astype(bool)   (evaluator.py:19,31,51) */
#define T2H_EVAL_EQ 1      /* type_mask == v  (evaluator.py:39-41) */
#define T2H_EVAL_GT 2      /* type_mask > v   (evaluator.py:42) */

/* out[i] = pred(src[i]) as 0 / 1.  Replaces the `.astype(bool)` / `== v` / `> 0` of evaluator.py:19,31,39-42,51. */
int t2h_eval_predicate(const void *src, int kind, int op, double value, uint8_t *out, int64_t n, t2h_stream_t stream);

/* scipy.ndimage.binary_dilation(mask, iterations=k) with its defaults (cross element, border 0), computed as ONE dilation
 * by the L1 ball of radius k (the same set on a rectangle).  iterations >= 1; out must not alias in.
 * Replaces utils/dilate_mask.py:4-15 (called at evaluator.py:32,44-46). */
int t2h_eval_dilate(const uint8_t *in, uint8_t *out, int R, int C, int iterations, t2h_stream_t stream);

/* Bit `bit` of the class plane: cls[i] (|)= ((gt_mask ? gt_mask[i] != 0 : 1) & ((mask ? mask[i] != 0 : 1) ^ invert)) << bit.
 * bit 0 STORES the word (it initialises the plane: call it first), every other bit is OR-ed in.  invert = 1 is the
 * `terrain = ~building` of evaluator.py:33.  Replaces the `gt_mask_clip & mask_clip` of evaluator.py:59,70-71, done once
 * per evaluator on the whole raster instead of once per class and eval. */
int t2h_eval_class_bits(const uint8_t *mask, int invert, const uint8_t *gt_mask, int bit, uint16_t *cls, int64_t n,
                        t2h_stream_t stream);

/* The residual plane of an [H, W] target against the window of the [R, C] ground truth at (t_row, l_col):
 *     r = (double)target - (double)gt;   diff = bit 0 of cls ? r : NaN;   cw = isnan(r) ? 0 : cls   (both [H, W]).
 * target_f64 / gt_f64: 1 = float64 plane, 0 = float32.  The window must lie inside the ground truth.
 * Replaces evaluator.py:58-63,77-78. */
int t2h_eval_residual(const void *target, int target_f64, int H, int W, const void *gt, int gt_f64, const uint16_t *cls,
                      int R, int C, int t_row, int l_col, double *diff, uint16_t *cw, t2h_stream_t stream);

size_t t2h_eval_stats_workspace_bytes(int64_t n, int ncls);

/* The statistics of every class from the two planes t2h_eval_residual wrote (n = H * W pixels):
 * table[c * T2H_EVAL_TABLE_COLS + ...] = { n_c (int64 bit pattern), min, max, sum |r|, sum r^2, median(r), median(|r|),
 * median(|r - median(r)|) }; the last seven are undefined where n_c = 0.  Sums are float64, slab-then-tree in a fixed order;
 * the three medians are exact order statistics ((s[(n-1)/2] + s[n/2]) / 2) found by a most-significant-digit radix select on
 * the device, with no host synchronisation: the caller copies `table` back when it wants the numbers.
 * Replaces evaluator.py:82-99 (calculate_statistics) for all classes of evaluator.py:66-75 at once. */
int t2h_eval_stats(const double *diff, const uint16_t *cw, int64_t n, int ncls, double *table, void *workspace,
                   size_t workspace_bytes, t2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2H_EVAL_H_ */
