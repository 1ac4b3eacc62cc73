/* t2h_pnpp.h -- C ABI of the PointNet++ point stages in libt2h_hip.so (csrc/pnpp.hip): farthest point sampling, radius
 * grouping, grouped rows, grouped max and 3-nearest-neighbour feature propagation -- the index and gather work of the
 * reference's tomosar2height/encoder/pointnetpp.py (farthest_point_sample :220-241, query_ball_point :244-264,
 * sample_and_group :279-296, torch.max(new_points, 2) :55, PointNetFeaturePropagation.forward :90-97), and the adjoints of the
 * grouped rows, the grouped max and the propagation with respect to the FEATURES (xyz is input data: sampling, grouping, the
 * 3-NN indices and weights have no gradient).  The t2h_bn_* entries are BatchNorm in training mode over
 * the layers' rows: batch statistics, their backward and the running averages.
 *
 * Same conventions as t2h.h: device pointers owned by the caller, no allocation, no state, stream-ordered calls, 0 or a
 * negative T2H_ERR_* code, every argument validated before any launch.  The entries live in the same library but are typed by
 * tomosar2height_amd/pointops.py (its own SIGNATURES table); T2H_ABI_VERSION is unchanged.
 *
 * Inputs are dense [B, N, ...] fp32.  Every squared distance is taken by differences,
 *   d2 = ((dx * dx + dy * dy) + dz * dz),  dx = x - cx, ...   each operation rounded once in fp32, no fused multiply-add,
 * never by the reference's -2 x.y + |x|^2 + |y|^2 matmul form, whose rounding depends on the BLAS underneath.  No kernel
 * uses a float atomic, waits for another workgroup or depends on scheduling: two runs give the same bytes.  (t2h_index_transpose
 * places entries with INTEGER atomics and then orders every segment, so its result does not depend on scheduling either.)
 * No entry needs a workspace but t2h_fps: every other buffer, scratch included, is a typed argument whose size is stated here.
 */
#ifndef T2H_PNPP_H_
#define T2H_PNPP_H_

#include "t2h.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2H_FPS_ONE_WG_MAX 2048   /* largest N of the one-workgroup form (16 bytes of LDS per point: 32 KB) */

/* Bytes t2h_fps needs for (B, N) at `slice` points per workgroup (0: the one-workgroup form, which needs none; 1 byte is
 * reported so that the caller always has a buffer).  0 for arguments the entry would refuse. */
size_t t2h_fps_workspace_bytes(int B, int N, int slice);

/* Farthest point sampling: centroids [B, npoint] int64.  centroids[b, 0] = start[b] (int64 [B], clamped to [0, N)); then
 * `npoint - 1` times: distance[i] = min(distance[i], d2(i, last centroid)) (the reference's `dist < distance` update, from
 * 1e10), next centroid = the LOWEST index at which distance is largest.  That tie rule is this library's: the reference takes
 * whatever torch.max returns among equal maxima.  N < npoint repeats centroids as the reference does (all distances 0 ->
 * index 0).
 * slice == 0: one workgroup per cloud, coordinates and distances in LDS, N <= T2H_FPS_ONE_WG_MAX.
 * slice  > 0 (a multiple of 64): one LAUNCH per centroid over ceil(N / slice) workgroups per cloud.  Each workgroup first
 *   reduces the previous launch's per-slice (max, index) partials to find the centroid, then updates its own slice of the
 *   distances and writes its partial into the other half of a ping-pong pair.  Launch boundaries are the only
 *   synchronisation.  Both forms give the same bytes. */
int t2h_fps(const float *xyz, int B, int N, int npoint, const int64_t *start, int slice, int64_t *centroids, void *workspace,
            size_t workspace_bytes, t2h_stream_t stream);

/* Radius grouping: idx [B, S, nsample] int64 = per query new_xyz[b, s] the first `nsample` indices i, in index order, with
 * NOT (d2(xyz[b, i], query) > radius2); the remaining slots repeat the first index found.  A query that is one of the points
 * is always inside its own ball, so a group is never empty for the encoder; if it ever is, every slot holds N as in the
 * reference.  One wave per query, scanning 64 points at a time, leaving as soon as `nsample` are found. */
int t2h_ball_query(const float *xyz, const float *new_xyz, int B, int N, int S, float radius2, int nsample, int64_t *idx,
                   t2h_stream_t stream);

/* Grouped rows for the layers' products: rows [B * S * nsample, ld] fp32, row (b, s, j) =
 *   xyz[b, idx[b, s, j]] - new_xyz[b, s]  (3 columns) | points[b, idx[b, s, j]]  (D columns; points may be NULL with D = 0)
 *   | zeros up to ld >= 3 + D.   An index outside [0, N) (the empty group above) reads row N - 1. */
int t2h_group_rows(const float *xyz, const float *new_xyz, const float *points, const int64_t *idx, int B, int N, int S,
                   int nsample, int D, int ld, float *rows, t2h_stream_t stream);

/* out [groups, C] = max over the `nsample` consecutive rows of each group of rows [groups * nsample, ld] (columns 0 .. C). */
int t2h_group_max(const float *rows, int ld, int64_t groups, int nsample, int C, float *out, t2h_stream_t stream);

/* 3-nearest-neighbour feature propagation from S sources (xyz2 [B, S, 3], points2 [B, S, D]) to N targets (xyz1 [B, N, 3]):
 * idx [B, N, 3] int64 = the three smallest d2 in ascending order, equal d2 in ascending index; r_k = 1 / (d2_k + 1e-8),
 * weight [B, N, 3] = r_k / ((r_0 + r_1) + r_2), out [B, N, D] = (p_0 * w_0 + p_1 * w_1) + p_2 * w_2.  S == 1 is the reference's
 * `repeat` branch: idx 0, weight (1, 0, 0), out = the one source row (any D >= 1).  S == 2 is refused, as the reference fails on it. */
int t2h_three_nn_interp(const float *xyz1, const float *xyz2, const float *points2, int B, int N, int S, int D, int64_t *idx,
                        float *weight, float *out, t2h_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------- adjoints */
#define T2H_TRANSPOSE_SORT_MAX 8192 /* longest segment t2h_index_transpose orders in LDS (4 bytes per entry); longer: see there */
#define T2H_GATHER_CHUNK 64         /* entries per chunk of t2h_rows_gather_bwd's sums */
#define T2H_GATHER_LANES 4          /* interleaved chunk sums per output element */

/* Adjoint of t2h_group_max (same rows, ld, groups, nsample, C; out = its result [groups, C]; gout [groups, C] = the gradient of
 * out): grows [groups * nsample, gld], gld >= C.  Per group and column c < C the LOWEST row j of the group with
 * rows[j, c] - out[c] == 0 (fp32 subtraction; a NaN or infinite maximum matches no row) receives gout[c]; every other row of the
 * column receives +0; columns C .. gld are +0.  relu != 0: a column with NOT (out[c] > 0) receives +0 in every row -- the mask of
 * a ReLU applied to `rows` before the max, fused (max and ReLU commute).
 * The tie rule cannot change a parameter gradient.  Rows of a group that tie are either padded slots -- the ball query repeats
 * the first index, so they are copies of ONE source row with the same layer inputs, and the sum over the group of
 * (row gradient x layer input) is the same whichever copy takes it, as is the sum the gather's adjoint forms for that source --
 * or distinct rows that tie at 0, the only value ReLU makes common, where relu != 0 gives +0 to all of them. */
int t2h_group_max_bwd(const float *rows, int ld, int64_t groups, int nsample, int C, const float *out, const float *gout, int relu,
                      float *grows, int gld, t2h_stream_t stream);

/* Transpose of an index list: the CSR of idx [B, E] int64 by VALUE over N sources.  offsets [B, N + 1] int32, entries [B, E]
 * int32: entries[b, offsets[b, i] .. offsets[b, i + 1]) are the positions e with idx[b, e] == i in ASCENDING e -- per cloud,
 * entries = the stable argsort of idx.  An index outside [0, N) counts as N - 1 (t2h_group_rows reads row N - 1 for the
 * empty-group marker N).  cursor [B, N] int32 is scratch (any contents; overwritten).
 * Four launches behind a memset: counts (integer atomic adds into cursor), an exclusive scan per cloud, placement (an integer
 * atomic add hands each entry the next free slot of its segment, in an order that depends on scheduling), then one workgroup
 * per segment orders it by e: up to T2H_TRANSPOSE_SORT_MAX entries by a min/max sorting network in LDS, a longer one by
 * re-reading idx[b, :] in order.  The keys of a segment are distinct, so the bytes are fixed. */
int t2h_index_transpose(const int64_t *idx, int B, int E, int N, int32_t *offsets, int32_t *entries, int32_t *cursor,
                        t2h_stream_t stream);

/* Adjoint of a row gather through (offsets, entries) of t2h_index_transpose: out [B, N, D],
 *   out[b, i, d] = sum over e in entries[b, offsets[b, i] .. offsets[b, i + 1]) of w[b, e] * g[(b * E + e) / fan, col0 + d],
 * g [B * E / fan, gld] fp32 with gld >= col0 + D, weight [B, E] fp32 or NULL (w = 1), fan = 1 or 3 (E % fan == 0).
 *   fan = 1, col0 = 3, weight NULL: the adjoint of t2h_group_rows with respect to `points` (g = the gradient of rows, gld = ld);
 *   fan = 3, weight = the 3-NN weights: the adjoint of t2h_three_nn_interp with respect to `points2` (g = the gradient of out).
 * S == 1 (the `repeat` branch) is the same call with N = 1: every entry in segment 0, weights (1, 0, 0).
 * Association, the same for every element: the segment is cut into chunks of T2H_GATHER_CHUNK consecutive entries, chunk k =
 * entries offsets[b, i] + 64 k ..; a chunk sum starts from +0 and adds its terms in ascending order, term = w * g rounded, then
 * added (two roundings, no fused multiply-add); an entry with w == 0 is skipped, it adds no term (not even 0 * g, which an
 * infinite g would turn into NaN).  Lane sum y of T2H_GATHER_LANES starts from +0 and adds the chunk sums k = y, y + 4, y + 8,
 * ... in ascending k; out = ((lane_0 + lane_1) + lane_2) + lane_3.  An empty segment gives +0.  One workgroup per (b, i) and
 * 64 columns, one lane per column. */
int t2h_rows_gather_bwd(const float *g, int gld, int col0, int D, const float *weight, int fan, const int32_t *offsets,
                        const int32_t *entries, int B, int E, int N, float *out, t2h_stream_t stream);

/* ------------------------------------------------------------------------------------------- BatchNorm batch statistics */
#define T2H_BN_SLAB 256             /* rows per slab of the column reductions */
#define T2H_BN_WAVES 4              /* interleaved row sums per slab and column */

/* nn.BatchNorm2d / BatchNorm1d in training mode over the rows layout: the [B, C, nsample, S] / [B, C, N] reduction is the
 * reduction over the M rows of z [M, ld] fp32, per column c < C <= ld.  2 <= M <= 2^24 (M is used as an exact float; one value
 * per channel has no variance: torch raises, these entries refuse M < 2).  Every operation below is rounded once in fp32, no
 * fused multiply-add, no float atomic; launch boundaries are the only synchronisation.
 *
 * Association of a COLUMN SUM of terms t[r], the same for every reduction here: the rows are cut into slabs of T2H_BN_SLAB
 * consecutive rows, slab k = rows 256 k ..; lane sum w of T2H_BN_WAVES starts from +0 and adds the slab's terms of rows
 * 256 k + w, 256 k + w + 4, ... in ascending order; the slab's partial is ((lane_0 + lane_1) + lane_2) + lane_3; the column sum
 * starts from +0 and adds the slab partials in ascending k (a second launch).  `partial` is scratch of
 * ceil(M / T2H_BN_SLAB) * C floats (t2h_bn_bwd_reduce: twice that), any contents, overwritten.
 *
 * t2h_bn_col_stats, two passes (never E[z^2] - E[z]^2):  mean[c] = (column sum of z) / M;
 *   var[c] = (column sum of d * d, d = z - mean[c]) / M   (the biased variance);   rstd[c] = 1 / sqrt(var[c] + eps)
 *   (an addition, a correctly rounded square root, a correctly rounded division); 1e-30 <= eps <= 1e30. */
int t2h_bn_col_stats(const float *z, int ld, int M, int C, float eps, float *partial, float *mean, float *var, float *rstd,
                     t2h_stream_t stream);

/* y [M, ldy]: y[r, c] = max(z[r, c] * s + t, 0) with s = gamma[c] * rstd[c], t = beta[c] - mean[c] * s (a product, then a sum,
 * then the max); columns C .. ldy are +0 (the next product reads padded rows). */
int t2h_bn_apply_relu(const float *z, int ldz, int M, int C, const float *mean, const float *rstd, const float *gamma,
                      const float *beta, float *y, int ldy, t2h_stream_t stream);

/* running_mean = (1 - momentum) * running_mean + momentum * mean;
 * running_var  = (1 - momentum) * running_var  + momentum * (var * (M / (M - 1)))   in place, per column; (1 - momentum) and
 * M / (M - 1) are fp32 values, each side of the sum a rounded product.  num_batches_tracked is the caller's. */
int t2h_bn_running_update(const float *mean, const float *var, int M, int C, float momentum, float *running_mean,
                          float *running_var, t2h_stream_t stream);

/* Backward of y = [relu](gamma * xhat + beta), xhat = (z - mean) * rstd, given gy [M, ldg] = the gradient of y.
 * g = gy where relu == 0; relu != 0: g = gy & -(y > 0) (the bits of gy where y[r, c] > 0, +0 elsewhere; y [M, ldy] may be NULL
 * with relu == 0 -- the last layer of a set abstraction, where t2h_group_max_bwd(relu = 1) has applied the mask).
 * t2h_bn_bwd_reduce: dbeta[c] = column sum of g, dgamma[c] = column sum of g * xhat (xhat = (z - mean) * rstd: a difference, a
 *   product; then the product with g), in the association above. */
int t2h_bn_bwd_reduce(const float *gy, int ldg, const float *y, int ldy, const float *z, int ldz, int M, int C, const float *mean,
                      const float *rstd, int relu, float *partial, float *dbeta, float *dgamma, t2h_stream_t stream);

/* dz [M, gld]: dz[r, c] = a * ((g - mb) - xhat * mg) with a = gamma[c] * rstd[c], mb = dbeta[c] / M, mg = dgamma[c] / M;
 * columns C .. gld are +0. */
int t2h_bn_bwd_apply(const float *gy, int ldg, const float *y, int ldy, const float *z, int ldz, int M, int C, const float *mean,
                     const float *rstd, const float *gamma, const float *dbeta, const float *dgamma, int relu, float *dz, int gld,
                     t2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2H_PNPP_H_ */
