/* t2h_hg.h -- C ABI of the hourglass image encoder's own kernels in libt2h_hip.so (csrc/hourglass.hip): GroupNorm statistics
 * and apply, the direct stride-2 convolution, the 2 x 2 average pool and the ConvBlock tail -- what the reference's
 * tomosar2height/encoder/hourglass.py (ConvBlock :25-82, HourGlass :85-131, HGFilter :134-218) needs beside the 3 x 3 / 1 x 1
 * convolutions and the bicubic upsampling of t2h.h -- and the adjoints of GroupNorm, of the pool, of the tail and of the stride-2
 * convolution, on which ConvBlock, HourGlass and HGFilter train behind their `trainable` / `stem_gradients` switches (DESIGN.md
 * section 4.10).
 *
 * Same conventions as t2h.h: device pointers owned by the caller, no allocation, no state, stream-ordered calls, 0 or a
 * negative T2H_ERR_* code, every argument validated before any launch.  The entries live in the same library but are typed by
 * tomosar2height_amd/encoder/hourglass.py (its own SIGNATURES table); T2H_ABI_VERSION is unchanged.
 *
 * Every tensor is dense fp32 NHWC ([B, H, W, C]); pointers are 16-byte aligned and, except for the convolution's input, C is a
 * multiple of 4 (16-byte loads and stores along C).  No kernel uses a float atomic, waits for another workgroup or depends on
 * scheduling: two runs give the same bytes.
 */
#ifndef T2H_HG_H_
#define T2H_HG_H_

#include "t2h.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes t2h_hg_groupnorm_stats needs for the shape (the per-workgroup partials of groups that span several workgroups; 1 byte
 * is reported when one workgroup covers a sample, so that the caller always has a buffer).  0 for arguments the entry refuses. */
size_t t2h_hg_groupnorm_workspace_bytes(int B, int H, int W, int C, int G);

/* GroupNorm(G, C) statistics of x [B, H, W, C]: stats [B, G, 2] = (mean, rstd) per sample and group, rstd = 1 / sqrt(var + eps)
 * with the biased variance over the H * W * C / G elements of the group.  x is read once: every thread keeps a running
 * (n, mean, M2) per channel (Welford), and the partials are merged pairwise (n, mean, M2) -> (n, mean, M2) in a fixed order --
 * within a workgroup through LDS, across the workgroups of a sample through `workspace` in a second launch; the variance is
 * never formed as E[x^2] - E[x]^2.  C % 4 == 0, C % G == 0, at most 2^24 elements per group. */
int t2h_hg_groupnorm_stats(const float *x, int B, int H, int W, int C, int G, float eps, float *stats, void *workspace,
                           size_t workspace_bytes, t2h_stream_t stream);

/* y = relu?(((x - mean) * rstd) * scale[c] + shift[c]) with (mean, rstd) = stats[b, c / (C / G)] -- GroupNorm's affine output --
 * or, stats == NULL (G ignored), y = relu?(x * scale[c] + shift[c]): BatchNorm in eval() with the running statistics folded
 * into scale and shift by the caller.  Every operation is rounded once in fp32 (no fused multiply-add); relu is max(., 0).
 * y must not overlap x. */
int t2h_hg_norm_apply(const float *x, const float *stats, const float *scale, const float *shift, int B, int H, int W, int C, int G,
                      int relu, float *y, t2h_stream_t stream);

/* Direct K x K convolution with stride 2 and zero padding `pad`: x [B, H, W, Cin] -> y [B, OH, OW, Cout], OH = (H + 2 pad - K) / 2
 * + 1 (OW likewise), y = bias + sum over (cin chunk, ky) of [sum over (kx, ci) of x * w]: the inner sums by fp32 fused
 * multiply-adds in that order, each added to the running sum in (chunk, ky) order.  `w` is [K][K][Cin][Cout] (Cout contiguous); bias [Cout] or NULL.  K odd, 1 <= K <= 7, Cout a multiple of 64, any
 * Cin >= 1 (x needs 4-byte alignment only).  One workgroup per 8 x 8 output tile and 64 output channels, weights and the input
 * patch in LDS. */
int t2h_hg_conv_s2_fwd(const float *x, const float *w, const float *bias, float *y, int B, int H, int W, int Cin, int Cout, int K,
                       int pad, t2h_stream_t stream);

/* 2 x 2 average pool, stride 2: y [B, H / 2, W / 2, C] = (((x00 + x01) + x10) + x11) * 0.25 (row-major order of the window). */
int t2h_hg_avgpool2x2(const float *x, int B, int H, int W, int C, float *y, t2h_stream_t stream);

/* ConvBlock tail: y [P, C] = cat(o1 [P, C / 2], o2 [P, C / 4], o3 [P, C / 4]) + res [P, C] over P pixels in one pass.
 * C % 16 == 0. */
int t2h_hg_block_tail(const float *o1, const float *o2, const float *o3, const float *res, int64_t P, int C, float *y,
                      t2h_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------- adjoints */
#define T2H_HG_GNB_PIXELS 64        /* pixels of one sample per workgroup of the GroupNorm backward reduction */

/* Backward of y = relu?(gamma * xhat + beta), xhat = (x - mean) * rstd with (mean, rstd) = stats[b, c / (C / G)] of
 * t2h_hg_groupnorm_stats, given gy [B, H, W, C] = the gradient of y.  g = gy where y == NULL; else g = gy & -(y > 0): the bits of
 * gy where y [B, H, W, C] (the forward's output after its ReLU) is positive, +0 elsewhere.  xhat is rounded as the forward rounds
 * it (a difference, a product).  Every operation is rounded once in fp32, no fused multiply-add, no float atomic; launch
 * boundaries are the only synchronisation.  Shapes: those of t2h_hg_groupnorm_stats with C / G <= 256.
 *
 * t2h_hg_groupnorm_bwd_reduce writes
 *   dbeta[c] = sum over (b, pixel) of g,   dgamma[c] = sum over (b, pixel) of g * xhat,
 *   gsum[b, group] = (sum over the group of g * gamma, sum over the group of g * gamma * xhat)        [B, G, 2]
 * in this association, the same for both sums (term = g, or g * xhat rounded):  a sample's pixels are cut into chunks of
 * T2H_HG_GNB_PIXELS consecutive pixels, chunk k = pixels 64 k ..; with L = 256 / (C / 4) lanes (integer division), lane l starts
 * from +0 and adds the chunk's terms of pixels 64 k + l, 64 k + l + L, ... in ascending order; the chunk's partial is
 * ((lane_0 + lane_1) + lane_2) + ...; the SAMPLE's channel sum s[b, c] starts from +0 and adds the chunk partials in ascending k
 * (a second launch).  dbeta[c] / dgamma[c] start from +0 and add s[b, c] in ascending b.  A group sum starts from +0 and adds
 * gamma[c] * s[b, c] (rounded) over the group's channels in ascending c: the sum over the pixels is taken before the product
 * with gamma.  `partial` is scratch of  B * ceil(H * W / T2H_HG_GNB_PIXELS) * 2 * C  floats, any contents, overwritten. */
int t2h_hg_groupnorm_bwd_reduce(const float *gy, const float *y, const float *x, const float *stats, const float *gamma, int B,
                                int H, int W, int C, int G, float *partial, float *gsum, float *dbeta, float *dgamma,
                                t2h_stream_t stream);

/* dx [B, H, W, C] = rstd * ((g * gamma[c] - m1) - xhat * m2) [+ addend], m1 = gsum[b, group, 0] / n, m2 = gsum[b, group, 1] / n,
 * n = H * W * C / G (exact in fp32); g and xhat as above.  `addend` [B, H, W, C] or NULL is added last: the gradient of another
 * consumer of x (bn1 and bn4 of a ConvBlock normalise the same tensor; the identity residual).  dx must not overlap an input. */
int t2h_hg_groupnorm_bwd_apply(const float *gy, const float *y, const float *x, const float *stats, const float *gamma,
                               const float *gsum, const float *addend, int B, int H, int W, int C, int G, float *dx,
                               t2h_stream_t stream);

/* Adjoint of t2h_hg_avgpool2x2: dx [B, H, W, C], every pixel of a 2 x 2 window = gy [B, H / 2, W / 2, C] * 0.25 (exact).  H and W
 * even. */
int t2h_hg_avgpool2x2_bwd(const float *gy, int B, int H, int W, int C, float *dx, t2h_stream_t stream);

/* Adjoint of t2h_hg_block_tail: g [P, C] copied into three DENSE tensors d1 [P, C / 2], d2 [P, C / 4], d3 [P, C / 4] -- what the
 * 3 x 3 data and weight gradient kernels and t2h_hg_groupnorm_bwd_* (as gy or addend) take; no entry of this library reads the
 * slices of g in place.  The gradient of `res` is g itself: no copy is made.  C % 16 == 0. */
int t2h_hg_block_tail_bwd(const float *g, int64_t P, int C, float *d1, float *d2, float *d3, t2h_stream_t stream);

/* ------------------------------------------------------------------------- adjoints of the stride-2 convolution */
#define T2H_CS2_SLAB_ROWS 8         /* output rows ...                                                             */
#define T2H_CS2_SLAB_COLS 32        /* ... and columns of one sample that one workgroup of the weight gradient sums */

/* Both adjoints take the shapes of t2h_hg_conv_s2_fwd (K odd <= 7, pad <= K / 2, Cout % 64 == 0, any Cin >= 1, H + 2 pad >= K,
 * W + 2 pad >= K; anything else: T2H_ERR_ARG before a launch), the forward's weight layout [K][K][Cin][Cout] and, with
 * OH = (H + 2 pad - K) / 2 + 1 (OW likewise), gy [B, OH, OW, Cout].  fp32 fused multiply-adds (v_fma_f32), no float atomic, no
 * zero-fill pass: two runs give the same bytes.
 *
 * Data gradient: dx [B, H, W, Cin] = [addend +] sum over (ky, kx, co) of gy[b, oy, ox, co] * w[ky, kx, ci, co] over the taps with
 * iy + pad - ky = 2 oy, ix + pad - kx = 2 ox, 0 <= oy < OH, 0 <= ox < OW -- a gather: every element of dx is written exactly once,
 * an element no tap reaches (the last row when H + 2 pad - K is odd) is +0, or the addend (an addend of -0 gives +0).  One sum is
 * ONE chain of fused multiply-adds from +0, in this order: chunks of CK output channels ascending (what fits the staging buffers: CK = 16 for a
 * 3 x 3 layer of more than 16 input channels, 8 for the 7 x 7 stem), then the kernel rows of the parity of iy + pad ascending, then the kernel
 * columns of the parity of ix + pad ascending, then the chunk's output channels ascending; `addend` [B, H, W, Cin] or NULL (the
 * gradient of another consumer of x) is added last.  gy and w 16-byte aligned; dx and addend too when Cin % 4 == 0, else 4-byte.
 * dx must not overlap an input. */
int t2h_hg_conv_s2_dgrad(const float *gy, const float *w, const float *addend, float *dx, int B, int H, int W, int Cin, int Cout,
                         int K, int pad, t2h_stream_t stream);

/* Weight gradient: dw [K][K][Cin][Cout] = sum over (b, oy, ox) of x[b, 2 oy + ky - pad, 2 ox + kx - pad, ci] * gy[b, oy, ox, co]
 * (zero padding), dbias [Cout] = sum over (b, oy, ox) of gy (dbias may be NULL), in this association, the same for every
 * element: a sample's output pixels are cut into slabs of T2H_CS2_SLAB_ROWS x T2H_CS2_SLAB_COLS pixels, slab (sy, sx) = rows
 * 8 sy .., columns 32 sx ..; the slab's partial starts from +0 and adds its terms -- by one fused multiply-add each for dw, one
 * addition each for dbias -- over the slab's 8 x 8 tiles from left to right and the 64 pixels of a tile in row-major order (a pixel
 * outside the plane, or of the padding, counts as zero); a second launch starts from +0 and adds the slab partials in ascending
 * (b, sy, sx).  `partial` is scratch of
 *   B * ceil(OH / T2H_CS2_SLAB_ROWS) * ceil(OW / T2H_CS2_SLAB_COLS) * (K * K * Cin + 1) * Cout  floats,
 * any contents, overwritten (per slab the rows of dw, then dbias).  gy, partial, dw, dbias 16-byte aligned, x 4-byte. */
int t2h_hg_conv_s2_wgrad(const float *x, const float *gy, float *partial, float *dw, float *dbias, int B, int H, int W, int Cin,
                         int Cout, int K, int pad, t2h_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2H_HG_H_ */
