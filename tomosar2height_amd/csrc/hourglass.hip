// The hourglass image encoder's own kernels (include/t2h_hg.h; reference: tomosar2height/encoder/hourglass.py): GroupNorm
// statistics and apply, the direct stride-2 convolution (the 7 x 7 stem and the 3 x 3 hg_down = 'conv64' / 'conv128' layer), the
// 2 x 2 average pool and the ConvBlock tail cat(out1, out2, out3) + residual, and the adjoints of GroupNorm, of the pool, of the
// tail and of the stride-2 convolution (a gather over four parity classes for dx, slab-reduced dw: described at the kernels).
// fp32 NHWC throughout, 16-byte accesses along C wherever C % 4 == 0 is required.
//
// GroupNorm statistics.  x is read once.  A workgroup of 256 threads takes a run of pixels of one sample; thread t owns the four
// channels of float4 column t % (C / 4) and every (256 / (C / 4))-th pixel of the run, and keeps one Welford (n, mean, M2) per
// channel (n is shared by the four).  The partials go to LDS and one thread per group merges those of its channels in a fixed
// order (channel-major, then pixel lane) with the pairwise update
//     n = na + nb,  d = mb - ma,  mean = ma + d nb / n,  M2 = M2a + M2b + d^2 na nb / n,
// so the variance is never a difference of two large sums.  A sample that one workgroup covers is finished there; otherwise the
// per-workgroup (n, mean, M2) go to the workspace and a second launch merges them in workgroup order.  No atomics anywhere: two
// runs give the same bytes.
//
// The apply kernel's ReLU is fmaxf(y, 0): no compare whose result feeds a later select.
//
// GroupNorm backward.  Pass 1 (gn_bwd_partial_kernel) reads gy, y and x once: a workgroup takes T2H_HG_GNB_PIXELS pixels of one
// sample, thread t the float4 column t % (C / 4) and every (256 / (C / 4))-th pixel, and sums g and g * xhat per channel; the
// pixel lanes are added through LDS in ascending lane order and the workgroup's two sums per channel go to `partial`.  Pass 2
// (gn_bwd_finish_kernel, one lane per channel) adds the partials in ascending workgroup order into the sample's channel sums,
// those over the samples into dbeta / dgamma, and gamma times those over a group's channels into the two group sums.  The
// ReLU mask is gy & -(y > 0) by an opaque v_med3_i32 and an AND; bounds are loop limits and branches.  The association is
// stated in include/t2h_hg.h.
#include <math.h>

#include "t2h_common.h"
#include "../../include/t2h_hg.h"

namespace t2h {

constexpr int kHgThreads = 256;
constexpr int kGnChunkFloats = 65536;          // floats of one sample a statistics workgroup reads
constexpr int kGnbPixels = T2H_HG_GNB_PIXELS;  // pixels of one sample a workgroup of the backward reduction reads
constexpr int kGnbMaxCpg = kHgThreads;         // channels per group the backward takes (a group never straddles a finish workgroup)

constexpr int kCvTile = 8;                     // output tile of the strided convolution: 8 x 8 pixels x 64 channels per workgroup
constexpr int kCvCout = 64;
constexpr int kCvWMax = 7 * 7 * 3 * kCvCout;   // floats of weights staged at a time: the whole 7 x 7 x 3 stem, 16 channels of a 3 x 3
constexpr int kCvPMax = 17 * 17 * 16;          // floats of input patch staged at a time (3 x 3: 17 x 17 x 16; 7 x 7: 21 x 21 x 3)

constexpr int kDgWFloats = 9 * 16 * 68;        // data gradient: floats of transposed weights staged at a time (3 x 3, 16 output channels, 64 + 4 input channels)
constexpr int kDgPFloats = 6144;               // ... and of gy patch (7 x 7 stem: 19 x 35 pixels x (8 | 1) output channels)
constexpr int kWgRows = 10;                    // weight gradient: weight rows (tap, input channel) per thread, 16 kWgRows per workgroup
constexpr int kWgPFloats = kCvPMax;            // ... floats of input patch staged at a time (the forward's patches)
constexpr int kWgSlabRows = T2H_CS2_SLAB_ROWS; // ... output pixels of one slab
constexpr int kWgSlabCols = T2H_CS2_SLAB_COLS;
static_assert(kWgSlabRows == kCvTile && kWgSlabCols % kCvTile == 0, "a slab is a row of whole 8 x 8 tiles");

namespace {

struct Moments { float n, mean, m2; };

// Without a compare (no compare result feeds a select): counts are whole numbers, so fmaxf(n, 1) changes
// nothing but 0 / 0; an empty b (n = 0, mean = M2 = 0) leaves a as it is (f = 0), an empty a takes b exactly (f = 1, na f = 0).
__device__ inline void merge(Moments &a, const Moments &b) {
    const float n = a.n + b.n, d = b.mean - a.mean, f = b.n / fmaxf(n, 1.f);
    a.mean = a.mean + d * f;
    a.m2 = (a.m2 + b.m2) + (d * d) * (a.n * f);
    a.n = n;
}

__device__ inline void finish(const Moments &m, float eps, float *stats) {
    stats[0] = m.mean;
    stats[1] = 1.f / sqrtf(m.m2 / m.n + eps);
}

// grid (chunks, B).  out: stats [B, G, 2] when one chunk covers the sample, else partials [B, chunks, G, 3].
__global__ __launch_bounds__(kHgThreads) void gn_partial_kernel(const float *__restrict__ x, int HW, int C, int G, int chunk_pixels,
                                                                int final_pass, float eps, float *__restrict__ out) {
    __shared__ float s_n[kHgThreads];
    __shared__ float s_mean[kHgThreads * 4];
    __shared__ float s_m2[kHgThreads * 4];
    const int t = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int C4 = C >> 2, lanes = kHgThreads / C4;
    const int c4 = t % C4, lane = t / C4;
    float n = 0.f, mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane < lanes) {
        const int p0 = chunk * chunk_pixels, p1 = min(HW, p0 + chunk_pixels);
        const float *src = x + ((long long)b * HW) * C + c4 * 4;
        for (int p = p0 + lane; p < p1; p += lanes) {
            const float4 v4 = *reinterpret_cast<const float4 *>(src + (long long)p * C);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
            n += 1.f;
            const float inv = 1.f / n;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = v[j] - mean[j];
                mean[j] += d * inv;
                m2[j] += d * (v[j] - mean[j]);
            }
        }
    }
    s_n[t] = n;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s_mean[t * 4 + j] = mean[j]; s_m2[t * 4 + j] = m2[j]; }
    __syncthreads();
    for (int g = t; g < G; g += kHgThreads) {
        const int cpg = C / G;
        Moments acc{0.f, 0.f, 0.f};
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            const int col = c >> 2, j = c & 3;
            for (int l = 0; l < lanes; ++l) {
                const int o = l * C4 + col;
                merge(acc, Moments{s_n[o], s_mean[o * 4 + j], s_m2[o * 4 + j]});
            }
        }
        if (final_pass) {
            finish(acc, eps, out + ((long long)b * G + g) * 2);
        } else {
            float *dst = out + (((long long)b * gridDim.x + chunk) * G + g) * 3;
            dst[0] = acc.n; dst[1] = acc.mean; dst[2] = acc.m2;
        }
    }
}

// one thread per (sample, group): the chunks' partials merged in chunk order
__global__ __launch_bounds__(kHgThreads) void gn_final_kernel(const float *__restrict__ partials, int BG, int G, int chunks, float eps,
                                                              float *__restrict__ stats) {
    const int i = blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= BG) return;
    const int b = i / G, g = i % G;
    Moments acc{0.f, 0.f, 0.f};
    for (int k = 0; k < chunks; ++k) {
        const float *src = partials + (((long long)b * chunks + k) * G + g) * 3;
        merge(acc, Moments{src[0], src[1], src[2]});
    }
    finish(acc, eps, stats + (long long)i * 2);
}

// one thread per float4 of the output
__global__ __launch_bounds__(kHgThreads) void norm_apply_kernel(const float *__restrict__ x, const float *__restrict__ stats,
                                                                const float *__restrict__ scale, const float *__restrict__ shift,
                                                                long long total4, int HW, int C, int G, int relu,
                                                                float *__restrict__ y) {
    const long long i = (long long)blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= total4) return;
    const int C4 = C >> 2;
    const int c = (int)(i % C4) * 4;
    const float4 v4 = *reinterpret_cast<const float4 *>(x + i * 4);
    const float4 s4 = *reinterpret_cast<const float4 *>(scale + c), h4 = *reinterpret_cast<const float4 *>(shift + c);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w}, s[4] = {s4.x, s4.y, s4.z, s4.w}, h[4] = {h4.x, h4.y, h4.z, h4.w};
    float r[4];
    if (stats) {
        const int b = (int)((i / C4) / HW), cpg = C / G;
        const float *st = stats + (long long)b * G * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int g = (c + j) / cpg;
            r[j] = ((v[j] - st[2 * g]) * st[2 * g + 1]) * s[j] + h[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = v[j] * s[j] + h[j];
    }
    if (relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = fmaxf(r[j], 0.f);
    }
    *reinterpret_cast<float4 *>(y + i * 4) = make_float4(r[0], r[1], r[2], r[3]);
}

// all ones where x > 0, 0 elsewhere (+-0, negative, NaN with the sign bit): -med3(bits, 0, 1) on the bits as a signed integer.
// (the clamp is an opaque v_med3_i32: written as min(max(bits, 0), 1) the compiler may turn it into a compare and a select)
__device__ inline unsigned hg_positive_mask(float x) {
    int m;
    asm("v_med3_i32 %0, %1, 0, 1" : "=v"(m) : "v"(__float_as_int(x)));
    return (unsigned)(-m);
}

// g of the GroupNorm backward: the bits of gy where y > 0 (or everywhere: keep_all), +0 elsewhere
__device__ inline float hg_masked(float gy, float y, unsigned keep_all) {
    return __uint_as_float(__float_as_uint(gy) & (hg_positive_mask(y) | keep_all));
}

// grid (chunks, B).  partial [B, chunks, 2, C]: per channel, the workgroup's sums of g and of g * xhat.
__global__ __launch_bounds__(kHgThreads) void gn_bwd_partial_kernel(const float *__restrict__ gy, const float *__restrict__ y,
                                                                    const float *__restrict__ x, const float *__restrict__ stats,
                                                                    int HW, int C, int G, unsigned keep_all,
                                                                    float *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_sum[2][kHgThreads * 4];
    const int t = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x;
    const int C4 = C >> 2, lanes = kHgThreads / C4, cpg = C / G;
    const int c4 = t % C4, lane = t / C4;
    float sg[4] = {0.f, 0.f, 0.f, 0.f}, sx[4] = {0.f, 0.f, 0.f, 0.f};
    if (lane < lanes) {
        const int p0 = chunk * kGnbPixels, p1 = min(HW, p0 + kGnbPixels);
        const long long base = ((long long)b * HW) * C + c4 * 4;
        float mu[4], rs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float *st = stats + ((long long)b * G + (c4 * 4 + j) / cpg) * 2;
            mu[j] = st[0];
            rs[j] = st[1];
        }
        for (int p = p0 + lane; p < p1; p += lanes) {
            const long long o = base + (long long)p * C;
            const float4 g4 = *reinterpret_cast<const float4 *>(gy + o), y4 = *reinterpret_cast<const float4 *>(y + o);
            const float4 x4 = *reinterpret_cast<const float4 *>(x + o);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, yv[4] = {y4.x, y4.y, y4.z, y4.w}, xv[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float g = hg_masked(gv[j], yv[j], keep_all);
                const float xhat = __fmul_rn(__fsub_rn(xv[j], mu[j]), rs[j]);
                sg[j] = __fadd_rn(sg[j], g);
                sx[j] = __fadd_rn(sx[j], __fmul_rn(g, xhat));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { s_sum[0][t * 4 + j] = sg[j]; s_sum[1][t * 4 + j] = sx[j]; }
    __syncthreads();
    if (t < C4) {                                  // lane 0 of column t: its own sums, then lanes 1, 2, ... in ascending order
        for (int l = 1; l < lanes; ++l) {
            const int o = (l * C4 + t) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) { sg[j] = __fadd_rn(sg[j], s_sum[0][o + j]); sx[j] = __fadd_rn(sx[j], s_sum[1][o + j]); }
        }
        float *dst = partial + (((long long)b * gridDim.x + chunk) * 2) * C + t * 4;
        *reinterpret_cast<float4 *>(dst) = make_float4(sg[0], sg[1], sg[2], sg[3]);
        *reinterpret_cast<float4 *>(dst + C) = make_float4(sx[0], sx[1], sx[2], sx[3]);
    }
}

// grid (ceil(C / cb)), cb = the largest multiple of C / G up to 256: one lane per channel, whole groups per workgroup.  Per sample
// in ascending order: the channel's two sums over the workgroups of pass 1 in ascending order from +0; added to dbeta / dgamma;
// gamma times them through LDS to the first lane of the group, which adds the group's channels in ascending order from +0.
__global__ __launch_bounds__(kHgThreads) void gn_bwd_finish_kernel(const float *__restrict__ partial, const float *__restrict__ gamma,
                                                                   int B, int chunks, int C, int G, int cb, float *__restrict__ gsum,
                                                                   float *__restrict__ dbeta, float *__restrict__ dgamma) {
    __shared__ float ss[2][kHgThreads];
    const int t = threadIdx.x, c = blockIdx.x * cb + t, cpg = C / G;
    const bool live = t < cb && c < C;
    float gm = 0.f, db = 0.f, dg = 0.f;
    if (live) gm = gamma[c];
    for (int b = 0; b < B; ++b) {
        float s0 = 0.f, s1 = 0.f;
        if (live) {
            const float *src = partial + ((long long)b * chunks) * 2 * C + c;
#pragma unroll 8
            for (int k = 0; k < chunks; ++k) {
                s0 = __fadd_rn(s0, src[(long long)k * 2 * C]);
                s1 = __fadd_rn(s1, src[(long long)k * 2 * C + C]);
            }
            db = __fadd_rn(db, s0);
            dg = __fadd_rn(dg, s1);
        }
        ss[0][t] = __fmul_rn(gm, s0);
        ss[1][t] = __fmul_rn(gm, s1);
        __syncthreads();
        if (live && t % cpg == 0) {
            float a0 = 0.f, a1 = 0.f;
            for (int k = 0; k < cpg; ++k) { a0 = __fadd_rn(a0, ss[0][t + k]); a1 = __fadd_rn(a1, ss[1][t + k]); }
            float *dst = gsum + ((long long)b * G + c / cpg) * 2;
            dst[0] = a0;
            dst[1] = a1;
        }
        __syncthreads();
    }
    if (live) { dbeta[c] = db; dgamma[c] = dg; }
}

// one thread per float4 of dx: dx = rstd * ((g * gamma - m1) - xhat * m2) [+ addend], m1 and m2 the group sums over n = HW * C / G
__global__ __launch_bounds__(kHgThreads) void gn_bwd_apply_kernel(const float *__restrict__ gy, const float *__restrict__ y,
                                                                  const float *__restrict__ x, const float *__restrict__ stats,
                                                                  const float *__restrict__ gamma, const float *__restrict__ gsum,
                                                                  const float *__restrict__ addend, long long total4, int HW, int C,
                                                                  int G, unsigned keep_all, float *__restrict__ dx) {
    const long long i = (long long)blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= total4) return;
    const int C4 = C >> 2, cpg = C / G;
    const int c = (int)(i % C4) * 4, b = (int)((i / C4) / HW);
    const float n = (float)((long long)HW * cpg);
    float mu[4], rs[4], m1[4], m2[4];
    const bool shared = (cpg & 3) == 0;                    // (uniform) the four channels of a float4 share a group
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j > 0 && shared) {
            mu[j] = mu[0]; rs[j] = rs[0]; m1[j] = m1[0]; m2[j] = m2[0];
            continue;
        }
        const long long o = ((long long)b * G + (c + j) / cpg) * 2;
        mu[j] = stats[o];
        rs[j] = stats[o + 1];
        m1[j] = __fdiv_rn(gsum[o], n);
        m2[j] = __fdiv_rn(gsum[o + 1], n);
    }
    const float4 g4 = *reinterpret_cast<const float4 *>(gy + i * 4), y4 = *reinterpret_cast<const float4 *>(y + i * 4);
    const float4 x4 = *reinterpret_cast<const float4 *>(x + i * 4), w4 = *reinterpret_cast<const float4 *>(gamma + c);
    const float gv[4] = {g4.x, g4.y, g4.z, g4.w}, yv[4] = {y4.x, y4.y, y4.z, y4.w}, xv[4] = {x4.x, x4.y, x4.z, x4.w};
    const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float g = hg_masked(gv[j], yv[j], keep_all);
        const float xhat = __fmul_rn(__fsub_rn(xv[j], mu[j]), rs[j]);
        r[j] = __fmul_rn(rs[j], __fsub_rn(__fsub_rn(__fmul_rn(g, wv[j]), m1[j]), __fmul_rn(xhat, m2[j])));
    }
    if (addend) {
        const float4 a4 = *reinterpret_cast<const float4 *>(addend + i * 4);
        r[0] = __fadd_rn(r[0], a4.x); r[1] = __fadd_rn(r[1], a4.y); r[2] = __fadd_rn(r[2], a4.z); r[3] = __fadd_rn(r[3], a4.w);
    }
    *reinterpret_cast<float4 *>(dx + i * 4) = make_float4(r[0], r[1], r[2], r[3]);
}

// grid (tiles, Cout / 64, B); thread t: channels 4 (t % 16) .. + 3 of the workgroup's 64, output row t / 32 of the tile and the
// four columns 4 ((t / 16) % 2) .. + 3.  Per chunk of CK input channels: weights [K][K][ck][64] and the zero-padded input patch
// [14 + K][14 + K][ck] are staged in LDS; the 16 lanes that share a pixel read the same patch word (broadcast) and 64 consecutive
// weights.
__global__ __launch_bounds__(kHgThreads) void conv_s2_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                             const float *__restrict__ bias, float *__restrict__ y, int H, int W,
                                                             int Cin, int Cout, int OH, int OW, int K, int pad, int CK, int tiles_x) {
    __shared__ __attribute__((aligned(16))) float sw[kCvWMax];
    __shared__ float sp[kCvPMax];
    const int t = threadIdx.x, cg = t & 15, pg = t >> 4, row = pg >> 1, colb = (pg & 1) * 4;
    const int ty0 = (blockIdx.x / tiles_x) * kCvTile, tx0 = (blockIdx.x % tiles_x) * kCvTile;
    const int co0 = blockIdx.y * kCvCout, b = blockIdx.z;
    const int PW = 2 * kCvTile + K - 2;
    const int iy0 = 2 * ty0 - pad, ix0 = 2 * tx0 - pad;
    float acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[j][k] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += CK) {
        const int ck = min(CK, Cin - c0);
        __syncthreads();
        const int nw = K * K * ck * kCvCout;
        for (int i = t; i < nw; i += kHgThreads) {
            const int co = i % kCvCout, r = i / kCvCout, ci = r % ck, kk = r / ck;
            sw[i] = w[((long long)kk * Cin + c0 + ci) * Cout + co0 + co];
        }
        const int np = PW * PW * ck;
        for (int i = t; i < np; i += kHgThreads) {
            const int ci = i % ck, r = i / ck, px = r % PW, py = r / PW;
            const int iy = iy0 + py, ix = ix0 + px;
            float v = 0.f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[(((long long)b * H + iy) * W + ix) * Cin + c0 + ci];
            sp[i] = v;
        }
        __syncthreads();
        for (int ky = 0; ky < K; ++ky) {
            float part[4][4];              // one kernel row of one chunk (K ck terms) on its own, then onto the running sum
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) part[j][k] = 0.f;
            for (int kx = 0; kx < K; ++kx) {
                const float *wk = sw + (ky * K + kx) * ck * kCvCout + cg * 4;
                const float *pk = sp + ((2 * row + ky) * PW + 2 * colb + kx) * ck;
                for (int ci = 0; ci < ck; ++ci) {
                    const float4 wv = *reinterpret_cast<const float4 *>(wk + ci * kCvCout);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xv = pk[2 * j * ck + ci];
                        part[j][0] = fmaf(xv, wv.x, part[j][0]);
                        part[j][1] = fmaf(xv, wv.y, part[j][1]);
                        part[j][2] = fmaf(xv, wv.z, part[j][2]);
                        part[j][3] = fmaf(xv, wv.w, part[j][3]);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[j][k] += part[j][k];
        }
    }
    const int oy = ty0 + row, co = co0 + cg * 4;
    if (oy >= OH) return;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) bv = *reinterpret_cast<const float4 *>(bias + co);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ox = tx0 + colb + j;
        if (ox < OW)
            *reinterpret_cast<float4 *>(y + (((long long)b * OH + oy) * OW + ox) * Cout + co) =
                make_float4(acc[j][0] + bv.x, acc[j][1] + bv.y, acc[j][2] + bv.z, acc[j][3] + bv.w);
    }
}

__global__ __launch_bounds__(kHgThreads) void avgpool2x2_kernel(const float *__restrict__ x, long long total4, int H, int W, int C,
                                                                float *__restrict__ y) {
    const long long i = (long long)blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= total4) return;
    const int C4 = C >> 2, OH = H >> 1, OW = W >> 1;
    const int c = (int)(i % C4) * 4;
    long long r = i / C4;
    const int ox = (int)(r % OW);
    r /= OW;
    const int oy = (int)(r % OH), b = (int)(r / OH);
    const float *p = x + ((((long long)b * H + 2 * oy) * W + 2 * ox) * C + c);
    const float4 a = *reinterpret_cast<const float4 *>(p), bq = *reinterpret_cast<const float4 *>(p + C);
    const float4 cq = *reinterpret_cast<const float4 *>(p + (long long)W * C), d = *reinterpret_cast<const float4 *>(p + (long long)W * C + C);
    *reinterpret_cast<float4 *>(y + i * 4) = make_float4((((a.x + bq.x) + cq.x) + d.x) * 0.25f, (((a.y + bq.y) + cq.y) + d.y) * 0.25f,
                                                         (((a.z + bq.z) + cq.z) + d.z) * 0.25f, (((a.w + bq.w) + cq.w) + d.w) * 0.25f);
}

__global__ __launch_bounds__(kHgThreads) void block_tail_kernel(const float *__restrict__ o1, const float *__restrict__ o2,
                                                                const float *__restrict__ o3, const float *__restrict__ res,
                                                                long long total4, int C, float *__restrict__ y) {
    const long long i = (long long)blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= total4) return;
    const int C4 = C >> 2, half = C >> 1, quarter = C >> 2;
    const int c = (int)(i % C4) * 4;
    const long long p = i / C4;
    const float *src = c < half ? o1 + p * half + c : (c < half + quarter ? o2 + p * quarter + (c - half) : o3 + p * quarter + (c - half - quarter));
    const float4 a = *reinterpret_cast<const float4 *>(src), r = *reinterpret_cast<const float4 *>(res + i * 4);
    *reinterpret_cast<float4 *>(y + i * 4) = make_float4(a.x + r.x, a.y + r.y, a.z + r.z, a.w + r.w);
}

// one thread per float4 of gy [B, H / 2, W / 2, C]: gy * 0.25 to the four pixels of its window (H and W even: every pixel of dx)
__global__ __launch_bounds__(kHgThreads) void avgpool2x2_bwd_kernel(const float *__restrict__ gy, long long total4, int H, int W, int C,
                                                                    float *__restrict__ dx) {
    const long long i = (long long)blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= total4) return;
    const int C4 = C >> 2, OH = H >> 1, OW = W >> 1;
    const int c = (int)(i % C4) * 4;
    long long r = i / C4;
    const int ox = (int)(r % OW);
    r /= OW;
    const int oy = (int)(r % OH), b = (int)(r / OH);
    const float4 g = *reinterpret_cast<const float4 *>(gy + i * 4);
    const float4 q = make_float4(g.x * 0.25f, g.y * 0.25f, g.z * 0.25f, g.w * 0.25f);
    float *p = dx + ((((long long)b * H + 2 * oy) * W + 2 * ox) * C + c);
    *reinterpret_cast<float4 *>(p) = q;
    *reinterpret_cast<float4 *>(p + C) = q;
    *reinterpret_cast<float4 *>(p + (long long)W * C) = q;
    *reinterpret_cast<float4 *>(p + (long long)W * C + C) = q;
}

// one thread per float4 of g [P, C]: copied to its place in d1 [P, C / 2], d2 [P, C / 4] or d3 [P, C / 4]
__global__ __launch_bounds__(kHgThreads) void block_tail_bwd_kernel(const float *__restrict__ g, long long total4, int C,
                                                                    float *__restrict__ d1, float *__restrict__ d2,
                                                                    float *__restrict__ d3) {
    const long long i = (long long)blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= total4) return;
    const int C4 = C >> 2, half = C >> 1, quarter = C >> 2;
    const int c = (int)(i % C4) * 4;
    const long long p = i / C4;
    float *dst = c < half ? d1 + p * half + c : (c < half + quarter ? d2 + p * quarter + (c - half) : d3 + p * quarter + (c - half - quarter));
    *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(g + i * 4);
}

// ---------------------------------------------------------------------------------- stride-2 convolution: data gradient
// One kernel row / column pair of one parity class of the data gradient for a thread's two q-blocks (a q-block = the 2 x 2 input
// pixels with (iy + pad) / 2 = qy, (ix + pad) / 2 = qx; class = 2 py + px, the parities of iy + pad and ix + pad): over the staged
// output channels in ascending order, acc += gy * w by one fused multiply-add each.  NY / NX: the tap pair also has a kernel
// row 2 a + 1 / a kernel column 2 c + 1 (a template argument: a loop bound of the caller, never a per-lane value).
template <bool NY, bool NX>
__device__ inline void dgrad_taps(float (&acc)[2][4][4], const float *g0, int PS, const float *wk, int WS, int row_step, int ck) {
    for (int co = 0; co < ck; ++co) {
        const float g[2] = {g0[co], g0[PS + co]};
        const float *wc = wk + co * WS;
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            if ((cls >= 2 && !NY) || ((cls & 1) && !NX)) continue;
            const float4 wv = *reinterpret_cast<const float4 *>(wc + (cls >> 1) * row_step + (cls & 1) * ck * WS);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                acc[q][cls][0] = fmaf(g[q], wv.x, acc[q][cls][0]);
                acc[q][cls][1] = fmaf(g[q], wv.y, acc[q][cls][1]);
                acc[q][cls][2] = fmaf(g[q], wv.z, acc[q][cls][2]);
                acc[q][cls][3] = fmaf(g[q], wv.w, acc[q][cls][3]);
            }
        }
    }
}

// grid (tiles, ceil(Cin / (4 CG)), B).  CG = 16: a workgroup takes 64 input channels and 4 x 8 q-blocks (8 x 16 pixels), the 16
// lanes of a pixel group hold consecutive float4s of channels (Cin = 128); CG = 1: 4 input channels and 16 x 32 q-blocks, every lane
// another pixel group (Cin = 3).  Thread: two q-blocks side by side x the four parity classes x 4 channels.  Per chunk of CK output
// channels the weights, transposed to [K][K][ck][4 CG (+ 4)] (input channels contiguous; zero past Cin), and the zero-padded gy
// patch [S + A - 1][2 S + A - 1][ck | 1], A = (K + 1) / 2, are staged in LDS: borders and parity are the patch's zeros and the
// loop bounds.  A gather: every dx element is written once, by the thread that summed it.
template <int CG>
__global__ __launch_bounds__(kHgThreads) void conv_s2_dgrad_kernel(const float *__restrict__ gy, const float *__restrict__ w,
                                                                   const float *__restrict__ addend, float *__restrict__ dx, int H,
                                                                   int W, int Cin, int Cout, int OH, int OW, int K, int pad, int CK,
                                                                   int tiles_x, int vec) {
    constexpr int S = CG == 16 ? 4 : 16, CIT = 4 * CG, WS = CIT + 4;
    __shared__ __attribute__((aligned(16))) float sw[kDgWFloats];
    __shared__ float sg[kDgPFloats];
    const int t = threadIdx.x, cg = t % CG, pg = t / CG, qyl = pg / S, qxl = 2 * (pg % S);
    const int A = (K + 1) / 2, PWX = 2 * S + A - 1, PWY = S + A - 1;
    const int q0y = (blockIdx.x / tiles_x) * S, q0x = (blockIdx.x % tiles_x) * 2 * S;
    const int ci0 = blockIdx.y * CIT, b = blockIdx.z;
    float acc[2][4][4];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[q][cls][j] = 0.f;
    for (int c0 = 0; c0 < Cout; c0 += CK) {
        const int ck = min(CK, Cout - c0), PS = ck | 1;
        __syncthreads();
        const int nw = K * K * ck * CIT;
        for (int i = t; i < nw; i += kHgThreads) {
            const int co = i % ck, r = i / ck, ci = r % CIT, kk = r / CIT;
            float v = 0.f;
            if (ci0 + ci < Cin) v = w[((long long)kk * Cin + ci0 + ci) * Cout + c0 + co];
            sw[(kk * ck + co) * WS + ci] = v;
        }
        const int np = PWY * PWX * ck;
        for (int i = t; i < np; i += kHgThreads) {
            const int co = i % ck, r = i / ck, cx = r % PWX, ry = r / PWX;
            const int oy = q0y - (A - 1) + ry, ox = q0x - (A - 1) + cx;
            float v = 0.f;
            if (oy >= 0 && oy < OH && ox >= 0 && ox < OW) v = gy[(((long long)b * OH + oy) * OW + ox) * Cout + c0 + co];
            sg[r * PS + co] = v;
        }
        __syncthreads();
        for (int a = 0; a < A; ++a) {                  // kernel rows 2 a (+ 1) meet output row qy - a
            for (int c = 0; c < A; ++c) {
                const float *g0 = sg + ((qyl + A - 1 - a) * PWX + (qxl + A - 1 - c)) * PS;
                const float *wk = sw + ((2 * a * K + 2 * c) * ck) * WS + cg * 4;
                const int row_step = K * ck * WS;
                const bool ny = 2 * a + 1 < K, nx = 2 * c + 1 < K;
                if (ny && nx) dgrad_taps<true, true>(acc, g0, PS, wk, WS, row_step, ck);
                else if (ny) dgrad_taps<true, false>(acc, g0, PS, wk, WS, row_step, ck);
                else if (nx) dgrad_taps<false, true>(acc, g0, PS, wk, WS, row_step, ck);
                else dgrad_taps<false, false>(acc, g0, PS, wk, WS, row_step, ck);
            }
        }
    }
    const int ci = ci0 + cg * 4;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int iy = 2 * (q0y + qyl) + (cls >> 1) - pad, ix = 2 * (q0x + qxl + q) + (cls & 1) - pad;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const long long o = (((long long)b * H + iy) * W + ix) * Cin + ci;
            if (vec) {
                if (ci < Cin) {
                    float4 r = make_float4(acc[q][cls][0], acc[q][cls][1], acc[q][cls][2], acc[q][cls][3]);
                    if (addend) {
                        const float4 a4 = *reinterpret_cast<const float4 *>(addend + o);
                        r = make_float4(r.x + a4.x, r.y + a4.y, r.z + a4.z, r.w + a4.w);
                    }
                    *reinterpret_cast<float4 *>(dx + o) = r;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (ci + j < Cin) {
                        float r = acc[q][cls][j];
                        if (addend) r += addend[o + j];
                        dx[o + j] = r;
                    }
                }
            }
        }
    }
}

// -------------------------------------------------------------------------------- stride-2 convolution: weight gradient
// grid (slabs of a sample, chunks of input channels x Cout / 64, B).  A workgroup owns one slab -- T2H_CS2_SLAB_ROWS x
// T2H_CS2_SLAB_COLS output pixels of one sample, up to four 8 x 8 tiles side by side --, CK input channels and 64 output channels.
// Thread t: output channels 4 (t % 16) .. + 3 and the kWgRows weight rows m = t / 16 + 16 r of the chunk's K K ck rows
// (m = (ky K + kx) ck + ci).  Per tile the gy tile [64][64] (zero outside the plane) and the zero-padded x patch
// [14 + K][14 + K][ck] are staged in LDS; a row past the chunk reads row K K ck - 1 again and is not stored.  Every sum is one
// chain of fused multiply-adds from +0 over the slab's tiles from left to right and a tile's 64 pixels in row-major order.
__global__ __launch_bounds__(kHgThreads) void conv_s2_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ gy,
                                                                   float *__restrict__ partial, int H, int W, int Cin, int Cout, int OH,
                                                                   int OW, int K, int pad, int CK, int slabs_x, int co_tiles) {
    __shared__ __attribute__((aligned(16))) float sgy[kCvTile * kCvTile * kCvCout];
    __shared__ float sp[kWgPFloats];
    const int t = threadIdx.x, cg = t & 15, mg = t >> 4;
    const int chunk = blockIdx.y / co_tiles, co0 = (blockIdx.y % co_tiles) * kCvCout, b = blockIdx.z;
    const int c0 = chunk * CK, ck = min(CK, Cin - c0), M = K * K * ck, PW = 2 * kCvTile + K - 2;
    const int oy0 = (blockIdx.x / slabs_x) * kWgSlabRows, sx0 = (blockIdx.x % slabs_x) * kWgSlabCols;
    // row m of the chunk -> its offset inside the patch of a pixel, and its row of dw: tabulated by loops over the taps (uniform
    // counters and a branch; a per-lane m / ck would assemble to compares kept for selects)
    __shared__ int s_off[16 * kWgRows], s_row[16 * kWgRows];
    for (int ky = 0, kk = 0; ky < K; ++ky)
        for (int kx = 0; kx < K; ++kx, ++kk)
            if (t < ck) {
                s_off[kk * ck + t] = (ky * PW + kx) * ck + t;
                s_row[kk * ck + t] = kk * Cin + c0 + t;
            }
    __syncthreads();
    int off[kWgRows];
#pragma unroll
    for (int r = 0; r < kWgRows; ++r) off[r] = s_off[min(mg + 16 * r, M - 1)];
    float acc[kWgRows][4], bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < kWgRows; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[r][j] = 0.f;
    for (int ox0 = sx0; ox0 < min(OW, sx0 + kWgSlabCols); ox0 += kCvTile) {
        __syncthreads();
        for (int i = t; i < kCvTile * kCvTile * (kCvCout / 4); i += kHgThreads) {
            const int p = i / (kCvCout / 4), c4 = i % (kCvCout / 4);
            const int oy = oy0 + p / kCvTile, ox = ox0 + p % kCvTile;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (oy < OH && ox < OW) v = *reinterpret_cast<const float4 *>(gy + (((long long)b * OH + oy) * OW + ox) * Cout + co0 + c4 * 4);
            *reinterpret_cast<float4 *>(sgy + i * 4) = v;
        }
        const int np = PW * PW * ck, iy0 = 2 * oy0 - pad, ix0 = 2 * ox0 - pad;
        for (int i = t; i < np; i += kHgThreads) {
            const int ci = i % ck, r = i / ck, px = r % PW, py = r / PW;
            const int iy = iy0 + py, ix = ix0 + px;
            float v = 0.f;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[(((long long)b * H + iy) * W + ix) * Cin + c0 + ci];
            sp[i] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int py = 0; py < kCvTile; ++py) {
#pragma unroll 2
            for (int px = 0; px < kCvTile; ++px) {
                const float4 g = *reinterpret_cast<const float4 *>(sgy + (py * kCvTile + px) * kCvCout + cg * 4);
                const float *xp = sp + (2 * py * PW + 2 * px) * ck;
                bsum[0] += g.x; bsum[1] += g.y; bsum[2] += g.z; bsum[3] += g.w;
#pragma unroll
                for (int r = 0; r < kWgRows; ++r) {
                    const float xv = xp[off[r]];
                    acc[r][0] = fmaf(xv, g.x, acc[r][0]);
                    acc[r][1] = fmaf(xv, g.y, acc[r][1]);
                    acc[r][2] = fmaf(xv, g.z, acc[r][2]);
                    acc[r][3] = fmaf(xv, g.w, acc[r][3]);
                }
            }
        }
    }
    const long long rows = (long long)K * K * Cin + 1;
    float *dst = partial + ((long long)b * gridDim.x + blockIdx.x) * rows * Cout + co0 + cg * 4;
#pragma unroll
    for (int r = 0; r < kWgRows; ++r) {
        const int m = mg + 16 * r;
        if (m < M) *reinterpret_cast<float4 *>(dst + (long long)s_row[m] * Cout) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    }
    if (chunk == 0 && mg == 0) *reinterpret_cast<float4 *>(dst + (rows - 1) * Cout) = make_float4(bsum[0], bsum[1], bsum[2], bsum[3]);
}

// one thread per float4 of (dw, dbias) = the K K Cin + 1 rows of a slab: the slabs added in ascending order from +0
__global__ __launch_bounds__(kHgThreads) void conv_s2_wgrad_reduce_kernel(const float *__restrict__ partial, int slabs, long long total4,
                                                                          long long dw4, float *__restrict__ dw, float *__restrict__ dbias) {
    const long long i = (long long)blockIdx.x * kHgThreads + threadIdx.x;
    if (i >= total4) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 *src = reinterpret_cast<const float4 *>(partial) + i;
#pragma unroll 4
    for (int k = 0; k < slabs; ++k) {
        const float4 v = src[(long long)k * total4];
        s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
    }
    if (i < dw4) *reinterpret_cast<float4 *>(dw + i * 4) = s;
    else if (dbias) *reinterpret_cast<float4 *>(dbias + (i - dw4) * 4) = s;
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned blocks_of(long long total) { return (unsigned)((total + kHgThreads - 1) / kHgThreads); }

// pixels of one sample a statistics workgroup reads, and how many workgroups a sample takes
inline int gn_chunk_pixels(int C) { return kGnChunkFloats / C; }
inline int gn_chunks(long long HW, int C) { return (int)((HW + gn_chunk_pixels(C) - 1) / gn_chunk_pixels(C)); }

int check_plane(const char *what, int B, int H, int W, int C) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || C < 4 || C % 4 != 0) return fail(T2H_ERR_ARG, "%s: bad shape B=%d H=%d W=%d C=%d (C %% 4 == 0)", what, B, H, W, C);
    if ((long long)B * H * W * C > (1LL << 40) || (long long)H * W > (1LL << 30)) return fail(T2H_ERR_ARG, "%s: plane too large", what);
    return T2H_OK;
}

bool gn_ok(int B, int H, int W, int C, int G) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= (1LL << 30) && C >= 4 && C % 4 == 0 && C <= 4 * kHgThreads &&
           G >= 1 && C % G == 0 && (long long)H * W * (C / G) <= (1LL << 24);
}

// what the GroupNorm backward takes: the forward's shapes with at most 256 channels per group
bool gnb_ok(int B, int H, int W, int C, int G) { return gn_ok(B, H, W, C, G) && C / G <= kGnbMaxCpg; }
inline int gnb_chunks(long long HW) { return (int)((HW + kGnbPixels - 1) / kGnbPixels); }

// the domain of t2h_hg_conv_s2_fwd, for its two adjoints
int check_conv_s2(const char *what, int B, int H, int W, int Cin, int Cout, int K, int pad) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768 || Cin < 1 || Cin > 4096)
        return fail(T2H_ERR_ARG, "%s: bad shape B=%d H=%d W=%d Cin=%d", what, B, H, W, Cin);
    if (K < 1 || K > 7 || K % 2 == 0 || pad < 0 || pad > K / 2 || Cout < kCvCout || Cout % kCvCout != 0 || Cout / kCvCout > 65535)
        return fail(T2H_ERR_ARG, "%s: no kernel for K=%d pad=%d Cout=%d (K odd <= 7, pad <= K / 2, Cout %% 64 == 0)", what, K, pad, Cout);
    if (H + 2 * pad < K || W + 2 * pad < K) return fail(T2H_ERR_ARG, "%s: the plane is smaller than the kernel", what);
    return T2H_OK;
}

}  // namespace
}  // namespace t2h

using namespace t2h;

T2H_API size_t t2h_hg_groupnorm_workspace_bytes(int B, int H, int W, int C, int G) {
    if (!gn_ok(B, H, W, C, G)) return 0;
    const int chunks = gn_chunks((long long)H * W, C);
    return chunks == 1 ? 1 : (size_t)B * chunks * G * 3 * sizeof(float);
}

T2H_API int t2h_hg_groupnorm_stats(const float *x, int B, int H, int W, int C, int G, float eps, float *stats, void *workspace,
                                   size_t workspace_bytes, t2h_stream_t stream) {
    if (!x || !stats) return fail(T2H_ERR_ARG, "hg_groupnorm_stats: null pointer");
    if (!gn_ok(B, H, W, C, G))
        return fail(T2H_ERR_ARG, "hg_groupnorm_stats: no kernel for B=%d H=%d W=%d C=%d G=%d (C %% 4 == 0, C <= 1024, C %% G == 0, "
                    "at most 2^24 elements per group)", B, H, W, C, G);
    if (!al16(x) || !(eps >= 0.f)) return fail(T2H_ERR_ARG, "hg_groupnorm_stats: x must be 16-byte aligned, eps >= 0");
    const int HW = H * W, chunks = gn_chunks(HW, C);
    if (chunks > 65535 * 32) return fail(T2H_ERR_ARG, "hg_groupnorm_stats: plane too large");
    hipStream_t s = as_stream(stream);
    if (chunks == 1) {
        hipLaunchKernelGGL(gn_partial_kernel, dim3(1, B), dim3(kHgThreads), 0, s, x, HW, C, G, gn_chunk_pixels(C), 1, eps, stats);
        note_kernel("gn_partial_kernel");
        return check_launch("hg_groupnorm_stats");
    }
    const size_t need = t2h_hg_groupnorm_workspace_bytes(B, H, W, C, G);
    if (!workspace || workspace_bytes < need || !al16(workspace))
        return fail(T2H_ERR_WORKSPACE, "hg_groupnorm_stats: workspace %zu < %zu bytes", workspace_bytes, need);
    float *partials = static_cast<float *>(workspace);
    hipLaunchKernelGGL(gn_partial_kernel, dim3(chunks, B), dim3(kHgThreads), 0, s, x, HW, C, G, gn_chunk_pixels(C), 0, eps, partials);
    hipLaunchKernelGGL(gn_final_kernel, dim3(blocks_of((long long)B * G)), dim3(kHgThreads), 0, s, partials, B * G, G, chunks, eps, stats);
    note_kernel("gn_partial_kernel");
    return check_launch("hg_groupnorm_stats");
}

T2H_API int t2h_hg_norm_apply(const float *x, const float *stats, const float *scale, const float *shift, int B, int H, int W, int C,
                              int G, int relu, float *y, t2h_stream_t stream) {
    if (!x || !scale || !shift || !y) return fail(T2H_ERR_ARG, "hg_norm_apply: null pointer");
    if (int rc = check_plane("hg_norm_apply", B, H, W, C)) return rc;
    if (stats && (G < 1 || C % G != 0)) return fail(T2H_ERR_ARG, "hg_norm_apply: C=%d is not a multiple of G=%d", C, G);
    if (!al16(x) || !al16(scale) || !al16(shift) || !al16(y)) return fail(T2H_ERR_ARG, "hg_norm_apply: pointers must be 16-byte aligned");
    const long long total4 = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(norm_apply_kernel, dim3(blocks_of(total4)), dim3(kHgThreads), 0, as_stream(stream), x, stats, scale, shift, total4,
                       H * W, C, stats ? G : 1, relu ? 1 : 0, y);
    note_kernel("norm_apply_kernel");
    return check_launch("hg_norm_apply");
}

T2H_API int t2h_hg_conv_s2_fwd(const float *x, const float *w, const float *bias, float *y, int B, int H, int W, int Cin, int Cout,
                               int K, int pad, t2h_stream_t stream) {
    if (!x || !w || !y) return fail(T2H_ERR_ARG, "hg_conv_s2_fwd: null pointer");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 32768 || W > 32768 || Cin < 1 || Cin > 4096)
        return fail(T2H_ERR_ARG, "hg_conv_s2_fwd: bad shape B=%d H=%d W=%d Cin=%d", B, H, W, Cin);
    if (K < 1 || K > 7 || K % 2 == 0 || pad < 0 || pad > K / 2 || Cout < kCvCout || Cout % kCvCout != 0 || Cout / kCvCout > 65535)
        return fail(T2H_ERR_ARG, "hg_conv_s2_fwd: no kernel for K=%d pad=%d Cout=%d (K odd <= 7, pad <= K / 2, Cout %% 64 == 0)", K, pad, Cout);
    if (H + 2 * pad < K || W + 2 * pad < K) return fail(T2H_ERR_ARG, "hg_conv_s2_fwd: the plane is smaller than the kernel");
    if (!al16(w) || !al16(y) || (bias && !al16(bias)) || ((uintptr_t)x & 3)) return fail(T2H_ERR_ARG, "hg_conv_s2_fwd: w, bias, y must be 16-byte aligned");
    const int OH = (H + 2 * pad - K) / 2 + 1, OW = (W + 2 * pad - K) / 2 + 1;
    const int PW = 2 * kCvTile + K - 2;
    int CK = Cin;
    if (CK > kCvWMax / (K * K * kCvCout)) CK = kCvWMax / (K * K * kCvCout);
    if (CK > kCvPMax / (PW * PW)) CK = kCvPMax / (PW * PW);
    if (CK < 1) return fail(T2H_ERR_ARG, "hg_conv_s2_fwd: K=%d does not fit the staging buffers", K);
    const int tiles_x = (OW + kCvTile - 1) / kCvTile, tiles_y = (OH + kCvTile - 1) / kCvTile;
    hipLaunchKernelGGL(conv_s2_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)(Cout / kCvCout), (unsigned)B), dim3(kHgThreads), 0,
                       as_stream(stream), x, w, bias, y, H, W, Cin, Cout, OH, OW, K, pad, CK, tiles_x);
    note_kernel("conv_s2_kernel");
    return check_launch("hg_conv_s2_fwd");
}

T2H_API int t2h_hg_avgpool2x2(const float *x, int B, int H, int W, int C, float *y, t2h_stream_t stream) {
    if (!x || !y) return fail(T2H_ERR_ARG, "hg_avgpool2x2: null pointer");
    if (int rc = check_plane("hg_avgpool2x2", B, H, W, C)) return rc;
    if (H < 2 || W < 2) return fail(T2H_ERR_ARG, "hg_avgpool2x2: H=%d, W=%d must be at least 2", H, W);
    if (!al16(x) || !al16(y)) return fail(T2H_ERR_ARG, "hg_avgpool2x2: pointers must be 16-byte aligned");
    const long long total4 = (long long)B * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(avgpool2x2_kernel, dim3(blocks_of(total4)), dim3(kHgThreads), 0, as_stream(stream), x, total4, H, W, C, y);
    note_kernel("avgpool2x2_kernel");
    return check_launch("hg_avgpool2x2");
}

T2H_API int t2h_hg_block_tail(const float *o1, const float *o2, const float *o3, const float *res, int64_t P, int C, float *y,
                              t2h_stream_t stream) {
    if (!o1 || !o2 || !o3 || !res || !y) return fail(T2H_ERR_ARG, "hg_block_tail: null pointer");
    if (P < 1 || C < 16 || C % 16 != 0 || P * (int64_t)C > (1LL << 40)) return fail(T2H_ERR_ARG, "hg_block_tail: bad shape P=%lld C=%d (C %% 16 == 0)", (long long)P, C);
    if (!al16(o1) || !al16(o2) || !al16(o3) || !al16(res) || !al16(y)) return fail(T2H_ERR_ARG, "hg_block_tail: pointers must be 16-byte aligned");
    const long long total4 = (long long)P * (C / 4);
    hipLaunchKernelGGL(block_tail_kernel, dim3(blocks_of(total4)), dim3(kHgThreads), 0, as_stream(stream), o1, o2, o3, res, total4, C, y);
    note_kernel("block_tail_kernel");
    return check_launch("hg_block_tail");
}

T2H_API int t2h_hg_groupnorm_bwd_reduce(const float *gy, const float *y, const float *x, const float *stats, const float *gamma, int B,
                                        int H, int W, int C, int G, float *partial, float *gsum, float *dbeta, float *dgamma,
                                        t2h_stream_t stream) {
    if (!gy || !x || !stats || !gamma || !partial || !gsum || !dbeta || !dgamma) return fail(T2H_ERR_ARG, "hg_groupnorm_bwd_reduce: null pointer");
    if (!gnb_ok(B, H, W, C, G))
        return fail(T2H_ERR_ARG, "hg_groupnorm_bwd_reduce: no kernel for B=%d H=%d W=%d C=%d G=%d (C %% 4 == 0, C <= 1024, C %% G == 0, "
                    "C / G <= 256, at most 2^24 elements per group)", B, H, W, C, G);
    if (!al16(gy) || (y && !al16(y)) || !al16(x) || !al16(partial)) return fail(T2H_ERR_ARG, "hg_groupnorm_bwd_reduce: gy, y, x, partial must be 16-byte aligned");
    const int HW = H * W, chunks = gnb_chunks(HW), cpg = C / G, cb = (kHgThreads / cpg) * cpg;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(kHgThreads), 0, s, gy, y ? y : gy, x, stats, HW, C, G,
                       y ? 0u : 0xffffffffu, partial);
    hipLaunchKernelGGL(gn_bwd_finish_kernel, dim3((unsigned)((C + cb - 1) / cb)), dim3(kHgThreads), 0, s, partial, gamma, B, chunks, C, G, cb,
                       gsum, dbeta, dgamma);
    note_kernel("gn_bwd_partial_kernel");
    return check_launch("hg_groupnorm_bwd_reduce");
}

T2H_API int t2h_hg_groupnorm_bwd_apply(const float *gy, const float *y, const float *x, const float *stats, const float *gamma,
                                       const float *gsum, const float *addend, int B, int H, int W, int C, int G, float *dx,
                                       t2h_stream_t stream) {
    if (!gy || !x || !stats || !gamma || !gsum || !dx) return fail(T2H_ERR_ARG, "hg_groupnorm_bwd_apply: null pointer");
    if (!gnb_ok(B, H, W, C, G))
        return fail(T2H_ERR_ARG, "hg_groupnorm_bwd_apply: no kernel for B=%d H=%d W=%d C=%d G=%d (C %% 4 == 0, C <= 1024, C %% G == 0, "
                    "C / G <= 256, at most 2^24 elements per group)", B, H, W, C, G);
    if (!al16(gy) || (y && !al16(y)) || !al16(x) || !al16(gamma) || (addend && !al16(addend)) || !al16(dx))
        return fail(T2H_ERR_ARG, "hg_groupnorm_bwd_apply: gy, y, x, gamma, addend, dx must be 16-byte aligned");
    const long long total4 = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(blocks_of(total4)), dim3(kHgThreads), 0, as_stream(stream), gy, y ? y : gy, x, stats, gamma,
                       gsum, addend, total4, H * W, C, G, y ? 0u : 0xffffffffu, dx);
    note_kernel("gn_bwd_apply_kernel");
    return check_launch("hg_groupnorm_bwd_apply");
}

T2H_API int t2h_hg_avgpool2x2_bwd(const float *gy, int B, int H, int W, int C, float *dx, t2h_stream_t stream) {
    if (!gy || !dx) return fail(T2H_ERR_ARG, "hg_avgpool2x2_bwd: null pointer");
    if (int rc = check_plane("hg_avgpool2x2_bwd", B, H, W, C)) return rc;
    if (H < 2 || W < 2 || H % 2 != 0 || W % 2 != 0) return fail(T2H_ERR_ARG, "hg_avgpool2x2_bwd: H=%d, W=%d must be even, at least 2", H, W);
    if (!al16(gy) || !al16(dx)) return fail(T2H_ERR_ARG, "hg_avgpool2x2_bwd: pointers must be 16-byte aligned");
    const long long total4 = (long long)B * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(avgpool2x2_bwd_kernel, dim3(blocks_of(total4)), dim3(kHgThreads), 0, as_stream(stream), gy, total4, H, W, C, dx);
    note_kernel("avgpool2x2_bwd_kernel");
    return check_launch("hg_avgpool2x2_bwd");
}

T2H_API int t2h_hg_block_tail_bwd(const float *g, int64_t P, int C, float *d1, float *d2, float *d3, t2h_stream_t stream) {
    if (!g || !d1 || !d2 || !d3) return fail(T2H_ERR_ARG, "hg_block_tail_bwd: null pointer");
    if (P < 1 || C < 16 || C % 16 != 0 || P * (int64_t)C > (1LL << 40)) return fail(T2H_ERR_ARG, "hg_block_tail_bwd: bad shape P=%lld C=%d (C %% 16 == 0)", (long long)P, C);
    if (!al16(g) || !al16(d1) || !al16(d2) || !al16(d3)) return fail(T2H_ERR_ARG, "hg_block_tail_bwd: pointers must be 16-byte aligned");
    const long long total4 = (long long)P * (C / 4);
    hipLaunchKernelGGL(block_tail_bwd_kernel, dim3(blocks_of(total4)), dim3(kHgThreads), 0, as_stream(stream), g, total4, C, d1, d2, d3);
    note_kernel("block_tail_bwd_kernel");
    return check_launch("hg_block_tail_bwd");
}

T2H_API int t2h_hg_conv_s2_dgrad(const float *gy, const float *w, const float *addend, float *dx, int B, int H, int W, int Cin, int Cout,
                                 int K, int pad, t2h_stream_t stream) {
    if (!gy || !w || !dx) return fail(T2H_ERR_ARG, "hg_conv_s2_dgrad: null pointer");
    if (int rc = check_conv_s2("hg_conv_s2_dgrad", B, H, W, Cin, Cout, K, pad)) return rc;
    if (!al16(gy) || !al16(w) || ((uintptr_t)dx & 3) || ((uintptr_t)addend & 3) || (Cin % 4 == 0 && (!al16(dx) || !al16(addend))))
        return fail(T2H_ERR_ARG, "hg_conv_s2_dgrad: gy, w (and, Cin %% 4 == 0, dx and addend) must be 16-byte aligned");
    const int OH = (H + 2 * pad - K) / 2 + 1, OW = (W + 2 * pad - K) / 2 + 1, A = (K + 1) / 2;
    const bool wide = Cin > 16;                          // lanes over channels (64 per workgroup), else lanes over pixels (4)
    const int S = wide ? 4 : 16, WS = (wide ? 64 : 4) + 4;
    int CK = 16;
    while (CK > 1 && (K * K * CK * WS > kDgWFloats || (S + A - 1) * (2 * S + A - 1) * (CK | 1) > kDgPFloats)) CK >>= 1;
    if (K * K * CK * WS > kDgWFloats || (S + A - 1) * (2 * S + A - 1) * (CK | 1) > kDgPFloats)
        return fail(T2H_ERR_ARG, "hg_conv_s2_dgrad: K=%d does not fit the staging buffers", K);
    const int qy = (H + pad - 1) / 2 + 1, qx = (W + pad - 1) / 2 + 1;          // q-blocks that hold a pixel of the plane
    const int tiles_y = (qy + S - 1) / S, tiles_x = (qx + 2 * S - 1) / (2 * S), cit = wide ? 64 : 4;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)((Cin + cit - 1) / cit), (unsigned)B);
    if (wide)
        hipLaunchKernelGGL(conv_s2_dgrad_kernel<16>, grid, dim3(kHgThreads), 0, as_stream(stream), gy, w, addend, dx, H, W, Cin, Cout, OH, OW,
                           K, pad, CK, tiles_x, Cin % 4 == 0 ? 1 : 0);
    else
        hipLaunchKernelGGL(conv_s2_dgrad_kernel<1>, grid, dim3(kHgThreads), 0, as_stream(stream), gy, w, addend, dx, H, W, Cin, Cout, OH, OW,
                           K, pad, CK, tiles_x, Cin % 4 == 0 ? 1 : 0);
    note_kernel("conv_s2_dgrad_kernel");
    return check_launch("hg_conv_s2_dgrad");
}

T2H_API int t2h_hg_conv_s2_wgrad(const float *x, const float *gy, float *partial, float *dw, float *dbias, int B, int H, int W, int Cin,
                                 int Cout, int K, int pad, t2h_stream_t stream) {
    if (!x || !gy || !partial || !dw) return fail(T2H_ERR_ARG, "hg_conv_s2_wgrad: null pointer");
    if (int rc = check_conv_s2("hg_conv_s2_wgrad", B, H, W, Cin, Cout, K, pad)) return rc;
    if (!al16(gy) || !al16(partial) || !al16(dw) || (dbias && !al16(dbias)) || ((uintptr_t)x & 3))
        return fail(T2H_ERR_ARG, "hg_conv_s2_wgrad: gy, partial, dw, dbias must be 16-byte aligned");
    const int OH = (H + 2 * pad - K) / 2 + 1, OW = (W + 2 * pad - K) / 2 + 1, PW = 2 * kCvTile + K - 2;
    int CK = 16 * kWgRows / (K * K);
    if (CK > 16) CK = 16;
    if (CK > Cin) CK = Cin;
    if (CK < 1 || PW * PW * CK > kWgPFloats) return fail(T2H_ERR_ARG, "hg_conv_s2_wgrad: K=%d does not fit the staging buffers", K);
    const int slabs_y = (OH + kWgSlabRows - 1) / kWgSlabRows, slabs_x = (OW + kWgSlabCols - 1) / kWgSlabCols;
    const int chunks = (Cin + CK - 1) / CK, co_tiles = Cout / kCvCout;
    const long long slabs = (long long)B * slabs_y * slabs_x, total4 = ((long long)K * K * Cin + 1) * (Cout / 4);
    if ((long long)chunks * co_tiles > 65535 || slabs > (1 << 24) || total4 > (1LL << 31) * kHgThreads / 2)
        return fail(T2H_ERR_ARG, "hg_conv_s2_wgrad: shape too large (B=%d H=%d W=%d Cin=%d Cout=%d)", B, H, W, Cin, Cout);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(conv_s2_wgrad_kernel, dim3((unsigned)(slabs_y * slabs_x), (unsigned)(chunks * co_tiles), (unsigned)B), dim3(kHgThreads), 0,
                       s, x, gy, partial, H, W, Cin, Cout, OH, OW, K, pad, CK, slabs_x, co_tiles);
    hipLaunchKernelGGL(conv_s2_wgrad_reduce_kernel, dim3(blocks_of(total4)), dim3(kHgThreads), 0, s, partial, (int)slabs, total4,
                       (long long)K * K * Cin * (Cout / 4), dw, dbias);
    note_kernel("conv_s2_wgrad_kernel");
    return check_launch("hg_conv_s2_wgrad");
}
