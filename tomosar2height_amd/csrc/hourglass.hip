// The hourglass image encoder's own kernels (include/t2h_hg.h; reference: tomosar2height/encoder/hourglass.py): GroupNorm
// statistics and apply, the direct stride-2 convolution (the 7 x 7 stem and the 3 x 3 hg_down = 'conv64' / 'conv128' layer), the
// 2 x 2 average pool and the ConvBlock tail cat(out1, out2, out3) + residual.  Forward only.  fp32 NHWC throughout, 16-byte
// accesses along C wherever C % 4 == 0 is required.
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
#include <math.h>

#include "t2h_common.h"
#include "../../include/t2h_hg.h"

namespace t2h {

constexpr int kHgThreads = 256;
constexpr int kGnChunkFloats = 65536;          // floats of one sample a statistics workgroup reads

constexpr int kCvTile = 8;                     // output tile of the strided convolution: 8 x 8 pixels x 64 channels per workgroup
constexpr int kCvCout = 64;
constexpr int kCvWMax = 7 * 7 * 3 * kCvCout;   // floats of weights staged at a time: the whole 7 x 7 x 3 stem, 16 channels of a 3 x 3
constexpr int kCvPMax = 17 * 17 * 16;          // floats of input patch staged at a time (3 x 3: 17 x 17 x 16; 7 x 7: 21 x 21 x 3)

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
