// DSM evaluation on the device (reference: evaluator.py:14-99, utils/dilate_mask.py; ABI in include/t2h_eval.h).
//
// Once per evaluator: predicate planes (`.astype(bool)`, `type == v`, `type > 0`), their dilations (one pass with the L1 ball
// of radius k = k iterations of scipy's cross element, border 0) and ONE uint16 plane of class bits (bit 0 = gt_mask =
// 'overall', bit c = gt_mask & mask_c).  Per eval: the float64 residual plane `diff` (NaN outside gt_mask) and the windowed
// class plane `cw` (0 where the residual is NaN), then every statistic of every class from those two planes, 10 B per pixel
// and pass, nothing compacted per class:
//
//   * n, min, max, sum |r|, sum r^2: one pass, float64 accumulators per thread (at most 2 048 terms each), a fixed shuffle /
//     LDS tree per workgroup into a slab, the slab reduced by one workgroup per class in a fixed order.  No floating-point
//     atomics anywhere: two runs give the same bytes.
//   * median(r), median(|r|), then median(|r - median(r)|): most-significant-digit radix select over the order-preserving
//     64-bit image of the float64 value (sign bit flipped for non-negatives, all bits for negatives).  A pass histograms one
//     digit of the keys that still match the prefix chosen so far -- all classes, both middle ranks ((n-1)/2 and n/2) and
//     both key streams of a round from ONE read of the planes -- into per-workgroup LDS histograms with integer LDS atomics
//     (order-independent, hence deterministic), merged into a global 64-bit histogram with integer atomics; a one-wave scan
//     launch per (class, stream) then picks the digit and the remaining rank on the device.  The host never waits.
//
// Digit width.  The LDS histograms are classes x streams x ranks x bins x 4 B.  With 8-bit digits and the full 16 classes
// that is 16 x 2 x 2 x 256 x 4 B = 64 KB: it fits the 64 KB a workgroup gets without opting into more, two workgroups per
// CU (160 KB).  11-bit digits (6 passes instead of 8) would need 512 KB at 16 classes, and still 224 KB at the 7 Berlin
// classes; splitting the classes over several reads of the planes to make it fit costs more than the two passes it saves,
// since a pass over a plane that stays in the Infinity Cache is about as long as its launch.  So: 8 bits, 8 passes per
// round, two rounds.  While the two middle ranks still share their prefix (always, for odd n) only the first rank's
// histogram is filled and the scan reads it for both.
//
// Compare results and vector selects: the evaluator is not issued beside a training step on any
// shipped path, so the rule for kernels that share a CU with the split convolutions does not bind here.  Where a mask is
// free by arithmetic it is made that way (class membership in the statistics pass is an integer AND with 0 - bit); the
// prefix tests of the select are plain compares used at once.
#include <math.h>

#include "dsm_common.h"
#include "../../include/t2h_eval.h"

namespace t2h {

constexpr int kEvalClasses = T2H_EVAL_MAX_CLASSES;
constexpr int kEvalBins = 256;                                   // 8-bit digits
constexpr int kEvalPasses = 8;                                   // per round
constexpr int kEvalCombos = kEvalClasses * 2 * 2;                // [class][stream][rank]
constexpr int kEvalHistBins = kEvalCombos * kEvalBins;           // one pass's global histogram (u64 bins)
constexpr int kEvalStatFields = 5;                               // n, min, max, sum |r|, sum r^2
constexpr int kEvalStatWgsCap = 2048, kEvalSelectWgsCap = 512, kEvalChunkCap = 2048;

struct EvalState {                                               // lives in the workspace, written by the kernels only
    u64 prefix[2][kEvalCombos];                                  // [round][(class * S + stream) * 2 + rank]: digits chosen so far
    u64 rank[2][kEvalCombos];                                    // rank still to find among the keys that match the prefix
    u64 cnt[kEvalClasses];
    double med[kEvalClasses];
};

// ------------------------------------------------------------------------------------------ construction-time planes
template <typename T>
__global__ __launch_bounds__(256) void eval_predicate_kernel(const T *__restrict__ src, int op, double value,
                                                             uint8_t *__restrict__ out, long long n) {
    long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        double v = (double)src[i];
        out[i] = op == T2H_EVAL_NONZERO ? v != 0.0 : op == T2H_EVAL_EQ ? v == value : v > value;
    }
}

__global__ __launch_bounds__(256) void eval_dilate_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int R,
                                                          int C, int k) {
    int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= C) return;
    for (int y = blockIdx.y; y < R; y += gridDim.y) {
        unsigned hit = 0;
        int y0 = max(y - k, 0), y1 = min(y + k, R - 1);
        for (int yy = y0; yy <= y1; ++yy) {
            int w = k - abs(yy - y);                              // the L1 ball's half width on this row
            int x0 = max(x - w, 0), x1 = min(x + w, C - 1);
            const uint8_t *row = in + (size_t)yy * C;
            for (int xx = x0; xx <= x1; ++xx) hit |= row[xx];
        }
        out[(size_t)y * C + x] = hit != 0;
    }
}

__global__ __launch_bounds__(256) void eval_class_bits_kernel(const uint8_t *__restrict__ mask, int invert,
                                                              const uint8_t *__restrict__ gt_mask, int bit,
                                                              uint16_t *__restrict__ cls, long long n) {
    long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        unsigned m = mask ? mask[i] != 0 : 1u, g = gt_mask ? gt_mask[i] != 0 : 1u;
        unsigned v = (g & (m ^ (unsigned)invert)) << bit;
        cls[i] = (uint16_t)(bit == 0 ? v : cls[i] | v);
    }
}

// ------------------------------------------------------------------------------------------ per eval: residual plane
template <typename TT, typename TG>
__global__ __launch_bounds__(256) void eval_residual_kernel(const TT *__restrict__ target, int H, int W,
                                                            const TG *__restrict__ gt, const uint16_t *__restrict__ cls,
                                                            int C, int t_row, int l_col, double *__restrict__ diff,
                                                            uint16_t *__restrict__ cw) {
    int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        size_t o = (size_t)y * W + x, g = (size_t)(t_row + y) * C + (l_col + x);
        double r = (double)target[o] - (double)gt[g];
        unsigned bits = cls[g];
        diff[o] = (bits & 1u) ? r : __longlong_as_double(0x7ff8000000000000ll);
        cw[o] = (uint16_t)(isnan(r) ? 0u : bits);
    }
}

// ------------------------------------------------------------------------------------------ sums, extrema, counts
template <int NC> struct EvalAcc {
    double mn[NC], mx[NC], sa[NC], sq[NC];
    u64 cnt[NC];
    __device__ void init() {
#pragma unroll
        for (int c = 0; c < NC; ++c) { mn[c] = INFINITY; mx[c] = -INFINITY; sa[c] = 0.0; sq[c] = 0.0; cnt[c] = 0; }
    }
    __device__ void take(double r, unsigned bits) {
        const u64 rb = (u64)__double_as_longlong(r);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            u64 m = 0ull - (u64)((bits >> c) & 1u);              // all ones for a member (a NaN residual has bits == 0)
            u64 in = rb & m;
            double rc = __longlong_as_double((long long)in);     // +0.0 for a non-member: adds nothing to either sum
            cnt[c] += m & 1ull;
            sa[c] += fabs(rc);
            sq[c] += rc * rc;
            mn[c] = fmin(mn[c], __longlong_as_double((long long)(in | (~m & 0x7ff0000000000000ull))));
            mx[c] = fmax(mx[c], __longlong_as_double((long long)(in | (~m & 0xfff0000000000000ull))));
        }
    }
};

template <int NC>
__global__ __launch_bounds__(256) void eval_stats_kernel(const double *__restrict__ diff, const uint16_t *__restrict__ cw,
                                                         long long n, double *__restrict__ slab) {
    __shared__ double red[4][NC * kEvalStatFields];
    EvalAcc<NC> a;
    a.init();
    const long long pairs = n >> 1, stride = (long long)gridDim.x * 256, gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const double2 *d2 = reinterpret_cast<const double2 *>(diff);
    const unsigned *c2 = reinterpret_cast<const unsigned *>(cw);
    for (long long i = gid; i < pairs; i += stride) {
        double2 r = d2[i];
        unsigned b = c2[i];
        a.take(r.x, b & 0xffffu);
        a.take(r.y, b >> 16);
    }
    if ((n & 1) && gid == 0) a.take(diff[n - 1], cw[n - 1]);
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {                 // fixed tree inside the wave
            a.cnt[c] += __shfl_down(a.cnt[c], off);
            a.mn[c] = fmin(a.mn[c], __shfl_down(a.mn[c], off));
            a.mx[c] = fmax(a.mx[c], __shfl_down(a.mx[c], off));
            a.sa[c] += __shfl_down(a.sa[c], off);
            a.sq[c] += __shfl_down(a.sq[c], off);
        }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double *o = &red[wave][c * kEvalStatFields];
            o[0] = __longlong_as_double((long long)a.cnt[c]); o[1] = a.mn[c]; o[2] = a.mx[c]; o[3] = a.sa[c]; o[4] = a.sq[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < NC * kEvalStatFields) {                     // the four waves, in order
        int f = threadIdx.x % kEvalStatFields, c = threadIdx.x / kEvalStatFields;
        double v = red[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) {
            double u = red[w][threadIdx.x];
            if (f == 0) v = __longlong_as_double(__double_as_longlong(v) + __double_as_longlong(u));
            else if (f == 1) v = fmin(v, u);
            else if (f == 2) v = fmax(v, u);
            else v += u;
        }
        slab[((size_t)blockIdx.x * kEvalClasses + c) * kEvalStatFields + f] = v;
    }
}

// one workgroup per class: the slab's workgroups strided over the threads (in order), then a fixed LDS tree
__global__ __launch_bounds__(256) void eval_stats_finalize_kernel(const double *__restrict__ slab, int wgs,
                                                                  double *__restrict__ table, EvalState *__restrict__ st) {
    __shared__ double red[256][kEvalStatFields];
    const int c = blockIdx.x, t = threadIdx.x;
    u64 cnt = 0;
    double mn = INFINITY, mx = -INFINITY, sa = 0.0, sq = 0.0;
    for (int g = t; g < wgs; g += 256) {
        const double *p = slab + ((size_t)g * kEvalClasses + c) * kEvalStatFields;
        cnt += (u64)__double_as_longlong(p[0]);
        mn = fmin(mn, p[1]); mx = fmax(mx, p[2]); sa += p[3]; sq += p[4];
    }
    red[t][0] = __longlong_as_double((long long)cnt); red[t][1] = mn; red[t][2] = mx; red[t][3] = sa; red[t][4] = sq;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) {
            red[t][0] = __longlong_as_double(__double_as_longlong(red[t][0]) + __double_as_longlong(red[t + off][0]));
            red[t][1] = fmin(red[t][1], red[t + off][1]);
            red[t][2] = fmax(red[t][2], red[t + off][2]);
            red[t][3] += red[t + off][3];
            red[t][4] += red[t + off][4];
        }
        __syncthreads();
    }
    if (t == 0) {
        double *o = table + (size_t)c * T2H_EVAL_TABLE_COLS;
        for (int f = 0; f < kEvalStatFields; ++f) o[f] = red[0][f];
        o[5] = o[6] = o[7] = 0.0;
        u64 nn = (u64)__double_as_longlong(red[0][0]);
        st->cnt[c] = nn;
        st->med[c] = 0.0;
        for (int s = 0; s < 2; ++s) {                             // round 1: streams r and |r|, ranks (n-1)/2 and n/2
            int i = (c * 2 + s) * 2;
            st->prefix[0][i] = st->prefix[0][i + 1] = 0;
            st->rank[0][i] = nn ? (nn - 1) >> 1 : 0;
            st->rank[0][i + 1] = nn >> 1;
        }
    }
}

// ------------------------------------------------------------------------------------------ radix select
// ROUND 0: keys of r (stream 0) and |r| (stream 1).  ROUND 1: keys of |r - med[class]| (one stream).
template <int ROUND>
__global__ __launch_bounds__(256) void eval_select_pass_kernel(const double *__restrict__ diff,
                                                               const uint16_t *__restrict__ cw, long long n, int ncls,
                                                               int pass, const EvalState *__restrict__ st,
                                                               u64 *__restrict__ ghist) {
    extern __shared__ unsigned hist[];
    constexpr int S = ROUND == 0 ? 2 : 1;
    const int bins = ncls * S * 2 * kEvalBins;
    for (int i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const u64 *__restrict__ prefix = st->prefix[ROUND];

    auto take = [&](double r, unsigned bits) {
        if (bits == 0) return;
        u64 key[2];
        if (ROUND == 0) { key[0] = key64(r); key[1] = key64(fabs(r)); }
        for (int c = 0; c < ncls; ++c) {
            if (!((bits >> c) & 1u)) continue;
            if (ROUND == 1) key[0] = key64(fabs(r - st->med[c]));
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int i = (c * S + s) * 2;
                const u64 p0 = prefix[i], p1 = prefix[i + 1];
                const u64 high = (key[s] >> (shift + 7)) >> 1;    // the digits above this pass's (none on pass 0)
                const unsigned digit = (unsigned)(key[s] >> shift) & 255u;
                if (high == p0) atomicAdd(&hist[i * kEvalBins + digit], 1u);
                if (p1 != p0 && high == p1) atomicAdd(&hist[(i + 1) * kEvalBins + digit], 1u);
            }
        }
    };

    const long long pairs = n >> 1, stride = (long long)gridDim.x * 256, gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const double2 *d2 = reinterpret_cast<const double2 *>(diff);
    const unsigned *c2 = reinterpret_cast<const unsigned *>(cw);
    for (long long i = gid; i < pairs; i += stride) {
        double2 r = d2[i];
        unsigned b = c2[i];
        take(r.x, b & 0xffffu);
        take(r.y, b >> 16);
    }
    if ((n & 1) && gid == 0) take(diff[n - 1], cw[n - 1]);
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256) {
        unsigned v = hist[i];
        if (v) atomicAdd(&ghist[i], (u64)v);
    }
}

// one wave per (class, stream): both ranks pick their digit from the merged histogram of the pass
__global__ __launch_bounds__(64) void eval_select_scan_kernel(const u64 *__restrict__ ghist, EvalState *__restrict__ st,
                                                              int round, int S) {
    const int cs = blockIdx.x, c = cs / S, lane = threadIdx.x;
    if (st->cnt[c] == 0) return;
    const int i0 = cs * 2;
    const u64 p[2] = {st->prefix[round][i0], st->prefix[round][i0 + 1]};
    const u64 rk[2] = {st->rank[round][i0], st->rank[round][i0 + 1]};
    for (int k = 0; k < 2; ++k) {
        const int h = (k == 1 && p[1] == p[0]) ? i0 : i0 + k;     // shared prefix: only the first histogram was filled
        const u64 *b = ghist + (size_t)h * kEvalBins + 4 * lane;
        const u64 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
        const u64 own = b0 + b1 + b2 + b3;
        u64 incl = own;
        for (int off = 1; off < 64; off <<= 1) {
            u64 up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        const u64 rank = k ? rk[1] : rk[0], pk = k ? p[1] : p[0];
        const u64 found = __ballot(incl > rank);
        if (found == 0) {                                         // cannot happen while cnt > rank; keep the state sane
            if (lane == 0) st->prefix[round][i0 + k] = pk << 8;
            continue;
        }
        const int first = __ffsll((long long)found) - 1;
        if (lane == first) {
            u64 rem = rank - (incl - own);
            unsigned j = 0;
            if (rem >= b0) { rem -= b0; j = 1;
                if (rem >= b1) { rem -= b1; j = 2;
                    if (rem >= b2) { rem -= b2; j = 3; } } }
            st->prefix[round][i0 + k] = (pk << 8) | (u64)(4 * lane + j);
            st->rank[round][i0 + k] = rem;
        }
    }
}

__device__ inline double eval_middle(u64 klo, u64 khi) {
    double lo = value64(klo), hi = value64(khi);
    return klo == khi ? lo : (lo + hi) / 2.0;
}

// after round 0: median(r), median(|r|) into the table, and the state of round 1
__global__ __launch_bounds__(64) void eval_medians_kernel(EvalState *__restrict__ st, double *__restrict__ table, int ncls) {
    const int c = threadIdx.x;
    if (c >= ncls) return;
    const u64 nn = st->cnt[c];
    double med = 0.0, amed = 0.0;
    if (nn) {
        med = eval_middle(st->prefix[0][c * 4 + 0], st->prefix[0][c * 4 + 1]);
        amed = eval_middle(st->prefix[0][c * 4 + 2], st->prefix[0][c * 4 + 3]);
    }
    table[(size_t)c * T2H_EVAL_TABLE_COLS + 5] = med;
    table[(size_t)c * T2H_EVAL_TABLE_COLS + 6] = amed;
    st->med[c] = med;
    st->prefix[1][c * 2] = st->prefix[1][c * 2 + 1] = 0;
    st->rank[1][c * 2] = nn ? (nn - 1) >> 1 : 0;
    st->rank[1][c * 2 + 1] = nn >> 1;
}

__global__ __launch_bounds__(64) void eval_mad_kernel(const EvalState *__restrict__ st, double *__restrict__ table, int ncls) {
    const int c = threadIdx.x;
    if (c >= ncls) return;
    table[(size_t)c * T2H_EVAL_TABLE_COLS + 7] = st->cnt[c] ? eval_middle(st->prefix[1][c * 2], st->prefix[1][c * 2 + 1]) : 0.0;
}

// ------------------------------------------------------------------------------------------ host side
static int eval_stat_wgs(int64_t n) {
    int64_t pairs = (n + 1) / 2, g = (pairs + 255) / 256;
    if (g > kEvalStatWgsCap) g = kEvalStatWgsCap;
    int64_t need = (n + (int64_t)256 * kEvalChunkCap - 1) / ((int64_t)256 * kEvalChunkCap);   // <= kEvalChunkCap terms per thread
    if (g < need) g = need;
    return (int)(g < 1 ? 1 : g);
}
constexpr size_t kEvalHistBytes = (size_t)2 * kEvalPasses * kEvalHistBins * sizeof(u64);
constexpr size_t kEvalStateBytes = (sizeof(EvalState) + 255) / 256 * 256;
constexpr int64_t kEvalMaxPixels = (int64_t)1 << 40;

}  // namespace t2h

using namespace t2h;

T2H_API int t2h_eval_predicate(const void *src, int kind, int op, double value, uint8_t *out, int64_t n,
                               t2h_stream_t stream) {
    if (!src || !out) return fail(T2H_ERR_ARG, "eval_predicate: null pointer");
    if (n < 1 || n > kEvalMaxPixels) return fail(T2H_ERR_ARG, "eval_predicate: bad size %lld", (long long)n);
    if (kind < T2H_EVAL_U8 || kind > T2H_EVAL_F64 || op < T2H_EVAL_NONZERO || op > T2H_EVAL_GT)
        return fail(T2H_ERR_ARG, "eval_predicate: unknown element kind %d or predicate %d", kind, op);
    dim3 grid(flat_wgs(n, 2048)), block(256);
    hipStream_t s = as_stream(stream);
#define T2H_EVAL_PRED(T) \
    hipLaunchKernelGGL(eval_predicate_kernel<T>, grid, block, 0, s, (const T *)src, op, value, out, (long long)n)
    switch (kind) {
        case T2H_EVAL_U8: T2H_EVAL_PRED(uint8_t); break;
        case T2H_EVAL_I16: T2H_EVAL_PRED(int16_t); break;
        case T2H_EVAL_I32: T2H_EVAL_PRED(int32_t); break;
        case T2H_EVAL_I64: T2H_EVAL_PRED(int64_t); break;
        case T2H_EVAL_F32: T2H_EVAL_PRED(float); break;
        default: T2H_EVAL_PRED(double); break;
    }
#undef T2H_EVAL_PRED
    return check_launch("eval_predicate");
}

T2H_API int t2h_eval_dilate(const uint8_t *in, uint8_t *out, int R, int C, int iterations, t2h_stream_t stream) {
    if (!in || !out) return fail(T2H_ERR_ARG, "eval_dilate: null pointer");
    if (in == out) return fail(T2H_ERR_ARG, "eval_dilate: out must not alias in");
    if (R < 1 || C < 1 || (int64_t)R * C > kEvalMaxPixels) return fail(T2H_ERR_ARG, "eval_dilate: bad shape %d x %d", R, C);
    if (iterations < 1 || iterations > 1024)
        return fail(T2H_ERR_ARG, "eval_dilate: iterations = %d (1 .. 1024; 'until stable' is not built)", iterations);
    hipLaunchKernelGGL(eval_dilate_kernel, dim3((C + 255) / 256, R < 4096 ? R : 4096), dim3(256), 0, as_stream(stream), in, out,
                       R, C, iterations);
    return check_launch("eval_dilate");
}

T2H_API int t2h_eval_class_bits(const uint8_t *mask, int invert, const uint8_t *gt_mask, int bit, uint16_t *cls, int64_t n,
                                t2h_stream_t stream) {
    if (!cls) return fail(T2H_ERR_ARG, "eval_class_bits: null pointer");
    if (n < 1 || n > kEvalMaxPixels) return fail(T2H_ERR_ARG, "eval_class_bits: bad size %lld", (long long)n);
    if (bit < 0 || bit >= T2H_EVAL_MAX_CLASSES || (invert != 0 && invert != 1))
        return fail(T2H_ERR_ARG, "eval_class_bits: bit %d (0 .. %d) / invert %d (0, 1)", bit, T2H_EVAL_MAX_CLASSES - 1, invert);
    hipLaunchKernelGGL(eval_class_bits_kernel, dim3(flat_wgs(n, 2048)), dim3(256), 0, as_stream(stream), mask, invert,
                       gt_mask, bit, cls, (long long)n);
    return check_launch("eval_class_bits");
}

T2H_API int t2h_eval_residual(const void *target, int target_f64, int H, int W, const void *gt, int gt_f64,
                              const uint16_t *cls, int R, int C, int t_row, int l_col, double *diff, uint16_t *cw,
                              t2h_stream_t stream) {
    if (!target || !gt || !cls || !diff || !cw) return fail(T2H_ERR_ARG, "eval_residual: null pointer");
    if (H < 1 || W < 1 || R < 1 || C < 1 || (int64_t)R * C > kEvalMaxPixels)
        return fail(T2H_ERR_ARG, "eval_residual: bad shape");
    if (t_row < 0 || l_col < 0 || (int64_t)t_row + H > R || (int64_t)l_col + W > C)
        return fail(T2H_ERR_ARG, "eval_residual: window rows [%d, %lld) x cols [%d, %lld) is not inside the %d x %d ground truth",
                    t_row, (long long)t_row + H, l_col, (long long)l_col + W, R, C);
    dim3 grid((W + 255) / 256, H < 4096 ? H : 4096), block(256);
    hipStream_t s = as_stream(stream);
#define T2H_EVAL_RES(TT, TG)                                                                                            \
    hipLaunchKernelGGL((eval_residual_kernel<TT, TG>), grid, block, 0, s, (const TT *)target, H, W, (const TG *)gt, cls, C, \
                       t_row, l_col, diff, cw)
    if (target_f64 && gt_f64) T2H_EVAL_RES(double, double);
    else if (target_f64) T2H_EVAL_RES(double, float);
    else if (gt_f64) T2H_EVAL_RES(float, double);
    else T2H_EVAL_RES(float, float);
#undef T2H_EVAL_RES
    return check_launch("eval_residual");
}

T2H_API size_t t2h_eval_stats_workspace_bytes(int64_t n, int ncls) {
    if (n < 1 || n > kEvalMaxPixels || ncls < 1 || ncls > T2H_EVAL_MAX_CLASSES) return 0;
    return kEvalHistBytes + kEvalStateBytes + (size_t)eval_stat_wgs(n) * kEvalClasses * kEvalStatFields * sizeof(double);
}

T2H_API int t2h_eval_stats(const double *diff, const uint16_t *cw, int64_t n, int ncls, double *table, void *workspace,
                           size_t workspace_bytes, t2h_stream_t stream) {
    if (!diff || !cw || !table || !workspace) return fail(T2H_ERR_ARG, "eval_stats: null pointer");
    if (n < 1 || n > kEvalMaxPixels) return fail(T2H_ERR_ARG, "eval_stats: bad size %lld", (long long)n);
    if (ncls < 1 || ncls > T2H_EVAL_MAX_CLASSES)
        return fail(T2H_ERR_ARG, "eval_stats: %d classes (1 .. %d)", ncls, T2H_EVAL_MAX_CLASSES);
    if (((uintptr_t)diff & 15) || ((uintptr_t)cw & 3) || ((uintptr_t)workspace & 15))
        return fail(T2H_ERR_ARG, "eval_stats: diff / workspace must be 16-byte aligned, cw 4-byte aligned");
    size_t need = t2h_eval_stats_workspace_bytes(n, ncls);
    if (workspace_bytes < need)
        return fail(T2H_ERR_WORKSPACE, "eval_stats: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    u64 *hist = reinterpret_cast<u64 *>(workspace);
    EvalState *st = reinterpret_cast<EvalState *>(reinterpret_cast<char *>(workspace) + kEvalHistBytes);
    double *slab = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + kEvalHistBytes + kEvalStateBytes);
    if (hipMemsetAsync(hist, 0, kEvalHistBytes, s) != hipSuccess) return check_launch("eval_stats (histogram clear)");

    const int wgs = eval_stat_wgs(n);
    if (ncls <= 8)
        hipLaunchKernelGGL(eval_stats_kernel<8>, dim3(wgs), dim3(256), 0, s, diff, cw, (long long)n, slab);
    else
        hipLaunchKernelGGL(eval_stats_kernel<16>, dim3(wgs), dim3(256), 0, s, diff, cw, (long long)n, slab);
    hipLaunchKernelGGL(eval_stats_finalize_kernel, dim3(ncls), dim3(256), 0, s, slab, wgs, table, st);

    const int swgs = flat_wgs((n + 1) / 2, kEvalSelectWgsCap);
    for (int round = 0; round < 2; ++round) {
        const int S = round == 0 ? 2 : 1;
        const size_t lds = (size_t)ncls * S * 2 * kEvalBins * sizeof(unsigned);
        for (int pass = 0; pass < kEvalPasses; ++pass) {
            u64 *h = hist + (size_t)(round * kEvalPasses + pass) * kEvalHistBins;
            if (round == 0)
                hipLaunchKernelGGL(eval_select_pass_kernel<0>, dim3(swgs), dim3(256), lds, s, diff, cw, (long long)n, ncls, pass,
                                   st, h);
            else
                hipLaunchKernelGGL(eval_select_pass_kernel<1>, dim3(swgs), dim3(256), lds, s, diff, cw, (long long)n, ncls, pass,
                                   st, h);
            hipLaunchKernelGGL(eval_select_scan_kernel, dim3(ncls * S), dim3(64), 0, s, h, st, round, S);
        }
        if (round == 0)
            hipLaunchKernelGGL(eval_medians_kernel, dim3(1), dim3(64), 0, s, st, table, ncls);
        else
            hipLaunchKernelGGL(eval_mad_kernel, dim3(1), dim3(64), 0, s, st, table, ncls);
    }
    note_kernel("eval_select_pass_kernel");
    return check_launch("eval_stats");
}
