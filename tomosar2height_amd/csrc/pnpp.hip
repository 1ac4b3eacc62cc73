// PointNet++ point stages on the device (reference: tomosar2height/encoder/pointnetpp.py; ABI in include/t2h_pnpp.h):
// farthest point sampling, radius grouping, grouped rows, grouped max, 3-nearest-neighbour feature propagation, and the adjoints
// of the last three with respect to the features.
//
// FPS: the running distance of every point to the chosen set and, per centroid, an arg-max with the lowest index among equal
//   maxima.  Distances are sums of squares, so never negative and never NaN after the min: their bit patterns order as unsigned
//   integers.  The arg-max is two integer reductions -- the maximum of the bits, then the minimum of
//   (index | 0x7fffffff where the bits differ from the maximum) -- v_max_u32 / v_min_u32, no compare.
//   One-workgroup form: coordinates and distances of a cloud in LDS (16 B per point), one barrier per reduction, two per centroid.
//   Sliced form: one launch per centroid; every workgroup repeats the (cheap) reduction of the previous launch's per-slice
//   partials, updates its slice and leaves its own partial in the other half of a ping-pong pair.  No workgroup ever waits for
//   another one: launch boundaries order everything.
//
// BALL QUERY: one wave per query walks the cloud 64 points at a time; the in-ball lanes of a step are a ballot (a scalar
//   mask), their output slots the running count plus the population of the lower lanes' bits.
//
// THREE-NN: one target per thread, sources staged through LDS 512 at a time, a sorted list of three (d2, index) in registers;
//   a source replaces an entry only when strictly closer, and sources arrive in index order, so equal d2 keep the lower index.
//
// ADJOINTS (features only: xyz is data).  Grouped max: the gradient goes to the lowest row that holds the maximum.  A gather's
//   adjoint is a sum per source over the positions that read it: t2h_index_transpose builds that list (a CSR by index value,
//   each segment in ascending position) with integer atomics and a per-segment sort, and rows_gather_bwd_kernel walks it, one
//   workgroup per source row, one lane per column, in the fixed association of include/t2h_pnpp.h.  No float atomic.
//
// Compare results and vector selects (audited on the emitted assembly with isa_pass.lifetimes, figures in
//   DESIGN.md section 4.9).  These kernels run in the same forward as the split convolutions of the U-Net, on the same stream,
//   and could share a CU with those of another stream.  fps_one, group_rows, nn_interp and nn_repeat contain no v_cndmask:
//   lanes are exchanged with ds_bpermute (__shfl_xor carries a bounds select), the arg-max factor comes from an opaque
//   v_min_u32, grids are per group so that no flat index is divided.  fps_slice and group_max keep one v_cndmask 0, 1 from a
//   scalar-written mask; the ball query's ballot is read by v_mbcnt as data and its store re-compares in a branch.
//   three_nn_kernel is NOT select-free: its sorted insertion is 20 v_cndmask, each fed by a compare at most 6 instructions
//   earlier.  The adjoint kernels are written to the same rule: equality and the ReLU mask come from opaque v_min_u32 /
//   v_med3_i32 and an AND, the sort exchanges by v_min_i32 / v_max_i32, guarded stores and the zero-weight skip are branches.
#include <math.h>

#include "t2h_common.h"
#include "../../include/t2h_pnpp.h"

namespace t2h {

constexpr int kFpsOneThreads = 512;
constexpr int kFpsSliceThreads = 256;
constexpr int kNnThreads = 256;
constexpr int kNnChunk = 512;
constexpr int kSortMax = T2H_TRANSPOSE_SORT_MAX;
constexpr int kGatherChunk = T2H_GATHER_CHUNK;
constexpr int kGatherWaves = T2H_GATHER_LANES;
constexpr int kBnSlab = T2H_BN_SLAB;
constexpr int kBnWaves = T2H_BN_WAVES;
static_assert(kGatherChunk == 64, "a chunk's entries are held one per lane of a wave");
static_assert((kSortMax & (kSortMax - 1)) == 0, "the sorting network pads to a power of two");

__device__ inline float pn_d2(float x, float y, float z, float cx, float cy, float cz) {
    const float dx = __fsub_rn(x, cx), dy = __fsub_rn(y, cy), dz = __fsub_rn(z, cz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// index where the bits equal the maximum, 0x7fffffff elsewhere: no compare (bits <= maxbits always).  The clamp is an opaque
// v_min_u32: written as min(x, 1u) the compiler recognises the idiom and emits the very v_cmp_eq + v_cndmask this avoids.
__device__ inline unsigned pn_candidate(unsigned maxbits, unsigned bits, unsigned index) {
    unsigned differs;
    asm("v_min_u32 %0, %1, 1" : "=v"(differs) : "v"(maxbits - bits));
    return index | ((0u - differs) >> 1);
}
// max without the NaN test hipcc wraps around fmaxf (a v_cmp_u + v_cndmask per element)
__device__ inline float pn_max(float a, float b) {
    float m;
    asm("v_max_f32 %0, %1, %2" : "=v"(m) : "v"(a), "v"(b));
    return m;
}

// lane ^ o through ds_bpermute: unlike __shfl_xor it carries no bounds select (every partner lane exists in a full wave)
__device__ inline unsigned pn_xor_lane(unsigned v, int o) {
    return (unsigned)__builtin_amdgcn_ds_bpermute((int)(((threadIdx.x & 63) ^ o) << 2), (int)v);
}
__device__ inline unsigned pn_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, pn_xor_lane(v, o));
    return v;
}
__device__ inline unsigned pn_wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, pn_xor_lane(v, o));
    return v;
}

// workgroup-wide max / min over WAVES waves through `slot`: ONE barrier.  Call sites alternate between two slot arrays, so the
// barrier of the next reduction separates a slot's read from its next write.
template <int WAVES, bool MAX>
__device__ inline unsigned pn_block_reduce(unsigned v, unsigned *slot) {
    v = MAX ? pn_wave_max(v) : pn_wave_min(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = slot[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) r = MAX ? max(r, slot[w]) : min(r, slot[w]);
    return r;
}

// (the start is uniform per cloud: scalar compares and selects)
__device__ inline int pn_clamp_start(long long s, int N) {
    return (int)(s < 0 ? 0 : (s >= N ? N - 1 : s));
}

// ---------------------------------------------------------------------------------------------------- FPS, one workgroup
__global__ __launch_bounds__(kFpsOneThreads) void fps_one_kernel(const float *__restrict__ xyz, int N, int npoint,
                                                                 const long long *__restrict__ start,
                                                                 long long *__restrict__ centroids) {
    extern __shared__ __attribute__((aligned(16))) float pts[];          // [N][4]: x, y, z, running distance
    __shared__ unsigned red_m[kFpsOneThreads / 64], red_i[kFpsOneThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *src = xyz + (size_t)b * N * 3;
    for (int i = tid; i < N; i += kFpsOneThreads) {
        pts[4 * i + 0] = src[3 * i + 0];
        pts[4 * i + 1] = src[3 * i + 1];
        pts[4 * i + 2] = src[3 * i + 2];
        pts[4 * i + 3] = 1e10f;
    }
    __syncthreads();
    int cur = pn_clamp_start(start[b], N);
    for (int k = 0; k < npoint; ++k) {
        if (tid == 0) centroids[(size_t)b * npoint + k] = cur;
        const float cx = pts[4 * cur + 0], cy = pts[4 * cur + 1], cz = pts[4 * cur + 2];
        unsigned m = 0;
        for (int i = tid; i < N; i += kFpsOneThreads) {
            const float d = pn_d2(pts[4 * i + 0], pts[4 * i + 1], pts[4 * i + 2], cx, cy, cz);
            const float nd = fminf(pts[4 * i + 3], d);
            pts[4 * i + 3] = nd;
            m = max(m, __float_as_uint(nd));
        }
        const unsigned top = pn_block_reduce<kFpsOneThreads / 64, true>(m, red_m);
        unsigned c = 0x7fffffffu;
        for (int i = tid; i < N; i += kFpsOneThreads) c = min(c, pn_candidate(top, __float_as_uint(pts[4 * i + 3]), (unsigned)i));
        cur = (int)pn_block_reduce<kFpsOneThreads / 64, false>(c, red_i);
    }
}

// ---------------------------------------------------------------------------------------------------- FPS, one launch per centroid
// workspace: dist [B][N] float, then pm [2][B][nslices] unsigned, then pi [2][B][nslices] unsigned
__global__ __launch_bounds__(kFpsSliceThreads) void fps_slice_kernel(const float *__restrict__ xyz, int N, int npoint, int k,
                                                                     int slice, const long long *__restrict__ start,
                                                                     float *__restrict__ dist, unsigned *__restrict__ pm,
                                                                     unsigned *__restrict__ pi, long long *__restrict__ centroids) {
    __shared__ unsigned red[4][kFpsSliceThreads / 64];
    const int b = blockIdx.y, s = blockIdx.x, nslices = gridDim.x, B = gridDim.y, tid = threadIdx.x;
    int cur;
    if (k == 0) {
        cur = pn_clamp_start(start[b], N);
    } else {
        const unsigned *qm = pm + ((size_t)((k - 1) & 1) * B + b) * nslices;
        const unsigned *qi = pi + ((size_t)((k - 1) & 1) * B + b) * nslices;
        unsigned m = 0;
        for (int j = tid; j < nslices; j += kFpsSliceThreads) m = max(m, qm[j]);
        const unsigned top = pn_block_reduce<kFpsSliceThreads / 64, true>(m, red[0]);
        unsigned c = 0x7fffffffu;
        for (int j = tid; j < nslices; j += kFpsSliceThreads) c = min(c, pn_candidate(top, qm[j], qi[j]));
        cur = (int)pn_block_reduce<kFpsSliceThreads / 64, false>(c, red[1]);
    }
    if (s == 0 && tid == 0) centroids[(size_t)b * npoint + k] = cur;
    const float *src = xyz + (size_t)b * N * 3;
    float *dd = dist + (size_t)b * N;
    const float cx = src[3 * cur + 0], cy = src[3 * cur + 1], cz = src[3 * cur + 2];
    const int lo = s * slice, hi = min(lo + slice, N);
    unsigned m = 0;
    for (int i = lo + tid; i < hi; i += kFpsSliceThreads) {
        const float d = pn_d2(src[3 * i + 0], src[3 * i + 1], src[3 * i + 2], cx, cy, cz);
        float prev = 1e10f;
        if (k > 0) prev = dd[i];                                          // (uniform branch: the first launch reads nothing)
        const float nd = fminf(prev, d);
        dd[i] = nd;
        m = max(m, __float_as_uint(nd));
    }
    const unsigned top = pn_block_reduce<kFpsSliceThreads / 64, true>(m, red[2]);
    unsigned c = 0x7fffffffu;
    for (int i = lo + tid; i < hi; i += kFpsSliceThreads) c = min(c, pn_candidate(top, __float_as_uint(dd[i]), (unsigned)i));
    c = pn_block_reduce<kFpsSliceThreads / 64, false>(c, red[3]);
    if (tid == 0) {
        pm[((size_t)(k & 1) * B + b) * nslices + s] = top;
        pi[((size_t)(k & 1) * B + b) * nslices + s] = c;
    }
}

// ---------------------------------------------------------------------------------------------------- ball query
// grid (ceil(S / 4), B), one wave per query
__global__ __launch_bounds__(256) void ball_query_kernel(const float *__restrict__ xyz, const float *__restrict__ new_xyz, int N,
                                                         int S, float radius2, int nsample, long long *__restrict__ idx) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int sq = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sq >= S) return;                                                   // (wave-uniform)
    const size_t q = (size_t)b * S + sq;
    const float *src = xyz + (size_t)b * N * 3;
    const float qx = new_xyz[3 * q + 0], qy = new_xyz[3 * q + 1], qz = new_xyz[3 * q + 2];
    long long *out = idx + q * nsample;
    int count = 0, first = N;
    for (int base = 0; base < N && count < nsample; base += 64) {
        const int i = base + lane, ic = min(i, N - 1);
        const float d2 = pn_d2(src[3 * ic + 0], src[3 * ic + 1], src[3 * ic + 2], qx, qy, qz);
        const unsigned long long in = __ballot(i < N && !(d2 > radius2));
        const unsigned lo = (unsigned)in, hi = (unsigned)(in >> 32);
        const int pos = count + (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));      // in-ball lanes below
        if (i < N && !(d2 > radius2) && pos < nsample) out[pos] = i;         // (compared again at the use: a branch)
        if (count == 0 && in != 0ull) first = base + (__ffsll((long long)in) - 1);     // (uniform: scalar)
        count += __popcll(in);
    }
    for (int pos = min(count, nsample) + lane; pos < nsample; pos += 64) out[pos] = first;
}

// ---------------------------------------------------------------------------------------------------- grouped rows, grouped max
// grid (S, B), block (bx, 256 / bx): a block writes the nsample rows of one group; no index arithmetic needs a division
__global__ __launch_bounds__(256) void group_rows_kernel(const float *__restrict__ xyz, const float *__restrict__ new_xyz,
                                                         const float *__restrict__ points, const long long *__restrict__ idx,
                                                         int N, int S, int nsample, int D, int ld, float *__restrict__ rows) {
    const int b = blockIdx.y;
    const size_t bs = (size_t)b * S + blockIdx.x;
    const float *cen = new_xyz + bs * 3;
    for (int j = threadIdx.y; j < nsample; j += blockDim.y) {
        const size_t row = bs * nsample + j;
        const int id = max(0, min((int)idx[row], N - 1));
        const float *px = xyz + ((size_t)b * N + id) * 3;
        float *dst = rows + row * ld;
        for (int c = threadIdx.x; c < 3; c += blockDim.x) dst[c] = __fsub_rn(px[c], cen[c]);
        for (int c = threadIdx.x; c < D; c += blockDim.x) dst[3 + c] = points[((size_t)b * N + id) * D + c];
        for (int c = 3 + D + threadIdx.x; c < ld; c += blockDim.x) dst[c] = 0.0f;
    }
}

// grid (groups), 256 threads over the columns
__global__ __launch_bounds__(256) void group_max_kernel(const float *__restrict__ rows, int ld, int nsample, int C,
                                                        float *__restrict__ out) {
    const size_t g = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float *p = rows + g * nsample * ld + c;
        float m = p[0];
        for (int j = 1; j < nsample; ++j) m = pn_max(m, p[(size_t)j * ld]);
        out[g * C + c] = m;
    }
}

// ---------------------------------------------------------------------------------------------------- three nearest + interpolation
__global__ __launch_bounds__(kNnThreads) void three_nn_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                              int N, int S, long long *__restrict__ idx,
                                                              float *__restrict__ weight) {
    __shared__ float src[kNnChunk * 3];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int i = blockIdx.x * kNnThreads + tid, ic = min(i, N - 1);
    const float *t = xyz1 + ((size_t)b * N + ic) * 3;
    const float x = t[0], y = t[1], z = t[2];
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int base = 0; base < S; base += kNnChunk) {
        const int n = min(kNnChunk, S - base);
        __syncthreads();
        for (int j = tid; j < 3 * n; j += kNnThreads) src[j] = xyz2[((size_t)b * S + base) * 3 + j];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float d = pn_d2(x, y, z, src[3 * j + 0], src[3 * j + 1], src[3 * j + 2]);
            const int g = base + j;
            if (d < d2) {
                if (d < d1) {
                    d2 = d1; i2 = i1;
                    if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = g; }
                    else { d1 = d; i1 = g; }
                } else { d2 = d; i2 = g; }
            }
        }
    }
    if (i >= N) return;
    const float r0 = __fdiv_rn(1.0f, __fadd_rn(d0, 1e-8f)), r1 = __fdiv_rn(1.0f, __fadd_rn(d1, 1e-8f)),
                r2 = __fdiv_rn(1.0f, __fadd_rn(d2, 1e-8f));
    const float norm = __fadd_rn(__fadd_rn(r0, r1), r2);
    const size_t o = ((size_t)b * N + i) * 3;
    idx[o + 0] = i0; idx[o + 1] = i1; idx[o + 2] = i2;
    weight[o + 0] = __fdiv_rn(r0, norm); weight[o + 1] = __fdiv_rn(r1, norm); weight[o + 2] = __fdiv_rn(r2, norm);
}

// grid (ceil(N / 4), B), block (64, 4): four targets per block, lanes over the columns
__global__ __launch_bounds__(256) void nn_interp_kernel(const float *__restrict__ points2, const long long *__restrict__ idx,
                                                        const float *__restrict__ weight, int N, int S, int D,
                                                        float *__restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 4 + threadIdx.y;
    if (i >= N) return;
    const size_t row = (size_t)b * N + i;
    const float *p = points2 + (size_t)b * S * D;
    const long long *k = idx + row * 3;
    const float *w = weight + row * 3;
    const float *p0 = p + k[0] * D, *p1 = p + k[1] * D, *p2 = p + k[2] * D;
    const float w0 = w[0], w1 = w[1], w2 = w[2];
    for (int c = threadIdx.x; c < D; c += 64)
        out[row * D + c] = __fadd_rn(__fadd_rn(__fmul_rn(p0[c], w0), __fmul_rn(p1[c], w1)), __fmul_rn(p2[c], w2));
}

// S == 1: the reference's points2.repeat(1, N, 1); same grid
__global__ __launch_bounds__(256) void nn_repeat_kernel(const float *__restrict__ points2, int N, int D,
                                                        long long *__restrict__ idx, float *__restrict__ weight,
                                                        float *__restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 4 + threadIdx.y;
    if (i >= N) return;
    const size_t row = (size_t)b * N + i;
    for (int c = threadIdx.x; c < D; c += 64) out[row * D + c] = points2[(size_t)b * D + c];
    if (threadIdx.x == 0) {
        idx[row * 3 + 0] = 0; idx[row * 3 + 1] = 0; idx[row * 3 + 2] = 0;
        weight[row * 3 + 0] = 1.0f; weight[row * 3 + 1] = 0.0f; weight[row * 3 + 2] = 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------- adjoints
// 0 where a == b, 1 elsewhere, and the ReLU mask, by opaque integer instructions (no compare, see the head of this file)
__device__ inline unsigned pn_differs(unsigned a, unsigned b) {
    unsigned d;
    asm("v_min_u32 %0, %1, 1" : "=v"(d) : "v"(a ^ b));
    return d;
}
// all ones where x > 0, 0 elsewhere (+-0, negative, NaN with the sign bit): -med3(bits, 0, 1) on the bits as a signed integer
__device__ inline unsigned pn_positive_mask(float x) {
    int m;
    asm("v_med3_i32 %0, %1, 0, 1" : "=v"(m) : "v"(__float_as_int(x)));
    return (unsigned)(-m);
}

// grid (groups), 256 threads over the columns 0 .. gld.  Pass 1 finds the lowest row j with rows[j, c] - out[c] == 0 as an
// integer minimum of j | 0x7fffffff * (difference != 0); pass 2 writes gout & -(j == first) row by row.
__global__ __launch_bounds__(256) void group_max_bwd_kernel(const float *__restrict__ rows, int ld, int nsample, int C,
                                                            const float *__restrict__ out, const float *__restrict__ gout,
                                                            int relu, float *__restrict__ grows, int gld) {
    const size_t g = blockIdx.x;
    const unsigned keep_all = relu ? 0u : 0xffffffffu;                    // (uniform)
    for (int c = threadIdx.x; c < gld; c += 256) {
        float *dst = grows + g * nsample * gld + c;
        if (c >= C) {
            for (int j = 0; j < nsample; ++j) dst[(size_t)j * gld] = 0.0f;
            continue;
        }
        const float o = out[g * C + c];
        const unsigned gv = __float_as_uint(gout[g * C + c]) & (pn_positive_mask(o) | keep_all);
        const float *p = rows + g * nsample * ld + c;
        unsigned first = 0x7fffffffu;
        for (int j = 0; j < nsample; ++j) {
            const unsigned differs = pn_differs(__float_as_uint(__fsub_rn(p[(size_t)j * ld], o)) & 0x7fffffffu, 0u);
            first = min(first, (unsigned)j | ((0u - differs) >> 1));
        }
        for (int j = 0; j < nsample; ++j)
            dst[(size_t)j * gld] = __uint_as_float(gv & (pn_differs((unsigned)j, first) - 1u));
    }
}

__device__ inline int pn_clamp_index(long long v, int N) {
    return (int)(v < 0 || v >= N ? N - 1 : v);
}

// grid (ceil(E / 256), B): cursor[b, i] += 1 per entry with index i (integer atomics: the counts do not depend on the order)
__global__ __launch_bounds__(256) void transpose_count_kernel(const long long *__restrict__ idx, int E, int N,
                                                              int *__restrict__ cursor) {
    const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    atomicAdd(cursor + (size_t)b * N + pn_clamp_index(idx[(size_t)b * E + e], N), 1);
}

// grid (B), 256 threads: offsets[b, 0 .. N] = exclusive prefix sums of the counts, 256 at a time behind a running total;
// cursor[b, i] = offsets[b, i]
__global__ __launch_bounds__(256) void transpose_scan_kernel(int N, int *__restrict__ offsets, int *__restrict__ cursor) {
    __shared__ int part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    int *cur = cursor + (size_t)b * N, *off = offsets + (size_t)b * (N + 1);
    int run = 0;
    for (int base = 0; base < N; base += 256) {
        const int i = base + tid;
        int count = 0;
        if (i < N) count = cur[i];
        part[tid] = count;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                               // Hillis-Steele inclusive scan
            int add = 0;
            if (tid >= o) add = part[tid - o];
            __syncthreads();
            part[tid] += add;
            __syncthreads();
        }
        const int incl = part[tid], total = part[255];
        if (i < N) {
            off[i] = run + incl - count;
            cur[i] = run + incl - count;
        }
        run += total;
        __syncthreads();
    }
    if (tid == 0) off[N] = run;
}

// grid (ceil(E / 256), B): entry e takes the next free slot of its segment (the order inside a segment depends on scheduling;
// transpose_sort_kernel then orders it)
__global__ __launch_bounds__(256) void transpose_place_kernel(const long long *__restrict__ idx, int E, int N,
                                                              int *__restrict__ cursor, int *__restrict__ entries) {
    const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int pos = atomicAdd(cursor + (size_t)b * N + pn_clamp_index(idx[(size_t)b * E + e], N), 1);
    if (pos >= 0 && pos < E) entries[(size_t)b * E + pos] = e;            // (always inside: the counts were taken from the same idx)
}

// grid (N, B), 256 threads: one segment per workgroup, ordered by e.  Up to kSortMax entries: in LDS, padded with INT_MAX to a
// power of two, by a sorting network whose every exchange is (min, max) -- each merge opens with the mirrored partner
// i ^ (k - 1), then halves the distance -- so no direction is ever selected.  Longer segments are written afresh: the workgroup
// walks e = 0 .. E in index order, 256 at a time, and hands the matching entries consecutive slots (ballot + population of
// the lower lanes, as the ball query).
__global__ __launch_bounds__(256) void transpose_sort_kernel(const long long *__restrict__ idx, int E, int N,
                                                             const int *__restrict__ offsets, int *__restrict__ entries) {
    __shared__ int key[kSortMax];
    __shared__ int wave_count[4];
    const int b = blockIdx.y, i = blockIdx.x, tid = threadIdx.x;
    const int *off = offsets + (size_t)b * (N + 1);
    const int lo = max(0, min(off[i], E)), hi = max(lo, min(off[i + 1], E)), len = hi - lo;
    if (len < 2) return;                                                  // (uniform)
    int *seg = entries + (size_t)b * E + lo;
    if (len <= kSortMax) {
        int P = 2;
        while (P < len) P <<= 1;
        for (int t = tid; t < P; t += 256) {
            int v = 0x7fffffff;
            if (t < len) v = seg[t];
            key[t] = v;
        }
        __syncthreads();
        for (int lk = 1; (1 << lk) <= P; ++lk) {                          // merges of k = 2^lk keys
            const int k = 1 << lk, half = k >> 1;
            for (int t = tid; t < (P >> 1); t += 256) {
                const int base = (t >> (lk - 1)) << lk, within = t & (half - 1);
                const int a = base + within, c = base + (k - 1 - within);
                const int x = key[a], y = key[c];
                key[a] = min(x, y);
                key[c] = max(x, y);
            }
            __syncthreads();
            for (int lj = lk - 2; lj >= 0; --lj) {                        // distances j = 2^lj
                const int j = 1 << lj;
                for (int t = tid; t < (P >> 1); t += 256) {
                    const int a = ((t >> lj) << (lj + 1)) + (t & (j - 1)), c = a + j;
                    const int x = key[a], y = key[c];
                    key[a] = min(x, y);
                    key[c] = max(x, y);
                }
                __syncthreads();
            }
        }
        for (int t = tid; t < len; t += 256) seg[t] = key[t];
        return;
    }
    const long long *src = idx + (size_t)b * E;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // (scalar: the sums below select by it)
    int run = 0;
    for (int base = 0; base < E; base += 256) {
        const int e = base + tid;
        int id = -1;
        if (e < E) id = pn_clamp_index(src[e], N);
        const unsigned long long in = __ballot(id == i);
        if (lane == 0) wave_count[wave] = __popcll(in);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < 4; ++w) {                                     // (uniform per wave: scalar)
            const int n = wave_count[w];
            if (w < wave) before += n;
            total += n;
        }
        const int pos = run + before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(in >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)in, 0u));
        if (id == i && pos < len) seg[pos] = e;                           // (compared again at the use: a branch)
        run += total;
        __syncthreads();
    }
}

// grid (N, B, ceil(D / 64)), block (64, kGatherWaves): one destination row and 64 columns per workgroup, one lane per column.
// Wave y sums the chunks k = y, y + kGatherWaves, ... of kGatherChunk consecutive entries of the segment, each chunk from +0 in
// ascending order, the chunk sums in ascending k from +0; out = ((s_0 + s_1) + s_2) + s_3.  Separate multiply and add.
__global__ __launch_bounds__(64 * kGatherWaves) void rows_gather_bwd_kernel(const float *__restrict__ g, int gld, int col0, int D,
                                                                            const float *__restrict__ weight, int fan,
                                                                            const int *__restrict__ offsets,
                                                                            const int *__restrict__ entries, int E, int N,
                                                                            float *__restrict__ out) {
    __shared__ float lane_sum[kGatherWaves][64];
    const int b = blockIdx.y, i = blockIdx.x, d = blockIdx.z * 64 + threadIdx.x, y = threadIdx.y;
    const int dc = min(d, D - 1);
    const int *off = offsets + (size_t)b * (N + 1);
    const int lo = max(0, min(off[i], E)), hi = max(lo, min(off[i + 1], E));
    const int *seg = entries + (size_t)b * E;
    const float *w = weight ? weight + (size_t)b * E : nullptr;
    const float *src = g + (size_t)b * (size_t)(E / fan) * gld + col0 + dc;
    float s = 0.0f;
    for (int c0 = lo + y * kGatherChunk; c0 < hi; c0 += kGatherWaves * kGatherChunk) {
        const int n = min(kGatherChunk, hi - c0);
        // the chunk's entries and weights, one per lane (lanes past the chunk repeat its last entry and are not read)
        const int mine = max(0, min(seg[c0 + min((int)threadIdx.x, n - 1)], E - 1));
        const int my_row = fan == 3 ? mine / 3 : mine;
        float my_w = 1.0f;
        if (w) my_w = w[mine];
        float p = 0.0f;
        for (int k = 0; k < n; k += 4) {                                  // four rows in flight; added in ascending order
            float v[4], we[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int ku = min(k + u, n - 1);                         // (uniform)
                v[u] = src[(size_t)__builtin_amdgcn_readlane(my_row, ku) * gld];
                we[u] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my_w), ku));
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)                                   // (uniform conditions: branches; w == 0 adds nothing)
                if (k + u < n && we[u] != 0.0f) p = __fadd_rn(p, __fmul_rn(we[u], v[u]));
        }
        s = __fadd_rn(s, p);
    }
    lane_sum[y][threadIdx.x] = s;
    __syncthreads();
    if (y == 0 && d < D) {
        float t = lane_sum[0][threadIdx.x];
        for (int k = 1; k < kGatherWaves; ++k) t = __fadd_rn(t, lane_sum[k][threadIdx.x]);
        out[((size_t)b * N + i) * D + d] = t;
    }
}

// ---------------------------------------------------------------------------------------- BatchNorm batch statistics
// Column reductions over rows [M, ld] in the association of include/t2h_pnpp.h.  grid (slabs, ceil(C / 64)), block (64, kBnWaves):
// one slab of kBnSlab rows and 64 columns per workgroup, one lane per column (256-byte coalesced row segments).  Wave y adds the
// terms of the slab's rows y, y + 4, ... in ascending order from +0; the slab's partial is ((w_0 + w_1) + w_2) + w_3.  Row bounds
// are loop limits, the column is clamped for the loads (v_min) and the store is a branch: no compare feeds a select.
//   MODE 0: term = z                        MODE 1: term = (z - mean)^2
//   MODE 2: two sums, g and g * xhat, with g = gy & (-(y > 0) | keep_all) (keep_all: y is any readable rows), xhat = (z - mean) * rstd  (second plane: nslabs * C floats on)
template <int MODE>
__global__ __launch_bounds__(64 * kBnWaves) void bn_partial_kernel(const float *__restrict__ z, int ldz, int M, int C,
                                                                    const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                    const float *__restrict__ gy, int ldg,
                                                                    const float *__restrict__ y, int ldy, unsigned keep_all,
                                                                    float *__restrict__ partial) {
    __shared__ float wave_sum[MODE == 2 ? 2 : 1][kBnWaves][64];
    const int c = blockIdx.y * 64 + threadIdx.x, cc = min(c, C - 1), w = threadIdx.y;
    const int r0 = blockIdx.x * kBnSlab, r1 = min(r0 + kBnSlab, M);
    float mu = 0.0f, rs = 0.0f;
    if (MODE >= 1) mu = mean[cc];
    if (MODE == 2) rs = rstd[cc];
    float s0 = 0.0f, s1 = 0.0f;
    for (int r = r0 + w; r < r1; r += kBnWaves) {
        const float v = z[(size_t)r * ldz + cc];
        if (MODE == 0) {
            s0 = __fadd_rn(s0, v);
        } else if (MODE == 1) {
            const float d = __fsub_rn(v, mu);
            s0 = __fadd_rn(s0, __fmul_rn(d, d));
        } else {
            const float g = __uint_as_float(__float_as_uint(gy[(size_t)r * ldg + cc]) & (pn_positive_mask(y[(size_t)r * ldy + cc]) | keep_all));
            s0 = __fadd_rn(s0, g);
            s1 = __fadd_rn(s1, __fmul_rn(g, __fmul_rn(__fsub_rn(v, mu), rs)));
        }
    }
    wave_sum[0][w][threadIdx.x] = s0;
    if (MODE == 2) wave_sum[1][w][threadIdx.x] = s1;
    __syncthreads();
    if (w == 0 && c < C) {
        const size_t plane = (size_t)gridDim.x * C;
#pragma unroll
        for (int p = 0; p < (MODE == 2 ? 2 : 1); ++p) {
            float t = wave_sum[p][0][threadIdx.x];
            for (int k = 1; k < kBnWaves; ++k) t = __fadd_rn(t, wave_sum[p][k][threadIdx.x]);
            partial[p * plane + (size_t)blockIdx.x * C + c] = t;
        }
    }
}

// Correctly rounded square root of a normal x without a compare: v_sqrt_f32 is within one ulp; its lower neighbour is the
// result when x - s_dn * s <= 0, its upper one when x - s_up * s > 0 (exact signs from one FMA each) -- the fix-up hipcc's own
// sqrtf makes with v_cmp + v_cndmask, here as integer steps from the opaque v_med3_i32 mask.
__device__ inline float bn_sqrt(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const int b = __float_as_int(s);
    const float r_dn = __fmaf_rn(-__int_as_float(b - 1), s, x), r_up = __fmaf_rn(-__int_as_float(b + 1), s, x);
    return __int_as_float(b + (int)~pn_positive_mask(r_dn) + (int)(pn_positive_mask(r_up) & 1u));
}

// grid (ceil(C / 256)), one lane per column: the slab partials in ascending slab order from +0, then
//   mode 0: out0 = mean = sum / M          mode 1: out0 = var = sum / M, out1 = rstd = 1 / sqrt(var + eps)
//   mode 2: out0 = the first plane's sum, out1 = the second plane's
__global__ __launch_bounds__(256) void bn_finish_kernel(const float *__restrict__ partial, int nslabs, int C, int mode, float m,
                                                        float eps, float *__restrict__ out0, float *__restrict__ out1) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s0 = 0.0f, s1 = 0.0f;
    for (int k = 0; k < nslabs; ++k) s0 = __fadd_rn(s0, partial[(size_t)k * C + c]);
    if (mode == 2) {                                                      // (uniform)
        for (int k = 0; k < nslabs; ++k) s1 = __fadd_rn(s1, partial[((size_t)nslabs + k) * C + c]);
        out0[c] = s0;
        out1[c] = s1;
        return;
    }
    const float q = __fdiv_rn(s0, m);
    out0[c] = q;
    if (mode == 1) out1[c] = __fdiv_rn(1.0f, bn_sqrt(__fadd_rn(q, eps)));
}

// grid (ceil(M / kBnSlab), ceil(ldy / 64)), block (64, kBnWaves): y = max(z * s + t, 0), s = gamma * rstd, t = beta - mean * s
// (once per lane: its column is fixed); columns C .. ldy are +0.  The max is an opaque v_max_f32.
__global__ __launch_bounds__(64 * kBnWaves) void bn_apply_relu_kernel(const float *__restrict__ z, int ldz, int M, int C,
                                                                       const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                       const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                       float *__restrict__ y, int ldy) {
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (c >= ldy) return;
    const int r0 = blockIdx.x * kBnSlab, r1 = min(r0 + kBnSlab, M);
    if (c >= C) {
        for (int r = r0 + threadIdx.y; r < r1; r += kBnWaves) y[(size_t)r * ldy + c] = 0.0f;
        return;
    }
    const float s = __fmul_rn(gamma[c], rstd[c]), t = __fsub_rn(beta[c], __fmul_rn(mean[c], s));
    for (int r = r0 + threadIdx.y; r < r1; r += kBnWaves)
        y[(size_t)r * ldy + c] = pn_max(__fadd_rn(__fmul_rn(z[(size_t)r * ldz + c], s), t), 0.0f);
}

// same grid: dz = a * ((g - mb) - xhat * mg), a = gamma * rstd, mb = dbeta / M, mg = dgamma / M, xhat = (z - mean) * rstd,
// g = gy [& (y > 0)]; columns C .. gld are +0
__global__ __launch_bounds__(64 * kBnWaves) void bn_bwd_apply_kernel(const float *__restrict__ gy, int ldg, const float *__restrict__ y,
                                                                      int ldy, const float *__restrict__ z, int ldz, int M, int C,
                                                                      const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                      const float *__restrict__ gamma, const float *__restrict__ dbeta,
                                                                      const float *__restrict__ dgamma, float m, unsigned keep_all,
                                                                      float *__restrict__ dz, int gld) {
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (c >= gld) return;
    const int r0 = blockIdx.x * kBnSlab, r1 = min(r0 + kBnSlab, M);
    if (c >= C) {
        for (int r = r0 + threadIdx.y; r < r1; r += kBnWaves) dz[(size_t)r * gld + c] = 0.0f;
        return;
    }
    const float mu = mean[c], rs = rstd[c], a = __fmul_rn(gamma[c], rs);
    const float mb = __fdiv_rn(dbeta[c], m), mg = __fdiv_rn(dgamma[c], m);
    for (int r = r0 + threadIdx.y; r < r1; r += kBnWaves) {
        const unsigned gb = __float_as_uint(gy[(size_t)r * ldg + c]) & (pn_positive_mask(y[(size_t)r * ldy + c]) | keep_all);
        const float xhat = __fmul_rn(__fsub_rn(z[(size_t)r * ldz + c], mu), rs);
        dz[(size_t)r * gld + c] = __fmul_rn(a, __fsub_rn(__fsub_rn(__uint_as_float(gb), mb), __fmul_rn(xhat, mg)));
    }
}

// one lane per column: the momentum recurrence of the running statistics, with the unbiased variance var * (M / (M - 1))
__global__ __launch_bounds__(256) void bn_running_kernel(const float *__restrict__ mean, const float *__restrict__ var, int C, float m,
                                                         float momentum, float *__restrict__ running_mean,
                                                         float *__restrict__ running_var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float keep = __fsub_rn(1.0f, momentum), unbias = __fdiv_rn(m, __fsub_rn(m, 1.0f));
    running_mean[c] = __fadd_rn(__fmul_rn(keep, running_mean[c]), __fmul_rn(momentum, mean[c]));
    running_var[c] = __fadd_rn(__fmul_rn(keep, running_var[c]), __fmul_rn(momentum, __fmul_rn(var[c], unbias)));
}

static unsigned blocks_for(long long total, int per) { return (unsigned)((total + per - 1) / per); }

// shapes every BatchNorm entry accepts: 2 <= M <= 2^24 (M is exact as a float), 1 <= C <= every row length
static bool bn_shape_ok(int M, int C) { return M >= 2 && M <= (1 << 24) && C >= 1 && C <= 64 * 65535; }

}  // namespace t2h

using namespace t2h;

T2H_API size_t t2h_fps_workspace_bytes(int B, int N, int slice) {
    if (B < 1 || N < 1 || slice < 0 || slice % 64 != 0) return 0;
    if (slice == 0) return N <= T2H_FPS_ONE_WG_MAX ? 1 : 0;
    const size_t nslices = ((size_t)N + slice - 1) / slice;
    return (size_t)B * N * sizeof(float) + 4 * (size_t)B * nslices * sizeof(unsigned);
}

T2H_API int t2h_fps(const float *xyz, int B, int N, int npoint, const int64_t *start, int slice, int64_t *centroids,
                    void *workspace, size_t workspace_bytes, t2h_stream_t stream) {
    if (!xyz || !start || !centroids) return fail(T2H_ERR_ARG, "fps: null pointer");
    if (B < 1 || B > 65535 || N < 1 || npoint < 1) return fail(T2H_ERR_ARG, "fps: bad shape B=%d N=%d npoint=%d", B, N, npoint);
    if (slice < 0 || slice % 64 != 0) return fail(T2H_ERR_ARG, "fps: slice=%d must be 0 or a multiple of 64", slice);
    hipStream_t s = as_stream(stream);
    if (slice == 0) {
        if (N > T2H_FPS_ONE_WG_MAX)
            return fail(T2H_ERR_ARG, "fps: the one-workgroup form holds N <= %d points, got %d", T2H_FPS_ONE_WG_MAX, N);
        hipLaunchKernelGGL(fps_one_kernel, dim3(B), dim3(kFpsOneThreads), (size_t)N * 16, s, xyz, N, npoint,
                           reinterpret_cast<const long long *>(start), reinterpret_cast<long long *>(centroids));
        note_kernel("fps_one_kernel");
        return check_launch("fps");
    }
    const size_t need = t2h_fps_workspace_bytes(B, N, slice);
    if (!workspace || workspace_bytes < need) return fail(T2H_ERR_WORKSPACE, "fps: workspace %zu < %zu bytes", workspace_bytes, need);
    const unsigned nslices = (unsigned)(((size_t)N + slice - 1) / slice);
    float *dist = static_cast<float *>(workspace);
    unsigned *pm = reinterpret_cast<unsigned *>(dist + (size_t)B * N);
    unsigned *pi = pm + 2 * (size_t)B * nslices;
    for (int k = 0; k < npoint; ++k)
        hipLaunchKernelGGL(fps_slice_kernel, dim3(nslices, B), dim3(kFpsSliceThreads), 0, s, xyz, N, npoint, k, slice,
                           reinterpret_cast<const long long *>(start), dist, pm, pi, reinterpret_cast<long long *>(centroids));
    note_kernel("fps_slice_kernel");
    return check_launch("fps");
}

T2H_API int t2h_ball_query(const float *xyz, const float *new_xyz, int B, int N, int S, float radius2, int nsample, int64_t *idx,
                           t2h_stream_t stream) {
    if (!xyz || !new_xyz || !idx) return fail(T2H_ERR_ARG, "ball_query: null pointer");
    if (B < 1 || B > 65535 || N < 1 || S < 1 || nsample < 1) return fail(T2H_ERR_ARG, "ball_query: bad shape");
    hipLaunchKernelGGL(ball_query_kernel, dim3(blocks_for(S, 4), B), dim3(256), 0, as_stream(stream), xyz, new_xyz, N, S, radius2,
                       nsample, reinterpret_cast<long long *>(idx));
    note_kernel("ball_query_kernel");
    return check_launch("ball_query");
}

T2H_API int t2h_group_rows(const float *xyz, const float *new_xyz, const float *points, const int64_t *idx, int B, int N, int S,
                           int nsample, int D, int ld, float *rows, t2h_stream_t stream) {
    if (!xyz || !new_xyz || !idx || !rows || (D > 0 && !points)) return fail(T2H_ERR_ARG, "group_rows: null pointer");
    if (B < 1 || B > 65535 || N < 1 || S < 1 || nsample < 1 || D < 0 || ld < 3 + D) return fail(T2H_ERR_ARG, "group_rows: bad shape");
    const unsigned bx = ld <= 8 ? 8u : (ld <= 32 ? 32u : 64u);
    hipLaunchKernelGGL(group_rows_kernel, dim3(S, B), dim3(bx, 256 / bx), 0, as_stream(stream), xyz, new_xyz, points,
                       reinterpret_cast<const long long *>(idx), N, S, nsample, D, ld, rows);
    note_kernel("group_rows_kernel");
    return check_launch("group_rows");
}

T2H_API int t2h_group_max(const float *rows, int ld, int64_t groups, int nsample, int C, float *out, t2h_stream_t stream) {
    if (!rows || !out) return fail(T2H_ERR_ARG, "group_max: null pointer");
    if (groups < 1 || groups > 0x7fffffffll || nsample < 1 || C < 1 || ld < C) return fail(T2H_ERR_ARG, "group_max: bad shape");
    hipLaunchKernelGGL(group_max_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(stream), rows, ld, nsample, C, out);
    note_kernel("group_max_kernel");
    return check_launch("group_max");
}

T2H_API int t2h_three_nn_interp(const float *xyz1, const float *xyz2, const float *points2, int B, int N, int S, int D,
                                int64_t *idx, float *weight, float *out, t2h_stream_t stream) {
    if (!xyz1 || !xyz2 || !points2 || !idx || !weight || !out) return fail(T2H_ERR_ARG, "three_nn_interp: null pointer");
    if (B < 1 || B > 65535 || N < 1 || S < 1 || D < 1) return fail(T2H_ERR_ARG, "three_nn_interp: bad shape");
    if (S == 2) return fail(T2H_ERR_ARG, "three_nn_interp: S = 2 has no three neighbours (the reference fails on it too)");
    hipStream_t s = as_stream(stream);
    if (S == 1) {
        hipLaunchKernelGGL(nn_repeat_kernel, dim3(blocks_for(N, 4), B), dim3(64, 4), 0, s, points2, N, D,
                           reinterpret_cast<long long *>(idx), weight, out);
        note_kernel("nn_repeat_kernel");
        return check_launch("three_nn_interp");
    }
    hipLaunchKernelGGL(three_nn_kernel, dim3(blocks_for(N, kNnThreads), B), dim3(kNnThreads), 0, s, xyz1, xyz2, N, S,
                       reinterpret_cast<long long *>(idx), weight);
    hipLaunchKernelGGL(nn_interp_kernel, dim3(blocks_for(N, 4), B), dim3(64, 4), 0, s, points2, reinterpret_cast<const long long *>(idx),
                       weight, N, S, D, out);
    note_kernel("three_nn_kernel");
    return check_launch("three_nn_interp");
}

T2H_API int t2h_group_max_bwd(const float *rows, int ld, int64_t groups, int nsample, int C, const float *out, const float *gout,
                              int relu, float *grows, int gld, t2h_stream_t stream) {
    if (!rows || !out || !gout || !grows) return fail(T2H_ERR_ARG, "group_max_bwd: null pointer");
    if (groups < 1 || groups > 0x7fffffffll || nsample < 1 || C < 1 || ld < C || gld < C)
        return fail(T2H_ERR_ARG, "group_max_bwd: bad shape groups=%lld nsample=%d C=%d ld=%d gld=%d", (long long)groups, nsample, C, ld, gld);
    hipLaunchKernelGGL(group_max_bwd_kernel, dim3((unsigned)groups), dim3(256), 0, as_stream(stream), rows, ld, nsample, C, out, gout,
                       relu ? 1 : 0, grows, gld);
    note_kernel("group_max_bwd_kernel");
    return check_launch("group_max_bwd");
}

T2H_API int t2h_index_transpose(const int64_t *idx, int B, int E, int N, int32_t *offsets, int32_t *entries, int32_t *cursor,
                                t2h_stream_t stream) {
    if (!idx || !offsets || !entries || !cursor) return fail(T2H_ERR_ARG, "index_transpose: null pointer");
    if (B < 1 || B > 65535 || E < 1 || N < 1) return fail(T2H_ERR_ARG, "index_transpose: bad shape B=%d E=%d N=%d", B, E, N);
    hipStream_t s = as_stream(stream);
    const long long *src = reinterpret_cast<const long long *>(idx);
    if (hipMemsetAsync(cursor, 0, (size_t)B * N * sizeof(int32_t), s) != hipSuccess) return fail(T2H_ERR_LAUNCH, "index_transpose: memset");
    hipLaunchKernelGGL(transpose_count_kernel, dim3(blocks_for(E, 256), B), dim3(256), 0, s, src, E, N, cursor);
    hipLaunchKernelGGL(transpose_scan_kernel, dim3(B), dim3(256), 0, s, N, offsets, cursor);
    hipLaunchKernelGGL(transpose_place_kernel, dim3(blocks_for(E, 256), B), dim3(256), 0, s, src, E, N, cursor, entries);
    hipLaunchKernelGGL(transpose_sort_kernel, dim3(N, B), dim3(256), 0, s, src, E, N, offsets, entries);
    note_kernel("transpose_sort_kernel");
    return check_launch("index_transpose");
}

T2H_API int t2h_rows_gather_bwd(const float *g, int gld, int col0, int D, const float *weight, int fan, const int32_t *offsets,
                                const int32_t *entries, int B, int E, int N, float *out, t2h_stream_t stream) {
    if (!g || !offsets || !entries || !out) return fail(T2H_ERR_ARG, "rows_gather_bwd: null pointer");
    if (fan != 1 && fan != 3) return fail(T2H_ERR_ARG, "rows_gather_bwd: fan=%d must be 1 or 3", fan);
    if (B < 1 || B > 65535 || E < 1 || N < 1 || D < 1 || D > 64 * 65535 || col0 < 0 || gld < col0 + D || E % fan != 0)
        return fail(T2H_ERR_ARG, "rows_gather_bwd: bad shape B=%d E=%d N=%d D=%d col0=%d gld=%d fan=%d", B, E, N, D, col0, gld, fan);
    hipLaunchKernelGGL(rows_gather_bwd_kernel, dim3(N, B, blocks_for(D, 64)), dim3(64, kGatherWaves), 0, as_stream(stream), g, gld,
                       col0, D, weight, fan, offsets, entries, E, N, out);
    note_kernel("rows_gather_bwd_kernel");
    return check_launch("rows_gather_bwd");
}

// ---------------------------------------------------------------------------------------- BatchNorm batch statistics
T2H_API int t2h_bn_col_stats(const float *z, int ld, int M, int C, float eps, float *partial, float *mean, float *var, float *rstd,
                             t2h_stream_t stream) {
    if (!z || !partial || !mean || !var || !rstd) return fail(T2H_ERR_ARG, "bn_col_stats: null pointer");
    if (!bn_shape_ok(M, C) || ld < C) return fail(T2H_ERR_ARG, "bn_col_stats: bad shape M=%d C=%d ld=%d (M >= 2)", M, C, ld);
    if (!(eps >= 1e-30f && eps <= 1e30f)) return fail(T2H_ERR_ARG, "bn_col_stats: eps=%g outside [1e-30, 1e30]", (double)eps);
    hipStream_t s = as_stream(stream);
    const unsigned nslabs = blocks_for(M, kBnSlab);
    const dim3 grid(nslabs, blocks_for(C, 64)), block(64, kBnWaves);
    hipLaunchKernelGGL(bn_partial_kernel<0>, grid, block, 0, s, z, ld, M, C, nullptr, nullptr, nullptr, 0, nullptr, 0, 0u, partial);
    hipLaunchKernelGGL(bn_finish_kernel, dim3(blocks_for(C, 256)), dim3(256), 0, s, partial, (int)nslabs, C, 0, (float)M, eps, mean,
                       nullptr);
    hipLaunchKernelGGL(bn_partial_kernel<1>, grid, block, 0, s, z, ld, M, C, mean, nullptr, nullptr, 0, nullptr, 0, 0u, partial);
    hipLaunchKernelGGL(bn_finish_kernel, dim3(blocks_for(C, 256)), dim3(256), 0, s, partial, (int)nslabs, C, 1, (float)M, eps, var, rstd);
    note_kernel("bn_partial_kernel");
    return check_launch("bn_col_stats");
}

T2H_API int t2h_bn_apply_relu(const float *z, int ldz, int M, int C, const float *mean, const float *rstd, const float *gamma,
                              const float *beta, float *y, int ldy, t2h_stream_t stream) {
    if (!z || !mean || !rstd || !gamma || !beta || !y) return fail(T2H_ERR_ARG, "bn_apply_relu: null pointer");
    if (!bn_shape_ok(M, C) || ldz < C || ldy < C || ldy > 64 * 65535)
        return fail(T2H_ERR_ARG, "bn_apply_relu: bad shape M=%d C=%d ldz=%d ldy=%d", M, C, ldz, ldy);
    hipLaunchKernelGGL(bn_apply_relu_kernel, dim3(blocks_for(M, kBnSlab), blocks_for(ldy, 64)), dim3(64, kBnWaves), 0, as_stream(stream),
                       z, ldz, M, C, mean, rstd, gamma, beta, y, ldy);
    note_kernel("bn_apply_relu_kernel");
    return check_launch("bn_apply_relu");
}

T2H_API int t2h_bn_running_update(const float *mean, const float *var, int M, int C, float momentum, float *running_mean,
                                  float *running_var, t2h_stream_t stream) {
    if (!mean || !var || !running_mean || !running_var) return fail(T2H_ERR_ARG, "bn_running_update: null pointer");
    if (!bn_shape_ok(M, C)) return fail(T2H_ERR_ARG, "bn_running_update: bad shape M=%d C=%d (M >= 2)", M, C);
    hipLaunchKernelGGL(bn_running_kernel, dim3(blocks_for(C, 256)), dim3(256), 0, as_stream(stream), mean, var, C, (float)M, momentum,
                       running_mean, running_var);
    note_kernel("bn_running_kernel");
    return check_launch("bn_running_update");
}

T2H_API int t2h_bn_bwd_reduce(const float *gy, int ldg, const float *y, int ldy, const float *z, int ldz, int M, int C,
                              const float *mean, const float *rstd, int relu, float *partial, float *dbeta, float *dgamma,
                              t2h_stream_t stream) {
    if (!gy || !z || !mean || !rstd || !partial || !dbeta || !dgamma || (relu && !y)) return fail(T2H_ERR_ARG, "bn_bwd_reduce: null pointer");
    if (!bn_shape_ok(M, C) || ldg < C || ldz < C || (relu && ldy < C))
        return fail(T2H_ERR_ARG, "bn_bwd_reduce: bad shape M=%d C=%d ldg=%d ldy=%d ldz=%d", M, C, ldg, ldy, ldz);
    hipStream_t s = as_stream(stream);
    const unsigned nslabs = blocks_for(M, kBnSlab);
    hipLaunchKernelGGL(bn_partial_kernel<2>, dim3(nslabs, blocks_for(C, 64)), dim3(64, kBnWaves), 0, s, z, ldz, M, C, mean, rstd, gy, ldg,
                       relu ? y : gy, relu ? ldy : ldg, relu ? 0u : 0xffffffffu, partial);      // (relu == 0: the mask is all ones)
    hipLaunchKernelGGL(bn_finish_kernel, dim3(blocks_for(C, 256)), dim3(256), 0, s, partial, (int)nslabs, C, 2, 1.0f, 0.0f, dbeta, dgamma);
    note_kernel("bn_partial_kernel");
    return check_launch("bn_bwd_reduce");
}

T2H_API int t2h_bn_bwd_apply(const float *gy, int ldg, const float *y, int ldy, const float *z, int ldz, int M, int C,
                             const float *mean, const float *rstd, const float *gamma, const float *dbeta, const float *dgamma,
                             int relu, float *dz, int gld, t2h_stream_t stream) {
    if (!gy || !z || !mean || !rstd || !gamma || !dbeta || !dgamma || !dz || (relu && !y))
        return fail(T2H_ERR_ARG, "bn_bwd_apply: null pointer");
    if (!bn_shape_ok(M, C) || ldg < C || ldz < C || (relu && ldy < C) || gld < C || gld > 64 * 65535)
        return fail(T2H_ERR_ARG, "bn_bwd_apply: bad shape M=%d C=%d ldg=%d ldy=%d ldz=%d gld=%d", M, C, ldg, ldy, ldz, gld);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(blocks_for(M, kBnSlab), blocks_for(gld, 64)), dim3(64, kBnWaves), 0, as_stream(stream),
                       gy, ldg, relu ? y : gy, relu ? ldy : ldg, z, ldz, M, C, mean, rstd, gamma, dbeta, dgamma, (float)M,
                       relu ? 0u : 0xffffffffu, dz, gld);
    note_kernel("bn_bwd_apply_kernel");
    return check_launch("bn_bwd_apply");
}
