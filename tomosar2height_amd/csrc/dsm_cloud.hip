// Point-cloud building-wise metrics on the device (reference: scripts/evaluator_instance.py:139-291; ABI in include/t2h_cloud.h).
//
// ASSIGN: one thread per point: the inverse raster transform with separate roundings, floor, a clip in float64, one gather
// from the label plane.
//
// MEDIANS: the structure of dsm_instances.hip on 64-bit keys and an unordered point list.  Counts per label (one integer
// atomic per member point: points arrive in any order, so the "a wave's pixels share a label" shortcut of the raster variant
// does not apply), exclusive scan to CSR offsets, compaction of (label, key) into label order -- the slot inside a segment
// depends on arrival, an exact order statistic does not -- then by size: up to 64 keys one wave ranks them in registers
// (a 64-bit shuffle is two 32-bit ones), up to 2 048 one workgroup sorts them in 16 KB of LDS, above that an 8-bit
// most-significant-digit radix select (8 passes over the 64-bit keys) with one histogram row per LARGE segment only; the wave
// that has read a row's histogram clears it for the next pass.  The key is the order-preserving image of the float64 value;
// every NaN maps to the largest key.
//
// METRICS: one workgroup, fixed-order float64 sums, exact radix select of |d|.
//
// No spin-waits, no flags, no last-arriver combines: every dependency is a launch boundary.
// Compare results and vector selects: like dsm_instances.hip this runs after a cloud is loaded, never
// beside a training step, so the rule for kernels that share a CU with the split convolutions does not bind here.
#include <float.h>
#include <math.h>

#include "t2h_common.h"
#include "../../include/t2h_cloud.h"

namespace t2h {

typedef unsigned long long cu64;

constexpr int kCloudScanBlock = 1024;                             // items per workgroup of the scans (4 per thread)
constexpr int kCloudTiny = T2H_CLOUD_TINY_MAX, kCloudSmall = T2H_CLOUD_SMALL_MAX;
constexpr int kCloudChunk = 4096;                                 // compacted keys per workgroup of a select pass
constexpr cu64 kCloudNanKey = 0xffffffffffffffffull;
constexpr int64_t kCloudMaxItems = 0x7fffffff;

// exclusive prefix of v over the 256 threads of the workgroup (thread order) and the workgroup's total
__device__ inline int cloud_block_scan(int v, int *total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
    }
    __syncthreads();                                              // (a previous call's readers are done with wsum)
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + incl - v;
}

__device__ inline cu64 cloud_shfl64(cu64 v, int src) {
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((cu64)hi << 32) | lo;
}

__device__ inline cu64 cloud_key(double v) {                      // a < b  <=>  key(a) < key(b); every NaN is the largest key
    cu64 b = (cu64)__double_as_longlong(v);
    return isnan(v) ? kCloudNanKey : b ^ ((cu64)((long long)b >> 63) | 0x8000000000000000ull);
}
__device__ inline double cloud_value(cu64 k) {
    return __longlong_as_double((long long)(k ^ ((cu64)((long long)~k >> 63) | 0x8000000000000000ull)));
}
// np.median of a segment whose middle keys are klo <= khi and whose largest key is kmax: numpy takes the mean of ONE element
// for an odd count (no sum that could overflow) and of two for an even one
__device__ inline double cloud_middle(cu64 klo, cu64 khi, cu64 kmax, bool odd) {
    if (kmax == kCloudNanKey) return __longlong_as_double(0x7ff8000000000000ll);
    // (+ 0.0: numpy's mean starts its sum at +0, so the median of negative zeros is +0 there; no other value changes)
    if (odd) return cloud_value(khi) + 0.0;
    return (cloud_value(klo) + cloud_value(khi)) / 2.0 + 0.0;
}

// ------------------------------------------------------------------------------------------ assign
__global__ __launch_bounds__(256) void cloud_assign_kernel(const double *__restrict__ pts, long long N, long long stride,
                                                           double ra, double rb, double rc, double rd, double re, double rf,
                                                           const int *__restrict__ labels, int R, int C,
                                                           int *__restrict__ point_label, int *__restrict__ n_bad) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += step) {
        const double x = pts[i * stride], y = pts[i * stride + 1];
        const double fx = __dadd_rn(__dadd_rn(__dmul_rn(x, ra), __dmul_rn(y, rb)), rc);
        const double fy = __dadd_rn(__dadd_rn(__dmul_rn(x, rd), __dmul_rn(y, re)), rf);
        int l = 0;
        if (isfinite(x) && isfinite(y) && !isnan(fx) && !isnan(fy)) {
            const int col = (int)fmin(fmax(floor(fx), 0.0), (double)(C - 1));   // clipped before the conversion
            const int row = (int)fmin(fmax(floor(fy), 0.0), (double)(R - 1));
            l = labels[(size_t)row * C + col];
        } else {
            atomicAdd(n_bad, 1);
        }
        point_label[i] = l;
    }
}

// ------------------------------------------------------------------------------------------ segmented medians
struct CloudHead { int n_member, n_large, pad[2]; };
struct CloudRow {                                                 // one per large segment, cleared before every call
    int seg, has_nan;
    unsigned rank[2];                                             // rank still to find, for (n-1)/2 and n/2
    cu64 prefix[2];                                               // digits chosen so far
};

__global__ __launch_bounds__(256) void cloud_count_kernel(const int *__restrict__ point_label, long long N, int K,
                                                          int *__restrict__ counts) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += step) {
        const int l = point_label[i];
        if (l >= 1 && l <= K) atomicAdd(&counts[l - 1], 1);
    }
}

__global__ __launch_bounds__(256) void cloud_seg_sums_kernel(const int *__restrict__ counts, int K, int *__restrict__ bsum_n,
                                                             int *__restrict__ bsum_large) {
    const long long base = (long long)blockIdx.x * kCloudScanBlock + 4 * threadIdx.x;
    int s = 0, g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < K) { int c = counts[base + j]; s += c; g += c > kCloudSmall; }
    int ts, tg;
    cloud_block_scan(s, &ts);
    cloud_block_scan(g, &tg);
    if (threadIdx.x == 0) { bsum_n[blockIdx.x] = ts; bsum_large[blockIdx.x] = tg; }
}

// one workgroup: a[0 .. nb) and b[0 .. nb) to their exclusive prefixes in place; the totals to total[0] and total[1]
__global__ __launch_bounds__(256) void cloud_scan_kernel(int *__restrict__ a, int *__restrict__ b, int nb,
                                                         int *__restrict__ total) {
    const int per = (nb + 255) / 256, lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    for (int s = 0; s < 2; ++s) {
        int *v = s ? b : a;
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += v[i];
        int tot, run = cloud_block_scan(sum, &tot);
        for (int i = lo; i < hi; ++i) { int t = v[i]; v[i] = run; run += t; }
        if (threadIdx.x == 0) total[s] = tot;
    }
}

__global__ __launch_bounds__(256) void cloud_seg_offsets_kernel(const int *__restrict__ counts, int K,
                                                                const int *__restrict__ bsum_n,
                                                                const int *__restrict__ bsum_large, int *__restrict__ offsets,
                                                                int *__restrict__ rowidx, CloudRow *__restrict__ rows,
                                                                int rows_cap) {
    const long long base = (long long)blockIdx.x * kCloudScanBlock + 4 * threadIdx.x;
    int c[4], s = 0, g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = base + j < K ? counts[base + j] : 0;
        s += c[j];
        g += c[j] > kCloudSmall;
    }
    int ts, tg;
    int off = cloud_block_scan(s, &ts) + bsum_n[blockIdx.x];
    int row = cloud_block_scan(g, &tg) + bsum_large[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j >= K) break;
        offsets[base + j] = off;
        rowidx[base + j] = row;
        off += c[j];
        if (c[j] > kCloudSmall) {
            if (row < rows_cap) {                                 // always: a large segment has more than kCloudSmall of the N points
                CloudRow *r = rows + row;
                r->seg = (int)(base + j);
                r->rank[0] = (unsigned)(c[j] - 1) >> 1;
                r->rank[1] = (unsigned)c[j] >> 1;
            }
            ++row;
        }
    }
}

__global__ __launch_bounds__(256) void cloud_compact_kernel(const double *__restrict__ z, long long stride,
                                                            const int *__restrict__ point_label, long long N, int K,
                                                            const int *__restrict__ offsets, int *__restrict__ cursor,
                                                            int *__restrict__ lab, cu64 *__restrict__ key) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += step) {
        const int l = point_label[i];
        if (l < 1 || l > K) continue;
        const long long slot = (long long)offsets[l - 1] + atomicAdd(&cursor[l - 1], 1);
        if (slot < N) {                                           // always, for counts taken from the same labels
            lab[slot] = l;
            key[slot] = cloud_key(z[i * stride]);
        }
    }
}

// segments of 1 .. 64 keys (and empty ones: NaN), one wave each: a key's rank is the number of keys before it
__global__ __launch_bounds__(256) void cloud_tiny_kernel(const cu64 *__restrict__ key, const int *__restrict__ offsets,
                                                         const int *__restrict__ counts, int K, double *__restrict__ medians) {
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= K) return;
    const int c = counts[s];
    if (c > kCloudTiny) return;
    if (c < 1) {
        if (lane == 0) medians[s] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const cu64 k = lane < c ? key[(size_t)offsets[s] + lane] : kCloudNanKey;
    int rank = 0;
    for (int j = 0; j < 64; ++j) {
        const cu64 kj = cloud_shfl64(k, j);
        rank += kj < k || (kj == k && j < lane);
    }
    const cu64 klo = cloud_shfl64(k, __ffsll((long long)__ballot(rank == (c - 1) / 2)) - 1);
    const cu64 khi = cloud_shfl64(k, __ffsll((long long)__ballot(rank == c / 2)) - 1);
    const cu64 kmax = cloud_shfl64(k, __ffsll((long long)__ballot(rank == c - 1)) - 1);
    if (lane == 0) medians[s] = cloud_middle(klo, khi, kmax, c & 1);
}

// segments of 65 .. 2 048 keys, one workgroup each: bitonic sort of the next power of two in LDS
__global__ __launch_bounds__(256) void cloud_small_kernel(const cu64 *__restrict__ key, const int *__restrict__ offsets,
                                                          const int *__restrict__ counts, double *__restrict__ medians) {
    __shared__ cu64 sk[kCloudSmall];
    const int s = blockIdx.x, c = counts[s];
    if (c <= kCloudTiny || c > kCloudSmall) return;
    int m = 128;
    while (m < c) m <<= 1;
    const cu64 *src = key + (size_t)offsets[s];
    for (int i = threadIdx.x; i < m; i += 256) sk[i] = i < c ? src[i] : kCloudNanKey;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < m; i += 256) {
                int o = i ^ j;
                if (o > i) {
                    cu64 a = sk[i], b = sk[o];
                    if ((a > b) == ((i & k) == 0)) { sk[i] = b; sk[o] = a; }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) medians[s] = cloud_middle(sk[(c - 1) / 2], sk[c / 2], sk[c - 1], c & 1);
}

// one digit of the keys of the large segments that still match their prefix.  A chunk of 4 096 compacted keys meets at most
// three large segments (each has more than 2 048 keys), and their rows are consecutive: row & 3 names an LDS histogram.
__global__ __launch_bounds__(256) void cloud_select_pass_kernel(const int *__restrict__ lab, const cu64 *__restrict__ key,
                                                                const int *__restrict__ counts, const int *__restrict__ rowidx,
                                                                const CloudHead *__restrict__ head, CloudRow *rows, int pass,
                                                                unsigned *__restrict__ ghist) {
    __shared__ unsigned hist[4][2][256];
    __shared__ int rowof[4];
    const long long c0 = (long long)blockIdx.x * kCloudChunk;
    const int n_member = head->n_member;
    if (c0 >= n_member || head->n_large == 0) return;
    for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256) (&hist[0][0][0])[i] = 0;
    if (threadIdx.x < 4) rowof[threadIdx.x] = -1;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const long long c1 = min(c0 + kCloudChunk, (long long)n_member);
    for (long long i = c0 + threadIdx.x; i < c1; i += 256) {
        const int l = lab[i];
        if (counts[l - 1] <= kCloudSmall) continue;
        const int row = rowidx[l - 1];
        const cu64 k = key[i];
        const cu64 high = pass == 0 ? 0ull : k >> (shift + 8);
        const unsigned digit = (unsigned)(k >> shift) & 255u;
        const cu64 p0 = rows[row].prefix[0], p1 = rows[row].prefix[1];   // written by the scan launch before this one
        rowof[row & 3] = row;
        if (high == p0) atomicAdd(&hist[row & 3][0][digit], 1u);
        if (high == p1) atomicAdd(&hist[row & 3][1][digit], 1u);
        if (pass == 0 && k == kCloudNanKey) atomicOr(&rows[row].has_nan, 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256) {
        const unsigned v = (&hist[0][0][0])[i];
        const int row = rowof[i >> 9];
        if (v && row >= 0) atomicAdd(&ghist[(size_t)row * 512 + (i & 511)], v);
    }
}

// one wave per large segment: both ranks pick their digit from the merged histogram, and the row is cleared for the next
// pass (a later launch); the last pass writes the median
__global__ __launch_bounds__(256) void cloud_select_scan_kernel(unsigned *ghist, const CloudHead *__restrict__ head,
                                                                CloudRow *__restrict__ rows, const int *__restrict__ counts,
                                                                int pass, double *__restrict__ medians) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= head->n_large) return;
    CloudRow *r = rows + row;
    cu64 done[2];
    for (int k = 0; k < 2; ++k) {
        unsigned *b = ghist + (size_t)row * 512 + k * 256 + 4 * lane;
        const unsigned b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3], own = b0 + b1 + b2 + b3;
        b[0] = b[1] = b[2] = b[3] = 0u;
        unsigned incl = own;
        for (int off = 1; off < 64; off <<= 1) {
            unsigned up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        const unsigned rank = r->rank[k];
        const cu64 pk = r->prefix[k];
        const cu64 found = __ballot(incl > rank);
        const int first = found ? __ffsll((long long)found) - 1 : 63;   // (found == 0 cannot happen while count > rank)
        unsigned rem = rank - (incl - own), j = 0;
        if (rem >= b0) { rem -= b0; j = 1;
            if (rem >= b1) { rem -= b1; j = 2;
                if (rem >= b2) { rem -= b2; j = 3; } } }
        const cu64 np = (pk << 8) | (cu64)(4 * lane + j);
        done[k] = cloud_shfl64(np, first);
        rem = __shfl(rem, first);
        // (every lane has read rank and prefix above: the ballot and the shuffles are behind those loads)
        if (lane == 0) { r->prefix[k] = done[k]; r->rank[k] = rem; }
    }
    if (pass == 7 && lane == 0)
        medians[r->seg] = cloud_middle(done[0], done[1], r->has_nan ? kCloudNanKey : 0ull, counts[r->seg] & 1);
}

// ------------------------------------------------------------------------------------------ building-wise aggregates
// |d| of building i, or false if the mode leaves it out; *h = the height before any NaN handling
__device__ inline bool cloud_diff(double pm, float dtm, float ref, int mode, double *h, double *d) {
    double v = pm - (double)dtm;
    *h = v;
    if (mode == T2H_CLOUD_MODE_ALL) {                             // np.nan_to_num
        if (isnan(v)) v = 0.0;
        else if (isinf(v)) v = v > 0.0 ? DBL_MAX : -DBL_MAX;
    } else if (isnan(v)) {
        return false;
    }
    if (isnan(ref)) return false;
    *d = fabs((double)ref - v);
    return true;
}

// ONE workgroup.  Thread t takes the buildings t, t + 256, ... in order, then a fixed LDS tree: the same bytes every run.
__global__ __launch_bounds__(256) void cloud_metrics_kernel(const double *__restrict__ pm, const float *__restrict__ dm,
                                                            const float *__restrict__ rm, const int *__restrict__ counts,
                                                            int K, int mode, const int *__restrict__ n_bad,
                                                            double *__restrict__ height, double *__restrict__ table) {
    __shared__ double red[256][3];
    __shared__ unsigned cnt[256][2];
    __shared__ unsigned hist[256];
    __shared__ cu64 sel_prefix;
    __shared__ unsigned sel_rank;
    const int t = threadIdx.x;
    double sa = 0.0, sq = 0.0, mx = 0.0;
    unsigned nv = 0, nc = 0;
    for (int i = t; i < K; i += 256) {
        double h, d;
        const bool ok = cloud_diff(pm[i], dm[i], rm[i], mode, &h, &d);
        height[i] = h;
        nc += counts[i] > 0;
        if (!ok) continue;
        sa += d; sq += d * d; mx = fmax(mx, d); ++nv;
    }
    red[t][0] = sa; red[t][1] = sq; red[t][2] = mx; cnt[t][0] = nv; cnt[t][1] = nc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) {
            red[t][0] += red[t + off][0];
            red[t][1] += red[t + off][1];
            red[t][2] = fmax(red[t][2], red[t + off][2]);
            cnt[t][0] += cnt[t + off][0];
            cnt[t][1] += cnt[t + off][1];
        }
        __syncthreads();
    }
    const unsigned n = cnt[0][0];
    double med[2] = {0.0, 0.0};
    for (int k = 0; k < 2 && n > 0; ++k) {                        // ranks (n-1)/2 and n/2: an 8-bit radix select each
        if (k == 1 && (n & 1u)) { med[1] = med[0]; break; }
        __syncthreads();
        if (t == 0) { sel_prefix = 0; sel_rank = k ? n >> 1 : (n - 1) >> 1; }
        for (int pass = 0; pass < 8; ++pass) {
            hist[t] = 0;
            __syncthreads();
            const int shift = 56 - 8 * pass;
            const cu64 prefix = sel_prefix;
            for (int i = t; i < K; i += 256) {
                double h, d;
                if (!cloud_diff(pm[i], dm[i], rm[i], mode, &h, &d)) continue;
                const cu64 key = cloud_key(d);
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (t == 0) {
                unsigned rank = sel_rank, dg = 0;
                while (dg < 255 && rank >= hist[dg]) rank -= hist[dg++];
                sel_prefix = (prefix << 8) | dg;
                sel_rank = rank;
            }
            __syncthreads();
        }
        med[k] = cloud_value(sel_prefix);
    }
    if (t == 0) {
        table[0] = (double)n; table[1] = (double)((unsigned)K - n);
        table[2] = red[0][0]; table[3] = red[0][1];
        table[4] = (n & 1u) ? med[0] : (med[0] + med[1]) / 2.0; table[5] = red[0][2];
        table[6] = (double)cnt[0][1];
        table[7] = n_bad ? (double)*n_bad : 0.0;
    }
}

// ------------------------------------------------------------------------------------------ host side
static size_t cloud_up256(size_t b) { return (b + 255) / 256 * 256; }
static int cloud_flat_wgs(int64_t n, int cap) {
    int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > cap ? cap : g);
}
static int64_t cloud_rows_cap(int64_t n) { return n / (kCloudSmall + 1) + 1; }

struct CloudLayout {                                              // byte offsets into the workspace
    size_t head, cursor, rows, hist, clear_end, offsets, rowidx, bsum_n, bsum_large, lab, key, end;
    CloudLayout(int64_t n, int K) {
        const size_t nb = ((size_t)K + kCloudScanBlock - 1) / kCloudScanBlock, rc = (size_t)cloud_rows_cap(n);
        head = 0;
        cursor = cloud_up256(sizeof(CloudHead));
        rows = cursor + cloud_up256(4 * (size_t)K);
        hist = rows + cloud_up256(rc * sizeof(CloudRow));
        clear_end = hist + cloud_up256(rc * 512 * sizeof(unsigned));   // [0, clear_end) is zeroed before every call
        offsets = clear_end;
        rowidx = offsets + cloud_up256(4 * (size_t)K);
        bsum_n = rowidx + cloud_up256(4 * (size_t)K);
        bsum_large = bsum_n + cloud_up256(4 * nb);
        lab = bsum_large + cloud_up256(4 * nb);
        key = lab + cloud_up256(4 * (size_t)n);
        end = key + cloud_up256(8 * (size_t)n);
    }
};

}  // namespace t2h

using namespace t2h;

T2H_API int t2h_cloud_assign(const double *points, int64_t N, int64_t stride, double ra, double rb, double rc, double rd,
                             double re, double rf, const int32_t *labels, int R, int C, int32_t *point_label, int32_t *n_bad,
                             t2h_stream_t stream) {
    if (!labels || !n_bad || (N > 0 && (!points || !point_label))) return fail(T2H_ERR_ARG, "cloud_assign: null pointer");
    if (N < 0 || N > kCloudMaxItems) return fail(T2H_ERR_ARG, "cloud_assign: N = %lld points (0 .. 2^31 - 1)", (long long)N);
    if (stride < 2 || stride > kCloudMaxItems) return fail(T2H_ERR_ARG, "cloud_assign: row stride %lld (2 .. 2^31 - 1 doubles)", (long long)stride);
    if (R < 1 || C < 1 || (int64_t)R * C > kCloudMaxItems)
        return fail(T2H_ERR_ARG, "cloud_assign: bad raster %d x %d (1 .. 2^31 - 1 pixels)", R, C);
    if (!(isfinite(ra) && isfinite(rb) && isfinite(rc) && isfinite(rd) && isfinite(re) && isfinite(rf)))
        return fail(T2H_ERR_ARG, "cloud_assign: a coefficient of the inverse transform is not finite");
    if (((uintptr_t)points & 7) || ((uintptr_t)labels & 3) || ((uintptr_t)point_label & 3) || ((uintptr_t)n_bad & 3))
        return fail(T2H_ERR_ARG, "cloud_assign: misaligned pointer");
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(n_bad, 0, 4, s) != hipSuccess) return check_launch("cloud_assign (clear)");
    if (N > 0)
        hipLaunchKernelGGL(cloud_assign_kernel, dim3(cloud_flat_wgs(N, 8192)), dim3(256), 0, s, points, (long long)N,
                           (long long)stride, ra, rb, rc, rd, re, rf, labels, R, C, point_label, n_bad);
    return check_launch("cloud_assign");
}

T2H_API size_t t2h_cloud_medians_workspace_bytes(int64_t N, int K) {
    if (N < 0 || N > kCloudMaxItems || K < 0) return 0;
    return CloudLayout(N, K).end;
}

T2H_API int t2h_cloud_medians(const double *z, int64_t stride, const int32_t *point_label, int64_t N, int K, int32_t *counts,
                              double *medians, void *workspace, size_t workspace_bytes, t2h_stream_t stream) {
    if (!workspace || (N > 0 && (!z || !point_label)) || (K > 0 && (!counts || !medians)))
        return fail(T2H_ERR_ARG, "cloud_medians: null pointer");
    if (N < 0 || N > kCloudMaxItems) return fail(T2H_ERR_ARG, "cloud_medians: N = %lld points (0 .. 2^31 - 1)", (long long)N);
    if (stride < 1 || stride > kCloudMaxItems) return fail(T2H_ERR_ARG, "cloud_medians: stride %lld (1 .. 2^31 - 1 doubles)", (long long)stride);
    if (K < 0) return fail(T2H_ERR_ARG, "cloud_medians: K = %d labels", K);
    if (((uintptr_t)z & 7) || ((uintptr_t)point_label & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)medians & 7) ||
        ((uintptr_t)workspace & 15))
        return fail(T2H_ERR_ARG, "cloud_medians: misaligned pointer (workspace: 16 bytes, arrays: their element)");
    const CloudLayout L(N, K);
    if (workspace_bytes < L.end)
        return fail(T2H_ERR_WORKSPACE, "cloud_medians: workspace %zu < %zu bytes", workspace_bytes, L.end);
    if (K == 0) return 0;
    hipStream_t s = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    CloudHead *head = reinterpret_cast<CloudHead *>(ws + L.head);
    int *cursor = reinterpret_cast<int *>(ws + L.cursor), *offsets = reinterpret_cast<int *>(ws + L.offsets);
    int *rowidx = reinterpret_cast<int *>(ws + L.rowidx), *bsum_n = reinterpret_cast<int *>(ws + L.bsum_n);
    int *bsum_large = reinterpret_cast<int *>(ws + L.bsum_large), *lab = reinterpret_cast<int *>(ws + L.lab);
    cu64 *key = reinterpret_cast<cu64 *>(ws + L.key);
    unsigned *hist = reinterpret_cast<unsigned *>(ws + L.hist);
    CloudRow *rows = reinterpret_cast<CloudRow *>(ws + L.rows);
    const int rc = (int)cloud_rows_cap(N), nb = (K + kCloudScanBlock - 1) / kCloudScanBlock;
    if (hipMemsetAsync(ws, 0, L.clear_end, s) != hipSuccess || hipMemsetAsync(counts, 0, 4 * (size_t)K, s) != hipSuccess)
        return check_launch("cloud_medians (clear)");
    const dim3 block(256), flat(cloud_flat_wgs(N, 8192));
    if (N > 0) hipLaunchKernelGGL(cloud_count_kernel, flat, block, 0, s, point_label, (long long)N, K, counts);
    hipLaunchKernelGGL(cloud_seg_sums_kernel, dim3(nb), block, 0, s, counts, K, bsum_n, bsum_large);
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(1), block, 0, s, bsum_n, bsum_large, nb, &head->n_member);
    hipLaunchKernelGGL(cloud_seg_offsets_kernel, dim3(nb), block, 0, s, counts, K, bsum_n, bsum_large, offsets, rowidx, rows, rc);
    if (N > 0)
        hipLaunchKernelGGL(cloud_compact_kernel, flat, block, 0, s, z, (long long)stride, point_label, (long long)N, K, offsets,
                           cursor, lab, key);
    hipLaunchKernelGGL(cloud_tiny_kernel, dim3((unsigned)(((int64_t)K + 3) / 4)), block, 0, s, key, offsets, counts, K, medians);
    if (N > kCloudTiny) hipLaunchKernelGGL(cloud_small_kernel, dim3(K), block, 0, s, key, offsets, counts, medians);
    if (N > kCloudSmall)                                          // otherwise no segment can be large
        for (int pass = 0; pass < 8; ++pass) {
            hipLaunchKernelGGL(cloud_select_pass_kernel, dim3((unsigned)((N + kCloudChunk - 1) / kCloudChunk)), block, 0, s, lab,
                               key, counts, rowidx, head, rows, pass, hist);
            hipLaunchKernelGGL(cloud_select_scan_kernel, dim3((rc + 3) / 4), block, 0, s, hist, head, rows, counts, pass, medians);
        }
    note_kernel("cloud_select_pass_kernel");
    return check_launch("cloud_medians");
}

T2H_API int t2h_cloud_metrics(const double *pred_med, const float *dtm_med, const float *ref_med, const int32_t *counts, int K,
                              int mode, const int32_t *n_bad, double *height, double *table, t2h_stream_t stream) {
    if (!table || (K > 0 && (!pred_med || !dtm_med || !ref_med || !counts || !height)))
        return fail(T2H_ERR_ARG, "cloud_metrics: null pointer");
    if (K < 0) return fail(T2H_ERR_ARG, "cloud_metrics: K = %d", K);
    if (mode != T2H_CLOUD_MODE_VALID_ONLY && mode != T2H_CLOUD_MODE_ALL)
        return fail(T2H_ERR_ARG, "cloud_metrics: mode = %d (0: valid only, 1: all)", mode);
    if (((uintptr_t)pred_med & 7) || ((uintptr_t)dtm_med & 3) || ((uintptr_t)ref_med & 3) || ((uintptr_t)counts & 3) ||
        ((uintptr_t)n_bad & 3) || ((uintptr_t)height & 7) || ((uintptr_t)table & 7))
        return fail(T2H_ERR_ARG, "cloud_metrics: misaligned pointer");
    hipLaunchKernelGGL(cloud_metrics_kernel, dim3(1), dim3(256), 0, as_stream(stream), pred_med, dtm_med, ref_med, counts, K, mode,
                       n_bad, height, table);
    return check_launch("cloud_metrics");
}
