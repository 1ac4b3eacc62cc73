// Exact median of every segment of a labelled list, on 32-bit keys (float32 values: dsm_instances.hip) or 64-bit keys (float64
// values: dsm_cloud.hip), and the one-workgroup statistics of the building-wise |d| that both files end with.
//
// The caller counts the members of each label into counts[0 .. K) and compacts (label, key) into label order at the CSR
// offsets made here, both from inside launch() below -- the slot inside a segment depends on arrival, an exact order
// statistic does not.  Then by size: up to 64 keys one wave ranks them in registers, up to 2 048 one workgroup sorts them in
// LDS, above that an 8-bit most-significant-digit radix select (one pass per byte of the key) with one histogram row per
// LARGE segment only; the wave that has read a row's histogram clears it for the next pass.  The key is the order-preserving
// image of the value; every NaN maps to the largest key.
//
// No spin-waits, no flags, no last-arriver combines: every dependency is a launch boundary.
#pragma once
#include <math.h>

#include "dsm_common.h"

namespace t2h {
namespace segmed {

constexpr int kTiny = 64, kSmall = 2048;                          // largest segment of the one-wave / one-workgroup class
constexpr int kChunk = 4096;                                      // compacted keys per workgroup of a select pass

template <typename Key> struct Traits;
template <> struct Traits<uint32_t> {
    typedef float Value;
    static constexpr uint32_t kNanKey = 0xffffffffu;
    __device__ static uint32_t encode(float v) {                  // a < b  <=>  key(a) < key(b); every NaN is the largest key
        uint32_t b = __float_as_uint(v);
        return isnan(v) ? kNanKey : b ^ ((uint32_t)((int)b >> 31) | 0x80000000u);
    }
    __device__ static float decode(uint32_t k) { return __uint_as_float(k ^ ((uint32_t)((int)~k >> 31) | 0x80000000u)); }
    __device__ static uint32_t shfl(uint32_t k, int src) { return __shfl(k, src); }
};
template <> struct Traits<uint64_t> {
    typedef double Value;
    static constexpr uint64_t kNanKey = 0xffffffffffffffffull;
    __device__ static uint64_t encode(double v) { return isnan(v) ? kNanKey : (uint64_t)key64(v); }
    __device__ static double decode(uint64_t k) { return value64(k); }
    __device__ static uint64_t shfl(uint64_t k, int src) {        // a 64-bit shuffle is two 32-bit ones
        const unsigned lo = __shfl((unsigned)k, src), hi = __shfl((unsigned)(k >> 32), src);
        return ((uint64_t)hi << 32) | lo;
    }
};
template <typename Key> constexpr int kPasses = (int)sizeof(Key);   // 8-bit digits

__device__ inline double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// np.median of a segment whose middle keys are klo <= khi and whose largest key is kmax, in float64: numpy takes the mean of
// ONE element for an odd count (no sum that could overflow) and of two for an even one.  The float32 entry rounds this once.
template <typename Key>
__device__ inline double middle(Key klo, Key khi, Key kmax, bool odd) {
    if (kmax == Traits<Key>::kNanKey) return quiet_nan();
    // (+ 0.0: numpy's mean starts its sum at +0, so the median of negative zeros is +0 there; no other value changes)
    if (odd) return (double)Traits<Key>::decode(khi) + 0.0;
    return ((double)Traits<Key>::decode(klo) + (double)Traits<Key>::decode(khi)) / 2.0 + 0.0;
}

struct Head { int n_member, n_large, pad[2]; };
template <typename Key> struct Row {                              // one per large segment, cleared before every call
    int seg, has_nan;
    unsigned rank[2];                                             // rank still to find, for (n-1)/2 and n/2
    Key prefix[2];                                                // digits chosen so far
};

inline int64_t rows_cap(int64_t n) { return n / (kSmall + 1) + 1; }
inline int scan_blocks(int K) { return (int)(((int64_t)K + kScanBlock - 1) / kScanBlock); }

template <typename Key> struct Layout {                           // byte offsets into the workspace, for n items and K labels
    size_t head, cursor, rows, hist, clear_end, offsets, rowidx, bsum_n, bsum_large, lab, key, end;
    Layout(int64_t n, int K) {
        const size_t nb = (size_t)scan_blocks(K), rc = (size_t)rows_cap(n);
        head = 0;
        cursor = up256(sizeof(Head));                             // the caller's compaction counts its arrivals here
        rows = cursor + up256(4 * (size_t)K);
        hist = rows + up256(rc * sizeof(Row<Key>));
        clear_end = hist + up256(rc * 512 * sizeof(unsigned));    // [0, clear_end) is zeroed before every call
        offsets = clear_end;
        rowidx = offsets + up256(4 * (size_t)K);
        bsum_n = rowidx + up256(4 * (size_t)K);
        bsum_large = bsum_n + up256(4 * nb);
        lab = bsum_large + up256(4 * nb);
        key = lab + up256(4 * (size_t)n);
        end = key + up256(sizeof(Key) * (size_t)n);
    }
};

static __global__ __launch_bounds__(256) void seg_sums_kernel(const int *__restrict__ counts, int K, int *__restrict__ bsum_n,
                                                              int *__restrict__ bsum_large) {
    const long long base = (long long)blockIdx.x * kScanBlock + 4 * threadIdx.x;
    int s = 0, g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < K) { int c = counts[base + j]; s += c; g += c > kSmall; }
    int ts, tg;
    block_scan(s, &ts);
    block_scan(g, &tg);
    if (threadIdx.x == 0) { bsum_n[blockIdx.x] = ts; bsum_large[blockIdx.x] = tg; }
}

template <typename Key>
__global__ __launch_bounds__(256) void seg_offsets_kernel(const int *__restrict__ counts, int K, const int *__restrict__ bsum_n,
                                                          const int *__restrict__ bsum_large, int *__restrict__ offsets,
                                                          int *__restrict__ rowidx, Row<Key> *__restrict__ rows, int rows_cap) {
    const long long base = (long long)blockIdx.x * kScanBlock + 4 * threadIdx.x;
    int c[4], s = 0, g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = base + j < K ? counts[base + j] : 0;
        s += c[j];
        g += c[j] > kSmall;
    }
    int ts, tg;
    int off = block_scan(s, &ts) + bsum_n[blockIdx.x];
    int row = block_scan(g, &tg) + bsum_large[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j >= K) break;
        offsets[base + j] = off;
        rowidx[base + j] = row;
        off += c[j];
        if (c[j] > kSmall) {
            if (row < rows_cap) {                                 // always: a large segment has more than kSmall of the n items
                Row<Key> *r = rows + row;
                r->seg = (int)(base + j);
                r->rank[0] = (unsigned)(c[j] - 1) >> 1;
                r->rank[1] = (unsigned)c[j] >> 1;
            }
            ++row;
        }
    }
}

// segments of 1 .. 64 keys (and empty ones: NaN), one wave each: a key's rank is the number of keys before it
template <typename Key>
__global__ __launch_bounds__(256) void tiny_kernel(const Key *__restrict__ key, const int *__restrict__ offsets,
                                                   const int *__restrict__ counts, int K,
                                                   typename Traits<Key>::Value *__restrict__ medians) {
    typedef Traits<Key> T;
    const long long s = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (s >= K) return;
    const int c = counts[s];
    if (c > kTiny) return;
    if (c < 1) {
        if (lane == 0) medians[s] = (typename T::Value)quiet_nan();
        return;
    }
    const Key k = lane < c ? key[(size_t)offsets[s] + lane] : T::kNanKey;
    int rank = 0;
    for (int j = 0; j < 64; ++j) {
        const Key kj = T::shfl(k, j);
        rank += kj < k || (kj == k && j < lane);
    }
    const Key klo = T::shfl(k, __ffsll((long long)__ballot(rank == (c - 1) / 2)) - 1);
    const Key khi = T::shfl(k, __ffsll((long long)__ballot(rank == c / 2)) - 1);
    const Key kmax = T::shfl(k, __ffsll((long long)__ballot(rank == c - 1)) - 1);
    if (lane == 0) medians[s] = (typename T::Value)middle(klo, khi, kmax, c & 1);
}

// segments of 65 .. 2 048 keys, one workgroup each: bitonic sort of the next power of two in LDS (8 KB or 16 KB)
template <typename Key>
__global__ __launch_bounds__(256) void small_kernel(const Key *__restrict__ key, const int *__restrict__ offsets,
                                                    const int *__restrict__ counts,
                                                    typename Traits<Key>::Value *__restrict__ medians) {
    __shared__ Key sk[kSmall];
    const int s = blockIdx.x, c = counts[s];
    if (c <= kTiny || c > kSmall) return;
    int m = 128;
    while (m < c) m <<= 1;
    const Key *src = key + (size_t)offsets[s];
    for (int i = threadIdx.x; i < m; i += 256) sk[i] = i < c ? src[i] : Traits<Key>::kNanKey;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < m; i += 256) {
                int o = i ^ j;
                if (o > i) {
                    Key a = sk[i], b = sk[o];
                    if ((a > b) == ((i & k) == 0)) { sk[i] = b; sk[o] = a; }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0)
        medians[s] = (typename Traits<Key>::Value)middle(sk[(c - 1) / 2], sk[c / 2], sk[c - 1], c & 1);
}

// one digit of the keys of the large segments that still match their prefix.  A chunk of 4 096 compacted keys meets at most
// three large segments (each has more than 2 048 keys), and their rows are consecutive: row & 3 names an LDS histogram.
template <typename Key>
__global__ __launch_bounds__(256) void select_pass_kernel(const int *__restrict__ lab, const Key *__restrict__ key,
                                                          const int *__restrict__ counts, const int *__restrict__ rowidx,
                                                          const Head *__restrict__ head, Row<Key> *rows, int pass,
                                                          unsigned *__restrict__ ghist) {
    __shared__ unsigned hist[4][2][256];
    __shared__ int rowof[4];
    const long long c0 = (long long)blockIdx.x * kChunk;
    const int n_member = head->n_member;
    if (c0 >= n_member || head->n_large == 0) return;
    for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256) (&hist[0][0][0])[i] = 0;
    if (threadIdx.x < 4) rowof[threadIdx.x] = -1;
    __syncthreads();
    const int shift = 8 * (kPasses<Key> - 1 - pass);
    const long long c1 = min(c0 + kChunk, (long long)n_member);
    for (long long i = c0 + threadIdx.x; i < c1; i += 256) {
        const int l = lab[i];
        if (counts[l - 1] <= kSmall) continue;
        const int row = rowidx[l - 1];
        const Key k = key[i];
        const Key high = pass == 0 ? (Key)0 : k >> (shift + 8);
        const unsigned digit = (unsigned)(k >> shift) & 255u;
        const Key p0 = rows[row].prefix[0], p1 = rows[row].prefix[1];   // written by the scan launch before this one
        rowof[row & 3] = row;
        if (high == p0) atomicAdd(&hist[row & 3][0][digit], 1u);
        if (high == p1) atomicAdd(&hist[row & 3][1][digit], 1u);
        if (pass == 0 && k == Traits<Key>::kNanKey) atomicOr(&rows[row].has_nan, 1);
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
template <typename Key>
__global__ __launch_bounds__(256) void select_scan_kernel(unsigned *ghist, const Head *__restrict__ head,
                                                          Row<Key> *__restrict__ rows, const int *__restrict__ counts, int pass,
                                                          typename Traits<Key>::Value *__restrict__ medians) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= head->n_large) return;
    Row<Key> *r = rows + row;
    Key done[2];
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
        const Key pk = r->prefix[k];
        const u64 found = __ballot(incl > rank);
        const int first = found ? __ffsll((long long)found) - 1 : 63;   // (found == 0 cannot happen while count > rank)
        unsigned rem = rank - (incl - own), j = 0;
        if (rem >= b0) { rem -= b0; j = 1;
            if (rem >= b1) { rem -= b1; j = 2;
                if (rem >= b2) { rem -= b2; j = 3; } } }
        const Key np = (pk << 8) | (Key)(4 * lane + j);
        done[k] = Traits<Key>::shfl(np, first);
        rem = __shfl(rem, first);
        // (every lane has read rank and prefix above: the ballot and the shuffles are behind those loads)
        if (lane == 0) { r->prefix[k] = done[k]; r->rank[k] = rem; }
    }
    if (pass == kPasses<Key> - 1 && lane == 0)
        medians[r->seg] = (typename Traits<Key>::Value)middle(done[0], done[1], r->has_nan ? Traits<Key>::kNanKey : (Key)0,
                                                              counts[r->seg] & 1);
}

// The whole launch sequence: the clears of [0, clear_end) and of counts, count() -- the caller's launch that counts the members
// of each label into counts --, the CSR offsets (a three-launch scan), compact(offsets, cursor, lab, key) -- the caller's launch
// that fills lab / key in label order --, then the size classes; the launches that cannot have work at this n are skipped.
// false if a clear could not be issued (nothing is launched then).
template <typename Key, typename Count, typename Compact>
bool launch(const Layout<Key> &L, int64_t n, int K, int *counts, typename Traits<Key>::Value *medians, void *workspace,
            hipStream_t s, Count count, Compact compact) {
    char *ws = reinterpret_cast<char *>(workspace);
    Head *head = reinterpret_cast<Head *>(ws + L.head);
    int *cursor = reinterpret_cast<int *>(ws + L.cursor), *offsets = reinterpret_cast<int *>(ws + L.offsets);
    int *rowidx = reinterpret_cast<int *>(ws + L.rowidx), *bsum_n = reinterpret_cast<int *>(ws + L.bsum_n);
    int *bsum_large = reinterpret_cast<int *>(ws + L.bsum_large), *lab = reinterpret_cast<int *>(ws + L.lab);
    Key *key = reinterpret_cast<Key *>(ws + L.key);
    unsigned *hist = reinterpret_cast<unsigned *>(ws + L.hist);
    Row<Key> *rows = reinterpret_cast<Row<Key> *>(ws + L.rows);
    const int rc = (int)rows_cap(n), nb = scan_blocks(K);
    if (hipMemsetAsync(ws, 0, L.clear_end, s) != hipSuccess || hipMemsetAsync(counts, 0, 4 * (size_t)K, s) != hipSuccess)
        return false;
    const dim3 block(256);
    count();
    hipLaunchKernelGGL(seg_sums_kernel, dim3(nb), block, 0, s, counts, K, bsum_n, bsum_large);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), block, 0, s, bsum_n, bsum_large, nb, &head->n_member);
    hipLaunchKernelGGL(seg_offsets_kernel<Key>, dim3(nb), block, 0, s, counts, K, bsum_n, bsum_large, offsets, rowidx, rows, rc);
    compact(offsets, cursor, lab, key);
    hipLaunchKernelGGL(tiny_kernel<Key>, dim3((unsigned)(((int64_t)K + 3) / 4)), block, 0, s, key, offsets, counts, K, medians);
    if (n > kTiny) hipLaunchKernelGGL(small_kernel<Key>, dim3(K), block, 0, s, key, offsets, counts, medians);
    if (n > kSmall)                                               // otherwise no segment can be large
        for (int pass = 0; pass < kPasses<Key>; ++pass) {
            hipLaunchKernelGGL(select_pass_kernel<Key>, dim3((unsigned)((n + kChunk - 1) / kChunk)), block, 0, s, lab, key, counts,
                               rowidx, head, rows, pass, hist);
            hipLaunchKernelGGL(select_scan_kernel<Key>, dim3((rc + 3) / 4), block, 0, s, hist, head, rows, counts, pass, medians);
        }
    return true;
}

// ------------------------------------------------------------------------------------------ building-wise aggregates
struct AbsStats { unsigned n; double sum, sum_sq, max, median; };

// Statistics of the |d| of the buildings i < K for which item(i, &d) is true.  Called by ONE workgroup of 256 threads, all of
// them.  Thread t takes the buildings t, t + 256, ... in order, then a fixed LDS tree: the same bytes every run.  The median is
// exact: an 8-bit radix select of each of the two middle ranks over the 64-bit keys; 0 if there is no such building.
template <typename Item>
__device__ inline AbsStats abs_stats(int K, Item item) {
    __shared__ double red[256][3];
    __shared__ unsigned cnt[256];
    __shared__ unsigned hist[256];
    __shared__ u64 sel_prefix;
    __shared__ unsigned sel_rank;
    const int t = threadIdx.x;
    double sa = 0.0, sq = 0.0, mx = 0.0;
    unsigned nv = 0;
    for (int i = t; i < K; i += 256) {
        double d;
        if (!item(i, &d)) continue;
        sa += d; sq += d * d; mx = fmax(mx, d); ++nv;
    }
    red[t][0] = sa; red[t][1] = sq; red[t][2] = mx; cnt[t] = nv;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) {
            red[t][0] += red[t + off][0];
            red[t][1] += red[t + off][1];
            red[t][2] = fmax(red[t][2], red[t + off][2]);
            cnt[t] += cnt[t + off];
        }
        __syncthreads();
    }
    const unsigned n = cnt[0];
    double med[2] = {0.0, 0.0};
    for (int k = 0; k < 2 && n > 0; ++k) {                        // ranks (n-1)/2 and n/2: an 8-bit radix select each
        if (k == 1 && (n & 1u)) break;
        __syncthreads();
        if (t == 0) { sel_prefix = 0; sel_rank = k ? n >> 1 : (n - 1) >> 1; }
        for (int pass = 0; pass < 8; ++pass) {
            hist[t] = 0;
            __syncthreads();
            const int shift = 56 - 8 * pass;
            const u64 prefix = sel_prefix;
            for (int i = t; i < K; i += 256) {
                double d;
                if (!item(i, &d)) continue;
                const u64 key = key64(d);
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
        med[k] = value64(sel_prefix);
    }
    AbsStats r;
    r.n = n; r.sum = red[0][0]; r.sum_sq = red[0][1]; r.max = red[0][2];
    r.median = (n & 1u) ? med[0] : (med[0] + med[1]) / 2.0;
    return r;
}

}  // namespace segmed
}  // namespace t2h
