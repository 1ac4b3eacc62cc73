// Building-instance metrics on the device (reference: scripts/evaluator_instance.py:15-57; ABI in include/t2h_inst.h).
//
// LABELS: union-find by label equivalence.  P is the parent plane (the caller's label plane), Q the flattened one (workspace).
//   1. local    one workgroup per 32 x 32 tile resolves its pixels in LDS (integer LDS atomics) and writes the GLOBAL linear
//               index of each pixel's tile-local root (-1 for background).
//   2. merge    one thread per pixel of a tile's first row / first column unites it with its in-mask neighbours across the
//               edge.  Every access of P in this launch is an agent-scope relaxed atomic (L2-served), and nothing depends on
//               freshness: parents only decrease, so a stale parent is still an ancestor, and the fixed point -- every
//               component rooted at its smallest linear index -- is unique.  No waits, no flags, no last arriver.
//   3. flatten  a launch of its own (the boundary makes step 2 visible): Q[i] = root of i; roots counted per 1 024 pixels.
//   4. scan     one workgroup: exclusive scan of those counts; K.
//   5. rank     P[root] = 1 + number of roots before it in raster order: the component's label.
//   6. relabel  P[i] = P[Q[i]] for the other foreground pixels, 0 for background.
//
// MEDIANS: counts per label (integer atomics, one per label and wave), exclusive scan to CSR offsets, compaction of
// (label, key) into label order -- the slot inside a segment depends on arrival, an exact order statistic does not -- then by
// size: up to 64 keys one wave ranks them in registers, up to 2 048 one workgroup sorts them in LDS, above that an 8-bit
// most-significant-digit radix select (4 passes over the 32-bit keys) with one histogram row per LARGE segment only.  The
// key is the order-preserving image of the float32 value; every NaN maps to the largest key.
//
// Compare results and vector selects: like dsm_eval.hip this runs after generate_dsm(), never beside
// a training step, so the rule for kernels that share a CU with the split convolutions does not bind here.
#include <math.h>

#include "t2h_common.h"
#include "../../include/t2h_inst.h"

namespace t2h {

typedef unsigned long long u64;

constexpr int kTile = T2H_INST_TILE;                              // 32 x 32 pixels, 4 per thread
constexpr int kTilePix = kTile * kTile;
constexpr int kScanBlock = 1024;                                  // items per workgroup of the scans (4 per thread)
constexpr int kTiny = T2H_INST_TINY_MAX, kSmall = T2H_INST_SMALL_MAX;
constexpr int kChunk = 4096;                                      // compacted keys per workgroup of a select pass
constexpr unsigned kNanKey = 0xffffffffu;
constexpr int64_t kInstMaxPixels = 0x7fffffff;

#define T2H_LD_WG(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define T2H_LD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// exclusive prefix of v over the 256 threads of the workgroup (thread order) and the workgroup's total
__device__ inline int block_scan(int v, int *total) {
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

// ------------------------------------------------------------------------------------------ labels
__device__ inline int lds_find(int *par, int x) {
    int p;
    while ((p = T2H_LD_WG(&par[x])) != x) x = p;
    return x;
}
__device__ inline void lds_unite(int *par, int a, int b) {
    for (;;) {
        a = lds_find(par, a);
        b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }                   // a > b: hang the larger root under the smaller
        int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;                                                  // a was no root any more: unite what it pointed to
    }
}

template <int CONN>
__global__ __launch_bounds__(256) void inst_local_kernel(const uint8_t *__restrict__ mask, int ld, int R, int C,
                                                         int *__restrict__ P) {
    __shared__ int par[kTilePix];
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int li = threadIdx.x + 256 * k, y = y0 + (li >> 5), x = x0 + (li & 31);
        bool fg = y < R && x < C && mask[(size_t)y * ld + x] != 0;
        par[li] = fg ? li : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int li = threadIdx.x + 256 * k, ly = li >> 5, lx = li & 31;
        if (T2H_LD_WG(&par[li]) < 0) continue;
        if (lx > 0 && T2H_LD_WG(&par[li - 1]) >= 0) lds_unite(par, li, li - 1);
        if (ly > 0) {
            if (T2H_LD_WG(&par[li - kTile]) >= 0) lds_unite(par, li, li - kTile);
            if (CONN == 2) {
                if (lx > 0 && T2H_LD_WG(&par[li - kTile - 1]) >= 0) lds_unite(par, li, li - kTile - 1);
                if (lx < kTile - 1 && T2H_LD_WG(&par[li - kTile + 1]) >= 0) lds_unite(par, li, li - kTile + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int li = threadIdx.x + 256 * k, y = y0 + (li >> 5), x = x0 + (li & 31);
        if (y >= R || x >= C) continue;
        int v = -1;
        if (par[li] >= 0) {
            int r = lds_find(par, li);
            v = (y0 + (r >> 5)) * C + x0 + (r & 31);
        }
        P[(size_t)y * C + x] = v;
    }
}

__device__ inline int agent_find(int *P, int x) {
    int p;
    while ((p = T2H_LD_AGENT(&P[x])) != x) x = p;
    return x;
}
__device__ inline void agent_unite(int *P, int a, int b) {
    for (;;) {
        a = agent_find(P, a);
        b = agent_find(P, b);
        if (a == b) return;
        if (a < b) { int t = a; a = b; b = t; }
        int old = __hip_atomic_fetch_min(&P[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}
// q = (x, y) if it is inside the plane and foreground, united with p
__device__ inline void agent_try(int *P, int R, int C, int p, int x, int y) {
    if (x < 0 || y < 0 || x >= C || y >= R) return;
    int q = y * C + x;
    if (T2H_LD_AGENT(&P[q]) >= 0) agent_unite(P, p, q);
}

// threads [0, rows_n): pixel x of tile boundary row 32 * (1 + i / C) with the row above; the rest: pixel y of boundary column
// 32 * (1 + j / R) with the column to its left.  A pair of neighbours that lies in two tiles is met by one of the two.
template <int CONN>
__global__ __launch_bounds__(256) void inst_merge_kernel(int *P, int R, int C, long long rows_n, long long total) {
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (i < rows_n) {
        int x = (int)(i % C), y = kTile * (1 + (int)(i / C)), p = y * C + x;
        if (T2H_LD_AGENT(&P[p]) < 0) return;
        agent_try(P, R, C, p, x, y - 1);
        if (CONN == 2) {
            agent_try(P, R, C, p, x - 1, y - 1);
            agent_try(P, R, C, p, x + 1, y - 1);
        }
    } else {
        long long j = i - rows_n;
        int y = (int)(j % R), x = kTile * (1 + (int)(j / R)), p = y * C + x;
        if (T2H_LD_AGENT(&P[p]) < 0) return;
        agent_try(P, R, C, p, x - 1, y);
        if (CONN == 2) {
            agent_try(P, R, C, p, x - 1, y - 1);
            agent_try(P, R, C, p, x - 1, y + 1);
        }
    }
}

__global__ __launch_bounds__(256) void inst_flatten_kernel(const int *__restrict__ P, int *__restrict__ Q, int n,
                                                           int *__restrict__ bsum) {
    const long long base = (long long)blockIdx.x * kScanBlock + 4 * threadIdx.x;
    int roots = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        long long i = base + j;
        if (i >= n) break;
        int r = P[i];
        if (r >= 0) {
            int p;
            while ((p = P[r]) != r) r = p;
            roots += r == (int)i;
        }
        Q[i] = r;
    }
    int total;
    block_scan(roots, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: a[0 .. nb) (and b, if given) to their exclusive prefixes in place; the totals to total[0] (and total[1])
__global__ __launch_bounds__(256) void inst_scan_kernel(int *__restrict__ a, int *__restrict__ b, int nb,
                                                        int *__restrict__ total) {
    const int per = (nb + 255) / 256, lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    for (int s = 0; s < 2; ++s) {
        int *v = s ? b : a;
        if (!v) break;
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += v[i];
        int tot, run = block_scan(sum, &tot);
        for (int i = lo; i < hi; ++i) { int t = v[i]; v[i] = run; run += t; }
        if (threadIdx.x == 0) total[s] = tot;
    }
}

__global__ __launch_bounds__(256) void inst_rank_kernel(const int *__restrict__ Q, int *__restrict__ P, int n,
                                                        const int *__restrict__ bsum) {
    const long long base = (long long)blockIdx.x * kScanBlock + 4 * threadIdx.x;
    int roots = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) roots += base + j < n && Q[base + j] == (int)(base + j);
    int total, rank = block_scan(roots, &total) + bsum[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < n && Q[base + j] == (int)(base + j)) P[base + j] = ++rank;
}

// (no __restrict__ on P: the words read -- roots -- are not the words written -- everything else -- but they share the plane)
__global__ __launch_bounds__(256) void inst_relabel_kernel(const int *__restrict__ Q, int *P, int n) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        int r = Q[i];
        if (r < 0) P[i] = 0;
        else if (r != (int)i) P[i] = P[r];
    }
}

// ------------------------------------------------------------------------------------------ segmented medians
struct InstHead { int n_member, n_large, pad[2]; };
struct InstRow {                                                  // one per large segment, cleared before every call
    int seg, has_nan;
    unsigned prefix[2], rank[2];                                  // digits chosen so far / rank still to find, for (n-1)/2 and n/2
};

__device__ inline unsigned inst_key(float v) {                    // a < b  <=>  key(a) < key(b); every NaN is the largest key
    unsigned b = __float_as_uint(v);
    return isnan(v) ? kNanKey : b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
}
__device__ inline float inst_value(unsigned k) {
    return __uint_as_float(k ^ ((unsigned)((int)~k >> 31) | 0x80000000u));
}
__device__ inline float inst_middle(unsigned klo, unsigned khi, unsigned kmax) {
    if (kmax == kNanKey) return __uint_as_float(0x7fc00000u);
    // (+ 0.0: numpy's mean starts its sum at +0, so the median of negative zeros is +0 there; no other value changes)
    return (float)(((double)inst_value(klo) + (double)inst_value(khi)) / 2.0 + 0.0);
}

// ctr[l - 1] += (lanes of this wave with label l); returns each active lane's place among them.  One atomic per distinct
// label and wave: a building's pixels are neighbours, so mostly one or two.  Called by whole waves.
__device__ inline int wave_take(int *ctr, int l, bool active) {
    const int lane = threadIdx.x & 63;
    int slot = 0;
    u64 todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int ll = __shfl(l, leader);
        const u64 same = __ballot(active && l == ll);
        int base = 0;
        if (lane == leader) base = atomicAdd(&ctr[ll - 1], __popcll(same));
        base = __shfl(base, leader);
        if (active && l == ll) slot = base + __popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return slot;
}

__global__ __launch_bounds__(256) void inst_count_kernel(const int *__restrict__ labels, int n, int K,
                                                         int *__restrict__ counts) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i0 = (long long)blockIdx.x * 256; i0 < n; i0 += stride) {   // uniform trip count per workgroup
        long long i = i0 + threadIdx.x;
        int l = i < n ? labels[i] : 0;
        wave_take(counts, l, l >= 1 && l <= K);
    }
}

__global__ __launch_bounds__(256) void inst_seg_sums_kernel(const int *__restrict__ counts, int K, int *__restrict__ bsum_n,
                                                            int *__restrict__ bsum_large) {
    const int base = blockIdx.x * kScanBlock + 4 * threadIdx.x;
    int s = 0, g = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < K) { int c = counts[base + j]; s += c; g += c > kSmall; }
    int ts, tg;
    block_scan(s, &ts);
    block_scan(g, &tg);
    if (threadIdx.x == 0) { bsum_n[blockIdx.x] = ts; bsum_large[blockIdx.x] = tg; }
}

__global__ __launch_bounds__(256) void inst_seg_offsets_kernel(const int *__restrict__ counts, int K,
                                                               const int *__restrict__ bsum_n,
                                                               const int *__restrict__ bsum_large, int *__restrict__ offsets,
                                                               int *__restrict__ rowidx, InstRow *__restrict__ rows,
                                                               int rows_cap) {
    const int base = blockIdx.x * kScanBlock + 4 * threadIdx.x;
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
            if (row < rows_cap) {                                 // always: a large segment has more than kSmall of the n pixels
                InstRow *r = rows + row;
                r->seg = base + j;
                r->rank[0] = (unsigned)(c[j] - 1) >> 1;
                r->rank[1] = (unsigned)c[j] >> 1;
            }
            ++row;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void inst_compact_kernel(const T *__restrict__ values, int ld, int W, int n,
                                                           const int *__restrict__ labels, int K,
                                                           const int *__restrict__ offsets, int *__restrict__ cursor,
                                                           int *__restrict__ lab, unsigned *__restrict__ key) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i0 = (long long)blockIdx.x * 256; i0 < n; i0 += stride) {
        long long i = i0 + threadIdx.x;
        int l = i < n ? labels[i] : 0;
        const bool active = l >= 1 && l <= K;
        const int place = wave_take(cursor, l, active);
        if (active) {
            int y = (int)(i / W), x = (int)(i - (long long)y * W);
            long long slot = (long long)offsets[l - 1] + place;
            if (slot < n) {                                       // always, for counts taken from the same labels
                lab[slot] = l;
                key[slot] = inst_key((float)values[(size_t)y * ld + x]);
            }
        }
    }
}

// segments of 1 .. 64 keys (and empty ones: NaN), one wave each: a key's rank is the number of keys before it
__global__ __launch_bounds__(256) void inst_tiny_kernel(const unsigned *__restrict__ key, const int *__restrict__ offsets,
                                                        const int *__restrict__ counts, int K, float *__restrict__ medians) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= K) return;
    const int c = counts[s];
    if (c > kTiny) return;
    if (c < 1) {
        if (lane == 0) medians[s] = __uint_as_float(0x7fc00000u);
        return;
    }
    const unsigned k = lane < c ? key[(size_t)offsets[s] + lane] : kNanKey;
    int rank = 0;
    for (int j = 0; j < 64; ++j) {
        unsigned kj = __shfl(k, j);
        rank += kj < k || (kj == k && j < lane);
    }
    const unsigned klo = __shfl(k, __ffsll((long long)__ballot(rank == (c - 1) / 2)) - 1);
    const unsigned khi = __shfl(k, __ffsll((long long)__ballot(rank == c / 2)) - 1);
    const unsigned kmax = __shfl(k, __ffsll((long long)__ballot(rank == c - 1)) - 1);
    if (lane == 0) medians[s] = inst_middle(klo, khi, kmax);
}

// segments of 65 .. 2 048 keys, one workgroup each: bitonic sort of the next power of two in LDS
__global__ __launch_bounds__(256) void inst_small_kernel(const unsigned *__restrict__ key, const int *__restrict__ offsets,
                                                         const int *__restrict__ counts, float *__restrict__ medians) {
    __shared__ unsigned sk[kSmall];
    const int s = blockIdx.x, c = counts[s];
    if (c <= kTiny || c > kSmall) return;
    int m = 128;
    while (m < c) m <<= 1;
    const unsigned *src = key + (size_t)offsets[s];
    for (int i = threadIdx.x; i < m; i += 256) sk[i] = i < c ? src[i] : kNanKey;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < m; i += 256) {
                int o = i ^ j;
                if (o > i) {
                    unsigned a = sk[i], b = sk[o];
                    if ((a > b) == ((i & k) == 0)) { sk[i] = b; sk[o] = a; }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) medians[s] = inst_middle(sk[(c - 1) / 2], sk[c / 2], sk[c - 1]);
}

// one digit of the keys of the large segments that still match their prefix.  A chunk of 4 096 compacted keys meets at most
// three large segments (each has more than 2 048 keys), and their rows are consecutive: row & 3 names an LDS histogram.
__global__ __launch_bounds__(256) void inst_select_pass_kernel(const int *__restrict__ lab, const unsigned *__restrict__ key,
                                                               const int *__restrict__ counts, const int *__restrict__ rowidx,
                                                               const InstHead *__restrict__ head, InstRow *rows, int pass,
                                                               unsigned *__restrict__ ghist) {
    __shared__ unsigned hist[4][2][256];
    __shared__ int rowof[4];
    const long long c0 = (long long)blockIdx.x * kChunk;
    const int n_member = head->n_member;
    if (c0 >= n_member || head->n_large == 0) return;
    for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256) (&hist[0][0][0])[i] = 0;
    if (threadIdx.x < 4) rowof[threadIdx.x] = -1;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const long long c1 = min(c0 + kChunk, (long long)n_member);
    for (long long i = c0 + threadIdx.x; i < c1; i += 256) {
        const int l = lab[i];
        if (counts[l - 1] <= kSmall) continue;
        const int row = rowidx[l - 1];
        const unsigned k = key[i];
        const unsigned high = pass == 0 ? 0u : k >> (shift + 8), digit = (k >> shift) & 255u;
        const unsigned p0 = rows[row].prefix[0], p1 = rows[row].prefix[1];   // written by the scan launch before this one
        rowof[row & 3] = row;
        if (high == p0) atomicAdd(&hist[row & 3][0][digit], 1u);
        if (high == p1) atomicAdd(&hist[row & 3][1][digit], 1u);
        if (pass == 0 && k == kNanKey) atomicOr(&rows[row].has_nan, 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256) {
        const unsigned v = (&hist[0][0][0])[i];
        const int row = rowof[i >> 9];
        if (v && row >= 0) atomicAdd(&ghist[(size_t)row * 512 + (i & 511)], v);
    }
}

// one wave per large segment: both ranks pick their digit from the merged histogram; the last pass writes the median
__global__ __launch_bounds__(256) void inst_select_scan_kernel(const unsigned *__restrict__ ghist,
                                                               const InstHead *__restrict__ head, InstRow *__restrict__ rows,
                                                               int pass, float *__restrict__ medians) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= head->n_large) return;
    InstRow *r = rows + row;
    unsigned done[2];
    for (int k = 0; k < 2; ++k) {
        const unsigned *b = ghist + (size_t)row * 512 + k * 256 + 4 * lane;
        const unsigned b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3], own = b0 + b1 + b2 + b3;
        unsigned incl = own;
        for (int off = 1; off < 64; off <<= 1) {
            unsigned up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        const unsigned rank = r->rank[k], pk = r->prefix[k];
        const u64 found = __ballot(incl > rank);
        const int first = found ? __ffsll((long long)found) - 1 : 63;   // (found == 0 cannot happen while count > rank)
        unsigned rem = rank - (incl - own), j = 0;
        if (rem >= b0) { rem -= b0; j = 1;
            if (rem >= b1) { rem -= b1; j = 2;
                if (rem >= b2) { rem -= b2; j = 3; } } }
        const unsigned np = (pk << 8) | (unsigned)(4 * lane + j);
        done[k] = __shfl(np, first);
        rem = __shfl(rem, first);
        if (lane == 0) { r->prefix[k] = done[k]; r->rank[k] = rem; }
    }
    if (pass == 3 && lane == 0) medians[r->seg] = inst_middle(done[0], done[1], r->has_nan ? kNanKey : 0u);
}

// ------------------------------------------------------------------------------------------ building-wise aggregates
__device__ inline u64 inst_key64(double v) {
    u64 b = (u64)__double_as_longlong(v);
    return b ^ ((u64)((long long)b >> 63) | 0x8000000000000000ull);
}
__device__ inline double inst_value64(u64 k) {
    return __longlong_as_double((long long)(k ^ ((u64)((long long)~k >> 63) | 0x8000000000000000ull)));
}

// ONE workgroup.  Thread t takes the buildings t, t + 256, ... in order, then a fixed LDS tree: the same bytes every run.
__global__ __launch_bounds__(256) void inst_metrics_kernel(const float *__restrict__ pm, const float *__restrict__ gm, int K,
                                                           double *__restrict__ table) {
    __shared__ double red[256][3];
    __shared__ unsigned cnt[256];
    __shared__ unsigned hist[256];
    __shared__ u64 sel_prefix;
    __shared__ unsigned sel_rank;
    const int t = threadIdx.x;
    double sa = 0.0, sq = 0.0, mx = 0.0;
    unsigned nv = 0;
    for (int i = t; i < K; i += 256) {
        float p = pm[i], g = gm[i];
        if (!(isfinite(p) && isfinite(g))) continue;
        double d = fabs((double)p - (double)g);
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
        if (k == 1 && (n & 1u)) { med[1] = med[0]; break; }
        __syncthreads();
        if (t == 0) { sel_prefix = 0; sel_rank = k ? n >> 1 : (n - 1) >> 1; }
        for (int pass = 0; pass < 8; ++pass) {
            hist[t] = 0;
            __syncthreads();
            const int shift = 56 - 8 * pass;
            const u64 prefix = sel_prefix;
            for (int i = t; i < K; i += 256) {
                float p = pm[i], g = gm[i];
                if (!(isfinite(p) && isfinite(g))) continue;
                u64 key = inst_key64(fabs((double)p - (double)g));
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (t == 0) {
                unsigned rank = sel_rank, d = 0;
                while (d < 255 && rank >= hist[d]) rank -= hist[d++];
                sel_prefix = (prefix << 8) | d;
                sel_rank = rank;
            }
            __syncthreads();
        }
        med[k] = inst_value64(sel_prefix);
    }
    if (t == 0) {
        table[0] = (double)n; table[1] = (double)((unsigned)K - n);
        table[2] = red[0][0]; table[3] = red[0][1];
        table[4] = (med[0] + med[1]) / 2.0; table[5] = red[0][2];
        table[6] = table[7] = 0.0;
    }
}

// ------------------------------------------------------------------------------------------ host side
static size_t up256(size_t b) { return (b + 255) / 256 * 256; }
static int flat_wgs(int64_t n, int cap) {
    int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > cap ? cap : g);
}
static int64_t rows_cap(int64_t n) { return n / (kSmall + 1) + 1; }

struct MedianLayout {                                             // byte offsets into the workspace
    size_t head, cursor, rows, hist, clear_end, offsets, rowidx, bsum_n, bsum_large, lab, key, end;
    MedianLayout(int64_t n, int K) {
        const size_t nb = ((size_t)K + kScanBlock - 1) / kScanBlock, rc = (size_t)rows_cap(n);
        head = 0;
        cursor = up256(sizeof(InstHead));
        rows = cursor + up256(4 * (size_t)K);
        hist = rows + up256(rc * sizeof(InstRow));
        clear_end = hist + up256(rc * 4 * 512 * sizeof(unsigned));   // [0, clear_end) is zeroed before every call
        offsets = clear_end;
        rowidx = offsets + up256(4 * (size_t)K);
        bsum_n = rowidx + up256(4 * (size_t)K);
        bsum_large = bsum_n + up256(4 * nb);
        lab = bsum_large + up256(4 * nb);
        key = lab + up256(4 * (size_t)n);
        end = key + up256(4 * (size_t)n);
    }
};

}  // namespace t2h

using namespace t2h;

T2H_API size_t t2h_inst_label_workspace_bytes(int R, int C) {
    if (R < 1 || C < 1 || (int64_t)R * C > kInstMaxPixels) return 0;
    const size_t n = (size_t)R * C;
    return up256(4 * n) + up256(4 * ((n + kScanBlock - 1) / kScanBlock));
}

T2H_API int t2h_inst_label(const uint8_t *mask, int ld, int R, int C, int connectivity, int32_t *labels, int32_t *n_labels,
                           void *workspace, size_t workspace_bytes, t2h_stream_t stream) {
    if (!mask || !labels || !n_labels || !workspace) return fail(T2H_ERR_ARG, "inst_label: null pointer");
    if (R < 1 || C < 1 || (int64_t)R * C > kInstMaxPixels)
        return fail(T2H_ERR_ARG, "inst_label: bad shape %d x %d (1 .. 2^31 - 1 pixels)", R, C);
    if (ld < C) return fail(T2H_ERR_ARG, "inst_label: row pitch %d < %d columns", ld, C);
    if (connectivity != 1 && connectivity != 2)
        return fail(T2H_ERR_ARG, "inst_label: connectivity = %d (1: 4 neighbours, 2: 8 neighbours)", connectivity);
    if (((uintptr_t)labels & 3) || ((uintptr_t)n_labels & 3) || ((uintptr_t)workspace & 3))
        return fail(T2H_ERR_ARG, "inst_label: labels / n_labels / workspace must be 4-byte aligned");
    const size_t need = t2h_inst_label_workspace_bytes(R, C);
    if (workspace_bytes < need) return fail(T2H_ERR_WORKSPACE, "inst_label: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const int n = R * C, nb = (n + kScanBlock - 1) / kScanBlock;
    int *P = labels, *Q = reinterpret_cast<int *>(workspace);
    int *bsum = reinterpret_cast<int *>(reinterpret_cast<char *>(workspace) + up256(4 * (size_t)n));
    const int tx = (C + kTile - 1) / kTile, ty = (R + kTile - 1) / kTile;
    const long long rows_n = (long long)(ty - 1) * C, total = rows_n + (long long)(tx - 1) * R;
    const dim3 tiles(tx, ty), block(256);
    if (connectivity == 2) hipLaunchKernelGGL(inst_local_kernel<2>, tiles, block, 0, s, mask, ld, R, C, P);
    else hipLaunchKernelGGL(inst_local_kernel<1>, tiles, block, 0, s, mask, ld, R, C, P);
    if (total > 0) {
        const dim3 grid((unsigned)((total + 255) / 256));
        if (connectivity == 2) hipLaunchKernelGGL(inst_merge_kernel<2>, grid, block, 0, s, P, R, C, rows_n, total);
        else hipLaunchKernelGGL(inst_merge_kernel<1>, grid, block, 0, s, P, R, C, rows_n, total);
    }
    hipLaunchKernelGGL(inst_flatten_kernel, dim3(nb), block, 0, s, P, Q, n, bsum);
    hipLaunchKernelGGL(inst_scan_kernel, dim3(1), block, 0, s, bsum, (int *)nullptr, nb, n_labels);
    hipLaunchKernelGGL(inst_rank_kernel, dim3(nb), block, 0, s, Q, P, n, bsum);
    hipLaunchKernelGGL(inst_relabel_kernel, dim3(flat_wgs(n, 4096)), block, 0, s, Q, P, n);
    note_kernel("inst_merge_kernel");
    return check_launch("inst_label");
}

T2H_API size_t t2h_inst_medians_workspace_bytes(int64_t n, int K) {
    if (n < 1 || n > kInstMaxPixels || K < 0 || K > n) return 0;
    return MedianLayout(n, K).end;
}

T2H_API int t2h_inst_medians(const void *values, int is_f64, int ld, int H, int W, const int32_t *labels, int K,
                             int32_t *counts, float *medians, void *workspace, size_t workspace_bytes, t2h_stream_t stream) {
    if (!values || !labels || !counts || !medians || !workspace) return fail(T2H_ERR_ARG, "inst_medians: null pointer");
    if (H < 1 || W < 1 || (int64_t)H * W > kInstMaxPixels)
        return fail(T2H_ERR_ARG, "inst_medians: bad shape %d x %d (1 .. 2^31 - 1 pixels)", H, W);
    if (ld < W) return fail(T2H_ERR_ARG, "inst_medians: row pitch %d < %d columns", ld, W);
    if (K < 0 || K > (int64_t)H * W) return fail(T2H_ERR_ARG, "inst_medians: K = %d labels for %d x %d pixels", K, H, W);
    if (is_f64 != 0 && is_f64 != 1) return fail(T2H_ERR_ARG, "inst_medians: is_f64 = %d (0, 1)", is_f64);
    if (((uintptr_t)values & (is_f64 ? 7 : 3)) || ((uintptr_t)labels & 3) || ((uintptr_t)counts & 3) ||
        ((uintptr_t)medians & 3) || ((uintptr_t)workspace & 15))
        return fail(T2H_ERR_ARG, "inst_medians: misaligned pointer (workspace: 16 bytes, planes: their element)");
    const int n = H * W;
    const MedianLayout L(n, K);
    if (workspace_bytes < L.end)
        return fail(T2H_ERR_WORKSPACE, "inst_medians: workspace %zu < %zu bytes", workspace_bytes, L.end);
    if (K == 0) return 0;
    hipStream_t s = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    InstHead *head = reinterpret_cast<InstHead *>(ws + L.head);
    int *cursor = reinterpret_cast<int *>(ws + L.cursor), *offsets = reinterpret_cast<int *>(ws + L.offsets);
    int *rowidx = reinterpret_cast<int *>(ws + L.rowidx), *bsum_n = reinterpret_cast<int *>(ws + L.bsum_n);
    int *bsum_large = reinterpret_cast<int *>(ws + L.bsum_large), *lab = reinterpret_cast<int *>(ws + L.lab);
    unsigned *key = reinterpret_cast<unsigned *>(ws + L.key), *hist = reinterpret_cast<unsigned *>(ws + L.hist);
    InstRow *rows = reinterpret_cast<InstRow *>(ws + L.rows);
    const int rc = (int)rows_cap(n), nb = (K + kScanBlock - 1) / kScanBlock;
    if (hipMemsetAsync(ws, 0, L.clear_end, s) != hipSuccess || hipMemsetAsync(counts, 0, 4 * (size_t)K, s) != hipSuccess)
        return check_launch("inst_medians (clear)");
    const dim3 block(256), flat(flat_wgs(n, 4096));
    hipLaunchKernelGGL(inst_count_kernel, flat, block, 0, s, labels, n, K, counts);
    hipLaunchKernelGGL(inst_seg_sums_kernel, dim3(nb), block, 0, s, counts, K, bsum_n, bsum_large);
    hipLaunchKernelGGL(inst_scan_kernel, dim3(1), block, 0, s, bsum_n, bsum_large, nb, &head->n_member);
    hipLaunchKernelGGL(inst_seg_offsets_kernel, dim3(nb), block, 0, s, counts, K, bsum_n, bsum_large, offsets, rowidx, rows, rc);
    if (is_f64)
        hipLaunchKernelGGL(inst_compact_kernel<double>, flat, block, 0, s, (const double *)values, ld, W, n, labels, K, offsets,
                           cursor, lab, key);
    else
        hipLaunchKernelGGL(inst_compact_kernel<float>, flat, block, 0, s, (const float *)values, ld, W, n, labels, K, offsets,
                           cursor, lab, key);
    hipLaunchKernelGGL(inst_tiny_kernel, dim3((K + 3) / 4), block, 0, s, key, offsets, counts, K, medians);
    hipLaunchKernelGGL(inst_small_kernel, dim3(K), block, 0, s, key, offsets, counts, medians);
    if (n > kSmall)                                               // otherwise no segment can be large
        for (int pass = 0; pass < 4; ++pass) {
            unsigned *h = hist + (size_t)pass * rc * 512;
            hipLaunchKernelGGL(inst_select_pass_kernel, dim3((n + kChunk - 1) / kChunk), block, 0, s, lab, key, counts, rowidx,
                               head, rows, pass, h);
            hipLaunchKernelGGL(inst_select_scan_kernel, dim3((rc + 3) / 4), block, 0, s, h, head, rows, pass, medians);
        }
    note_kernel("inst_select_pass_kernel");
    return check_launch("inst_medians");
}

T2H_API int t2h_inst_metrics(const float *pred_med, const float *gt_med, int K, double *table, t2h_stream_t stream) {
    if (!pred_med || !gt_med || !table) return fail(T2H_ERR_ARG, "inst_metrics: null pointer");
    if (K < 0) return fail(T2H_ERR_ARG, "inst_metrics: K = %d", K);
    if (((uintptr_t)pred_med & 3) || ((uintptr_t)gt_med & 3) || ((uintptr_t)table & 7))
        return fail(T2H_ERR_ARG, "inst_metrics: misaligned pointer");
    hipLaunchKernelGGL(inst_metrics_kernel, dim3(1), dim3(256), 0, as_stream(stream), pred_med, gt_med, K, table);
    return check_launch("inst_metrics");
}
