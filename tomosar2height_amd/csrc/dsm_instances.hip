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
// MEDIANS: counts per label (integer atomics, one per label and wave), then seg_median.h on 32-bit keys: exclusive scan to
// CSR offsets, compaction of (label, key) into label order (here, again one atomic per label and wave), and the median of
// every segment by size class.  The key is the order-preserving image of the float32 value; every NaN maps to the largest key.
//
// Compare results and vector selects: like dsm_eval.hip this runs after generate_dsm(), never beside
// a training step, so the rule for kernels that share a CU with the split convolutions does not bind here.
#include <math.h>

#include "seg_median.h"
#include "../../include/t2h_inst.h"

namespace t2h {

typedef segmed::Traits<uint32_t> InstKey;
static_assert(segmed::kTiny == T2H_INST_TINY_MAX && segmed::kSmall == T2H_INST_SMALL_MAX, "size classes of t2h_inst.h");

constexpr int kTile = T2H_INST_TILE;                              // 32 x 32 pixels, 4 per thread
constexpr int kTilePix = kTile * kTile;
constexpr int64_t kInstMaxPixels = 0x7fffffff;

#define T2H_LD_WG(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define T2H_LD_AGENT(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

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

template <typename T>
__global__ __launch_bounds__(256) void inst_compact_kernel(const T *__restrict__ values, int ld, int W, int n,
                                                           const int *__restrict__ labels, int K,
                                                           const int *__restrict__ offsets, int *__restrict__ cursor,
                                                           int *__restrict__ lab, uint32_t *__restrict__ key) {
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
                key[slot] = InstKey::encode((float)values[(size_t)y * ld + x]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ building-wise aggregates
// ONE workgroup (segmed::abs_stats)
__global__ __launch_bounds__(256) void inst_metrics_kernel(const float *__restrict__ pm, const float *__restrict__ gm, int K,
                                                           double *__restrict__ table) {
    const segmed::AbsStats st = segmed::abs_stats(K, [=](int i, double *d) {
        const float p = pm[i], g = gm[i];
        *d = fabs((double)p - (double)g);
        return isfinite(p) && isfinite(g);
    });
    if (threadIdx.x == 0) {
        table[0] = (double)st.n; table[1] = (double)((unsigned)K - st.n);
        table[2] = st.sum; table[3] = st.sum_sq;
        table[4] = st.median; table[5] = st.max;
        table[6] = table[7] = 0.0;
    }
}

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
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), block, 0, s, bsum, (int *)nullptr, nb, n_labels);
    hipLaunchKernelGGL(inst_rank_kernel, dim3(nb), block, 0, s, Q, P, n, bsum);
    hipLaunchKernelGGL(inst_relabel_kernel, dim3(flat_wgs(n, 4096)), block, 0, s, Q, P, n);
    note_kernel("inst_merge_kernel");
    return check_launch("inst_label");
}

T2H_API size_t t2h_inst_medians_workspace_bytes(int64_t n, int K) {
    if (n < 1 || n > kInstMaxPixels || K < 0 || K > n) return 0;
    return segmed::Layout<uint32_t>(n, K).end;
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
    const segmed::Layout<uint32_t> L(n, K);
    if (workspace_bytes < L.end)
        return fail(T2H_ERR_WORKSPACE, "inst_medians: workspace %zu < %zu bytes", workspace_bytes, L.end);
    if (K == 0) return 0;
    hipStream_t s = as_stream(stream);
    const dim3 block(256), flat(flat_wgs(n, 4096));
    const auto count = [&] { hipLaunchKernelGGL(inst_count_kernel, flat, block, 0, s, labels, n, K, counts); };
    const auto compact = [&](const int *offsets, int *cursor, int *lab, uint32_t *key) {
        if (is_f64)
            hipLaunchKernelGGL(inst_compact_kernel<double>, flat, block, 0, s, (const double *)values, ld, W, n, labels, K, offsets,
                               cursor, lab, key);
        else
            hipLaunchKernelGGL(inst_compact_kernel<float>, flat, block, 0, s, (const float *)values, ld, W, n, labels, K, offsets,
                               cursor, lab, key);
    };
    if (!segmed::launch(L, n, K, counts, medians, workspace, s, count, compact)) return check_launch("inst_medians (clear)");
    note_kernel("select_pass_kernel");
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
