// Point-cloud building-wise metrics on the device (reference: scripts/evaluator_instance.py:139-291; ABI in include/t2h_cloud.h).
//
// ASSIGN: one thread per point: the inverse raster transform with separate roundings, floor, a clip in float64, one gather
// from the label plane.
//
// MEDIANS: seg_median.h on 64-bit keys and an unordered point list.  Counts per label and the compaction of (label, key) into
// label order take one integer atomic per member point: points arrive in any order, so the "a wave's pixels share a label"
// shortcut of the raster variant does not apply.  The key is the order-preserving image of the float64 value; every NaN maps
// to the largest key.
//
// METRICS: one workgroup, fixed-order float64 sums, exact radix select of |d| (segmed::abs_stats).
//
// No spin-waits, no flags, no last-arriver combines: every dependency is a launch boundary.
// Compare results and vector selects: like dsm_instances.hip this runs after a cloud is loaded, never
// beside a training step, so the rule for kernels that share a CU with the split convolutions does not bind here.
#include <float.h>
#include <math.h>

#include "seg_median.h"
#include "../../include/t2h_cloud.h"

namespace t2h {

typedef segmed::Traits<uint64_t> CloudKey;
static_assert(segmed::kTiny == T2H_CLOUD_TINY_MAX && segmed::kSmall == T2H_CLOUD_SMALL_MAX, "size classes of t2h_cloud.h");
constexpr int64_t kCloudMaxItems = 0x7fffffff;

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
__global__ __launch_bounds__(256) void cloud_count_kernel(const int *__restrict__ point_label, long long N, int K,
                                                          int *__restrict__ counts) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += step) {
        const int l = point_label[i];
        if (l >= 1 && l <= K) atomicAdd(&counts[l - 1], 1);
    }
}

__global__ __launch_bounds__(256) void cloud_compact_kernel(const double *__restrict__ z, long long stride,
                                                            const int *__restrict__ point_label, long long N, int K,
                                                            const int *__restrict__ offsets, int *__restrict__ cursor,
                                                            int *__restrict__ lab, uint64_t *__restrict__ key) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += step) {
        const int l = point_label[i];
        if (l < 1 || l > K) continue;
        const long long slot = (long long)offsets[l - 1] + atomicAdd(&cursor[l - 1], 1);
        if (slot < N) {                                           // always, for counts taken from the same labels
            lab[slot] = l;
            key[slot] = CloudKey::encode(z[i * stride]);
        }
    }
}

// ------------------------------------------------------------------------------------------ building-wise aggregates
// |d| of a building of height v (before any NaN handling), or false if the mode leaves it out
__device__ inline bool cloud_diff(double v, float ref, int mode, double *d) {
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

// ONE workgroup: the heights and the number of buildings with a point here, the statistics of |d| by segmed::abs_stats
__global__ __launch_bounds__(256) void cloud_metrics_kernel(const double *__restrict__ pm, const float *__restrict__ dm,
                                                            const float *__restrict__ rm, const int *__restrict__ counts,
                                                            int K, int mode, const int *__restrict__ n_bad,
                                                            double *__restrict__ height, double *__restrict__ table) {
    __shared__ unsigned covered[256];
    const int t = threadIdx.x;
    unsigned nc = 0;
    for (int i = t; i < K; i += 256) {
        height[i] = pm[i] - (double)dm[i];
        nc += counts[i] > 0;
    }
    covered[t] = nc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) covered[t] += covered[t + off];
        __syncthreads();
    }
    const segmed::AbsStats st =
        segmed::abs_stats(K, [=](int i, double *d) { return cloud_diff(pm[i] - (double)dm[i], rm[i], mode, d); });
    if (t == 0) {
        table[0] = (double)st.n; table[1] = (double)((unsigned)K - st.n);
        table[2] = st.sum; table[3] = st.sum_sq;
        table[4] = st.median; table[5] = st.max;
        table[6] = (double)covered[0];
        table[7] = n_bad ? (double)*n_bad : 0.0;
    }
}

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
        hipLaunchKernelGGL(cloud_assign_kernel, dim3(flat_wgs(N, 8192)), dim3(256), 0, s, points, (long long)N,
                           (long long)stride, ra, rb, rc, rd, re, rf, labels, R, C, point_label, n_bad);
    return check_launch("cloud_assign");
}

T2H_API size_t t2h_cloud_medians_workspace_bytes(int64_t N, int K) {
    if (N < 0 || N > kCloudMaxItems || K < 0) return 0;
    return segmed::Layout<uint64_t>(N, K).end;
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
    const segmed::Layout<uint64_t> L(N, K);
    if (workspace_bytes < L.end)
        return fail(T2H_ERR_WORKSPACE, "cloud_medians: workspace %zu < %zu bytes", workspace_bytes, L.end);
    if (K == 0) return 0;
    hipStream_t s = as_stream(stream);
    const dim3 block(256), flat(flat_wgs(N, 8192));
    const auto count = [&] {
        if (N > 0) hipLaunchKernelGGL(cloud_count_kernel, flat, block, 0, s, point_label, (long long)N, K, counts);
    };
    const auto compact = [&](const int *offsets, int *cursor, int *lab, uint64_t *key) {
        if (N > 0)
            hipLaunchKernelGGL(cloud_compact_kernel, flat, block, 0, s, z, (long long)stride, point_label, (long long)N, K, offsets,
                               cursor, lab, key);
    };
    if (!segmed::launch(L, N, K, counts, medians, workspace, s, count, compact)) return check_launch("cloud_medians (clear)");
    note_kernel("select_pass_kernel");
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
