// Small helpers shared by the device-side DSM evaluators (dsm_*.hip): the workgroup scan, the one-workgroup top-level scan, the
// order-preserving 64-bit image of a float64, and the host-side rounding of workspace parts and flat grids.
#pragma once
#include "t2h_common.h"

namespace t2h {

typedef unsigned long long u64;

constexpr int kScanBlock = 1024;                                  // items per workgroup of the scans (4 per thread)

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

// one workgroup: a[0 .. nb) (and b, if given) to their exclusive prefixes in place; the totals to total[0] (and total[1]),
// if total is given.  (static: every source that includes this header gets a kernel of its own, as it had before)
static __global__ __launch_bounds__(256) void scan_top_kernel(int *__restrict__ a, int *__restrict__ b, int nb,
                                                              int *__restrict__ total) {
    const int per = (nb + 255) / 256, lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    for (int s = 0; s < 2; ++s) {
        int *v = s ? b : a;
        if (!v) break;
        int sum = 0;
        for (int i = lo; i < hi; ++i) sum += v[i];
        int tot, run = block_scan(sum, &tot);
        for (int i = lo; i < hi; ++i) { int t = v[i]; v[i] = run; run += t; }
        if (total && threadIdx.x == 0) total[s] = tot;
    }
}

__device__ inline u64 key64(double v) {                           // order-preserving image: a < b  <=>  key(a) < key(b)
    u64 b = (u64)__double_as_longlong(v);
    return b ^ ((u64)((long long)b >> 63) | 0x8000000000000000ull);
}
__device__ inline double value64(u64 k) {
    return __longlong_as_double((long long)(k ^ ((u64)((long long)~k >> 63) | 0x8000000000000000ull)));
}

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
inline int flat_wgs(int64_t n, int cap) {
    int64_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

}  // namespace t2h
