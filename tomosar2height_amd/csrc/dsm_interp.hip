// Interpolation baselines on the device (reference: scripts/interpolate_nearest.py, scripts/interpolate_idw.py; ABI in
// include/t2h_interp.h): exact k nearest neighbours of every node of a regular grid in a scattered float64 cloud.
//
// BOUNDS: min / max of X and Y and the count of rows with a non-finite value -- partial rows per workgroup, then one workgroup
//   that also derives the cell grid (edge h, gx x gy cells) on the device, so the index can be built before anything is
//   copied to the host.
//
// INDEX: counts per cell (integer atomics), exclusive scan to CSR offsets (three launches, as in dsm_instances.hip), the points
//   into their cells in arrival order, then every point's RANK inside its cell under (X, Y, -Z, slot) -- a count over the
//   cell's points, so the sorted image does not depend on arrival -- a flag on the first element of every run of equal
//   (X, Y), a scan of the flags, and the compaction: the unique cloud in cell-major order with its own cell offsets.
//   The rank pass is quadratic in a cell's population; h aims at T2H_INTERP_CELL_POINTS input points per cell.
//
// SEARCH: one workgroup per 16 x 16 tile of grid nodes, one node per thread.  B = the block of cells under the tile's nodes.
//   Ring 0 is B itself, ring r the cells at Chebyshev distance r around B, clipped to the grid; each cell belongs to exactly
//   one ring.  A ring's points are staged through LDS (16 B of coordinates + the index) in chunks of T2H_INTERP_CHUNK, and
//   every thread inserts what beats its k-th best (d2, X, Y) into a sorted list in registers.  After ring r a point not yet
//   seen lies at least r * h from every node of the tile, up to the rounding of the cell assignment (below 2^-34 relative
//   for any grid the index can build): the search stops when every thread's k-th d2 is strictly below (r * h * (1 - 2^-30))^2,
//   or when the rings have covered the grid.  Ties at equal d2 read the two (X, Y) from the unique cloud: rare, and total.
//
// Compare results and vector selects: like dsm_eval.hip and dsm_instances.hip this runs after the cloud
// is loaded, never beside a training step, so the rule for kernels that share a CU with the split convolutions does not bind.
#include <math.h>

#include "dsm_common.h"
#include "../../include/t2h_interp.h"

namespace t2h {

constexpr int kIpTile = T2H_INTERP_TILE;
constexpr int kIpChunk = T2H_INTERP_CHUNK;
constexpr int kIpMaxK = T2H_INTERP_MAX_K;
constexpr int kIpCols = T2H_INTERP_TABLE_COLS;
constexpr int kIpScanBlock = 1024;                                // items per workgroup of the scans (4 per thread)
constexpr int kIpPartials = 1024;                                 // workgroups of the bounds pass
constexpr int64_t kIpMaxPoints = 0x7fffffff;

// the cell of coordinate v along one axis: floor((v - vmin) / h), clamped to 0 .. g - 1 (v == vmax lands in the last cell).
// Monotone in v, and the same expression for points and for grid nodes.
__device__ inline int ip_cell(double v, double vmin, double h, int g) {
    const double t = (v - vmin) / h;
    if (!(t >= 0.0)) return 0;
    if (t >= (double)(g - 1)) return g - 1;
    return (int)t;
}

struct IpGrid { double xmin, ymin, h; int gx, gy; };
__device__ inline IpGrid ip_grid(const double *table) {
    IpGrid g;
    g.xmin = table[0]; g.ymin = table[2]; g.h = table[5]; g.gx = (int)table[6]; g.gy = (int)table[7];
    return g;
}
__device__ inline bool ip_finite3(double x, double y, double z) { return isfinite(x) && isfinite(y) && isfinite(z); }
__device__ inline int ip_cell_of(const IpGrid &g, double x, double y) {
    return ip_cell(y, g.ymin, g.h, g.gy) * g.gx + ip_cell(x, g.xmin, g.h, g.gx);
}

// ------------------------------------------------------------------------------------------ bounds
__device__ inline void ip_reduce5(double (*red)[5], int t) {
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) {
            red[t][0] = fmin(red[t][0], red[t + off][0]);
            red[t][1] = fmax(red[t][1], red[t + off][1]);
            red[t][2] = fmin(red[t][2], red[t + off][2]);
            red[t][3] = fmax(red[t][3], red[t + off][3]);
            red[t][4] += red[t + off][4];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void interp_bounds_partial_kernel(const double *__restrict__ pts, long long N,
                                                                    double *__restrict__ part) {
    __shared__ double red[256][5];
    const int t = threadIdx.x;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY, bad = 0.0;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + t; i < N; i += stride) {
        const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (ip_finite3(x, y, z)) { x0 = fmin(x0, x); x1 = fmax(x1, x); y0 = fmin(y0, y); y1 = fmax(y1, y); }
        else bad += 1.0;
    }
    red[t][0] = x0; red[t][1] = x1; red[t][2] = y0; red[t][3] = y1; red[t][4] = bad;
    __syncthreads();
    ip_reduce5(red, t);
    if (t < 5) part[blockIdx.x * 5 + t] = red[0][t];
}

// ONE workgroup: the partial rows in a fixed order, then the cell grid
__global__ __launch_bounds__(256) void interp_bounds_final_kernel(const double *__restrict__ part, int nb, long long N,
                                                                  double *__restrict__ table) {
    __shared__ double red[256][5];
    const int t = threadIdx.x;
    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY, bad = 0.0;
    for (int b = t; b < nb; b += 256) {
        x0 = fmin(x0, part[b * 5]); x1 = fmax(x1, part[b * 5 + 1]);
        y0 = fmin(y0, part[b * 5 + 2]); y1 = fmax(y1, part[b * 5 + 3]);
        bad += part[b * 5 + 4];
    }
    red[t][0] = x0; red[t][1] = x1; red[t][2] = y0; red[t][3] = y1; red[t][4] = bad;
    __syncthreads();
    ip_reduce5(red, t);
    if (t != 0) return;
    x0 = red[0][0]; x1 = red[0][1]; y0 = red[0][2]; y1 = red[0][3];
    double w = x1 - x0, hh = y1 - y0;
    if (!(w >= 0.0) || !isfinite(w)) w = 0.0;                     // no finite row at all, or an extent past the format
    if (!(hh >= 0.0) || !isfinite(hh)) hh = 0.0;
    const double n = (double)N, c = (double)T2H_INTERP_CELL_POINTS, cap = (double)(N / 2 + 8);
    double h = fmax(sqrt(c * w * hh / n), 2.0 * c * fmax(w, hh) / n);
    if (!(h > 0.0) || !isfinite(h)) h = 1.0;
    double gx = 1.0, gy = 1.0;
    bool ok = false;
    for (int it = 0; it < 2200 && !ok; ++it) {                    // (the first h fits by construction; rounding may ask for one doubling)
        gx = floor(w / h) + 1.0;
        gy = floor(hh / h) + 1.0;
        ok = gx * gy <= cap;
        if (!ok) h *= 2.0;
    }
    if (!ok || !isfinite(h)) { h = 1.0; gx = gy = 1.0; }
    table[0] = x0; table[1] = x1; table[2] = y0; table[3] = y1; table[4] = red[0][4];
    table[5] = h; table[6] = gx; table[7] = gy;
    for (int k = 8; k < kIpCols; ++k) table[k] = 0.0;
}

// ------------------------------------------------------------------------------------------ scans
__global__ __launch_bounds__(256) void interp_scan_sums_kernel(const int *__restrict__ in, long long n, int *__restrict__ bsum) {
    const long long base = (long long)blockIdx.x * kIpScanBlock + 4 * threadIdx.x;
    int s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (base + j < n) s += in[base + j];
    int total;
    block_scan(s, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// out[i] = in[0] + ... + in[i - 1]  (out may be in: a thread reads its four items before it writes them)
__global__ __launch_bounds__(256) void interp_scan_write_kernel(const int *in, long long n, const int *__restrict__ bsum, int *out) {
    const long long base = (long long)blockIdx.x * kIpScanBlock + 4 * threadIdx.x;
    int c[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = base + j < n ? in[base + j] : 0;
        s += c[j];
    }
    int total, run = block_scan(s, &total) + bsum[blockIdx.x];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j < n) out[base + j] = run;
        run += c[j];
    }
}

// ------------------------------------------------------------------------------------------ index
__global__ __launch_bounds__(256) void interp_count_kernel(const double *__restrict__ pts, long long N,
                                                           const double *__restrict__ table, int *__restrict__ cnt) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const IpGrid g = ip_grid(table);
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (ip_finite3(x, y, z)) atomicAdd(&cnt[ip_cell_of(g, x, y)], 1);
}

// the slot inside the cell depends on arrival (cnt counts down to 0); the rank pass below removes that
__global__ __launch_bounds__(256) void interp_fill_kernel(const double *__restrict__ pts, long long N,
                                                          const double *__restrict__ table, const int *__restrict__ off,
                                                          int *__restrict__ cnt, double *__restrict__ tmp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const IpGrid g = ip_grid(table);
    const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (!ip_finite3(x, y, z)) return;
    const int c = ip_cell_of(g, x, y);
    const long long slot = (long long)off[c] + (atomicSub(&cnt[c], 1) - 1);
    if (slot >= 0 && slot < N) {                                  // always, for counts taken from the same points
        tmp[3 * (size_t)slot] = x; tmp[3 * (size_t)slot + 1] = y; tmp[3 * (size_t)slot + 2] = z;
    }
}

// sorted[cell start + rank] = point, rank = the points of its cell before it under (X, Y, -Z, slot).  Points that are equal
// in all three values differ only by slot, and swapping them changes no byte.
__global__ __launch_bounds__(256) void interp_rank_kernel(const double *__restrict__ tmp, long long N, int cells_cap,
                                                          const double *__restrict__ table, const int *__restrict__ off,
                                                          double *__restrict__ sorted) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N || i >= off[cells_cap]) return;
    const IpGrid g = ip_grid(table);
    const double x = tmp[3 * (size_t)i], y = tmp[3 * (size_t)i + 1], z = tmp[3 * (size_t)i + 2];
    const int c = ip_cell_of(g, x, y), a = off[c], b = off[c + 1];
    int rank = 0;
    for (int j = a; j < b; ++j) {
        const double qx = tmp[3 * (size_t)j], qy = tmp[3 * (size_t)j + 1], qz = tmp[3 * (size_t)j + 2];
        const bool before = qx < x || (qx == x && (qy < y || (qy == y && (qz > z || (qz == z && j < i)))));
        rank += before;
    }
    const long long dst = (long long)a + rank;
    if (dst < N) { sorted[3 * (size_t)dst] = x; sorted[3 * (size_t)dst + 1] = y; sorted[3 * (size_t)dst + 2] = z; }
}

// flag[i] = 1 where sorted[i] opens a run of equal (X, Y) (equal pairs share a cell, and a cell is sorted), for i in [0, N]
__global__ __launch_bounds__(256) void interp_flag_kernel(const double *__restrict__ sorted, long long N, int cells_cap,
                                                          const double *__restrict__ table, const int *__restrict__ off,
                                                          int *__restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > N) return;
    int f = 0;
    if (i < N && i < off[cells_cap]) {
        const IpGrid g = ip_grid(table);
        const double x = sorted[3 * (size_t)i], y = sorted[3 * (size_t)i + 1];
        f = i == off[ip_cell_of(g, x, y)] || sorted[3 * (size_t)(i - 1)] != x || sorted[3 * (size_t)(i - 1) + 1] != y;
    }
    flag[i] = f;
}

__global__ __launch_bounds__(256) void interp_emit_kernel(const double *__restrict__ sorted, long long N,
                                                          const int *__restrict__ pos, double *__restrict__ unique) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int p = pos[i];
    if (pos[i + 1] == p || p < 0 || p >= N) return;
    unique[3 * (size_t)p] = sorted[3 * (size_t)i];
    unique[3 * (size_t)p + 1] = sorted[3 * (size_t)i + 1];
    unique[3 * (size_t)p + 2] = sorted[3 * (size_t)i + 2];
}

// cell offsets of the sorted image -> cell offsets of the unique cloud, in place (a thread reads and writes its own word)
__global__ __launch_bounds__(256) void interp_celloff_kernel(int *off, int cells_cap, long long N, const int *__restrict__ pos,
                                                             double *__restrict__ table) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c > cells_cap) return;
    const long long o = off[c];
    off[c] = pos[o < 0 ? 0 : o > N ? N : o];
    if (c == 0) table[8] = (double)pos[N];
}

// ------------------------------------------------------------------------------------------ search
enum { kIpKnn = 0, kIpNearest = 1, kIpIdw = 2 };

// (x, y) before the (X, Y) of unique row `other`; an empty slot comes after everything
__device__ inline bool ip_xy_before(const double *__restrict__ U, double x, double y, int other) {
    if (other < 0) return true;
    const double ox = U[3 * (size_t)other], oy = U[3 * (size_t)other + 1];
    return x < ox || (x == ox && y < oy);
}

template <int K, int MODE>
__global__ __launch_bounds__(256) void interp_search_kernel(const double *__restrict__ U, const int *__restrict__ off, int M,
                                                            double xmin, double ymin, double h, int gx, int gy, double res,
                                                            int ny, int nx, int tiles_x, double *__restrict__ out_d,
                                                            int *__restrict__ out_i) {
    __shared__ double2 sxy[kIpChunk];
    __shared__ int sid[kIpChunk];
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int i0 = tile_x * kIpTile, j0 = tile_y * kIpTile;
    const int i = i0 + (threadIdx.x & (kIpTile - 1)), j = j0 + (threadIdx.x / kIpTile);
    const bool valid = i < nx && j < ny;
    const double px = __dadd_rn(__dmul_rn((double)i, res), xmin), py = __dadd_rn(__dmul_rn((double)j, res), ymin);
    const int il = min(i0 + kIpTile, nx) - 1, jl = min(j0 + kIpTile, ny) - 1;
    // the block of cells under the tile's nodes (the node -> cell map is monotone, so the corners bound it)
    const int cx0 = ip_cell(__dadd_rn(__dmul_rn((double)i0, res), xmin), xmin, h, gx);
    const int cx1 = ip_cell(__dadd_rn(__dmul_rn((double)il, res), xmin), xmin, h, gx);
    const int cy0 = ip_cell(__dadd_rn(__dmul_rn((double)j0, res), ymin), ymin, h, gy);
    const int cy1 = ip_cell(__dadd_rn(__dmul_rn((double)jl, res), ymin), ymin, h, gy);

    double bd[K];
    int bi[K];
#pragma unroll
    for (int m = 0; m < K; ++m) { bd[m] = INFINITY; bi[m] = -1; }

    auto scan = [&](int fill) {
        if (!valid) return;
        for (int t = 0; t < fill; ++t) {
            const double2 q = sxy[t];                             // (every lane reads the same address: a broadcast)
            const double dx = q.x - px, dy = q.y - py;
            const double d2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
            if (!(d2 <= bd[K - 1])) continue;
            const int id = sid[t];
            bool lt[K];
#pragma unroll
            for (int m = 0; m < K; ++m) lt[m] = d2 < bd[m] || (d2 == bd[m] && ip_xy_before(U, q.x, q.y, bi[m]));
#pragma unroll
            for (int m = K - 1; m >= 1; --m) {
                if (lt[m - 1]) { bd[m] = bd[m - 1]; bi[m] = bi[m - 1]; }
                else if (lt[m]) { bd[m] = d2; bi[m] = id; }
            }
            if (lt[0]) { bd[0] = d2; bi[0] = id; }
        }
    };

    for (int r = 0;; ++r) {
        const int ax0 = cx0 - r, ax1 = cx1 + r, ay0 = cy0 - r, ay1 = cy1 + r;
        int fill = 0;
        for (int cy = max(ay0, 0); cy <= min(ay1, gy - 1); ++cy) {
            const bool full = r == 0 || cy == ay0 || cy == ay1;   // a whole row of the ring's box, or its two end cells
            for (int s = 0; s < (full ? 1 : 2); ++s) {
                int ca, cb;
                if (full) { ca = max(ax0, 0); cb = min(ax1, gx - 1); }
                else if (s == 0) { if (ax0 < 0) continue; ca = cb = ax0; }
                else { if (ax1 >= gx) continue; ca = cb = ax1; }
                // cells ca .. cb of one row are neighbours in the CSR order: one range of the unique cloud
                int a = __builtin_amdgcn_readfirstlane(off[cy * gx + ca]);
                int b = __builtin_amdgcn_readfirstlane(off[cy * gx + cb + 1]);
                a = max(a, 0);
                b = min(b, M);
                while (a < b) {
                    const int n = min(b - a, kIpChunk - fill);
                    for (int t = threadIdx.x; t < n; t += 256) {
                        sxy[fill + t] = make_double2(U[3 * (size_t)(a + t)], U[3 * (size_t)(a + t) + 1]);
                        sid[fill + t] = a + t;
                    }
                    fill += n;
                    a += n;
                    if (fill == kIpChunk) {
                        __syncthreads();
                        scan(fill);
                        __syncthreads();
                        fill = 0;
                    }
                }
            }
        }
        if (fill) {
            __syncthreads();
            scan(fill);
            __syncthreads();
        }
        if (ax0 <= 0 && ay0 <= 0 && ax1 >= gx - 1 && ay1 >= gy - 1) break;      // every cell has been searched
        const double lim = (double)r * h * (1.0 - 0x1p-30);
        if (__syncthreads_and(!valid || bd[K - 1] < lim * lim)) break;
    }

    if (!valid) return;
    const size_t pix = (size_t)j * nx + i;
    if (MODE == kIpKnn) {
#pragma unroll
        for (int m = 0; m < K; ++m) { out_d[pix * K + m] = bd[m]; out_i[pix * K + m] = bi[m]; }
    } else if (MODE == kIpNearest) {
        out_d[pix] = bi[0] >= 0 ? U[3 * (size_t)bi[0] + 2] : NAN;
    } else {
        double w[K], s = 0.0;
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const double dist = sqrt(bd[m]);
            w[m] = dist == 0.0 ? 1.0 : 1.0 / __dmul_rn(dist, dist);
            s = m == 0 ? w[0] : __dadd_rn(s, w[m]);
        }
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m < K; ++m) {
            const double z = bi[m] >= 0 ? U[3 * (size_t)bi[m] + 2] : NAN;
            const double term = __dmul_rn(w[m] / s, z);
            acc = m == 0 ? term : __dadd_rn(acc, term);
        }
        out_d[pix] = acc;
    }
}

// ------------------------------------------------------------------------------------------ host side
static int64_t ip_cells_cap(int64_t N) { return N / 2 + 8; }
static unsigned ip_wgs(int64_t n) { return (unsigned)((n + 255) / 256); }

struct IpIndexLayout {                                            // byte offsets into the workspace
    size_t cnt, bsum, tmp, sorted, pos, end;
    explicit IpIndexLayout(int64_t N) {
        const size_t n = (size_t)N, cap = (size_t)ip_cells_cap(N);
        const size_t items = (n + 1 > cap + 1 ? n + 1 : cap + 1), nb = (items + kIpScanBlock - 1) / kIpScanBlock;
        cnt = 0;
        bsum = cnt + up256(4 * (cap + 1));
        tmp = bsum + up256(4 * nb);
        sorted = tmp + up256(24 * n);
        pos = sorted + up256(24 * n);
        end = pos + up256(4 * (n + 1));
    }
};

static void ip_scan(const int *in, int64_t n, int *bsum, int *out, hipStream_t s) {
    const int nb = (int)((n + kIpScanBlock - 1) / kIpScanBlock);
    hipLaunchKernelGGL(interp_scan_sums_kernel, dim3(nb), dim3(256), 0, s, in, (long long)n, bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, (int *)nullptr, nb, (int *)nullptr);
    hipLaunchKernelGGL(interp_scan_write_kernel, dim3(nb), dim3(256), 0, s, in, (long long)n, (const int *)bsum, out);
}

static int ip_check_grid(const char *what, const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin,
                         double h, int gx, int gy, double res, int ny, int nx, int k, const void *out) {
    if (!unique || !cell_offsets || !out) return fail(T2H_ERR_ARG, "%s: null pointer", what);
    if (((uintptr_t)unique & 7) || ((uintptr_t)cell_offsets & 3) || ((uintptr_t)out & 7))
        return fail(T2H_ERR_ARG, "%s: misaligned pointer", what);
    if (M < 1) return fail(T2H_ERR_ARG, "%s: M = %d unique points", what, M);
    if (k < 1 || k > kIpMaxK || k > M) return fail(T2H_ERR_ARG, "%s: k = %d (1 .. min(M = %d, %d))", what, k, M, kIpMaxK);
    if (!isfinite(xmin) || !isfinite(ymin) || !(h > 0.0) || !isfinite(h) || !(res > 0.0) || !isfinite(res))
        return fail(T2H_ERR_ARG, "%s: origin (%g, %g), cell edge %g and resolution %g must be finite, the last two positive", what,
                    xmin, ymin, h, res);
    if (gx < 1 || gy < 1 || (int64_t)gx * gy > kIpMaxPoints / 2 + 8)
        return fail(T2H_ERR_ARG, "%s: bad cell grid %d x %d", what, gx, gy);
    if (ny < 1 || nx < 1 || (int64_t)ny * nx > kIpMaxPoints)
        return fail(T2H_ERR_ARG, "%s: bad raster %d x %d (1 .. 2^31 - 1 nodes)", what, ny, nx);
    return 0;
}

template <int MODE>
static void ip_launch(int k, dim3 grid, hipStream_t s, const double *U, const int *off, int M, double xmin, double ymin, double h,
                      int gx, int gy, double res, int ny, int nx, int tiles_x, double *out_d, int *out_i) {
#define T2H_IP_CASE(K)                                                                                                        \
    case K:                                                                                                                   \
        hipLaunchKernelGGL((interp_search_kernel<K, MODE>), grid, dim3(256), 0, s, U, off, M, xmin, ymin, h, gx, gy, res, ny,  \
                           nx, tiles_x, out_d, out_i);                                                                        \
        break;
    switch (k) {
        T2H_IP_CASE(1) T2H_IP_CASE(2) T2H_IP_CASE(3) T2H_IP_CASE(4) T2H_IP_CASE(5) T2H_IP_CASE(6) T2H_IP_CASE(7) T2H_IP_CASE(8)
    }
#undef T2H_IP_CASE
}

static int ip_search(int mode, const char *what, const double *unique, const int32_t *cell_offsets, int M, double xmin,
                     double ymin, double h, int gx, int gy, double res, int ny, int nx, int k, double *out_d, int32_t *out_i,
                     t2h_stream_t stream) {
    const int rc = ip_check_grid(what, unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, k, out_d);
    if (rc) return rc;
    const int tiles_x = (nx + kIpTile - 1) / kIpTile, tiles_y = (ny + kIpTile - 1) / kIpTile;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y));
    hipStream_t s = as_stream(stream);
    if (mode == kIpKnn) ip_launch<kIpKnn>(k, grid, s, unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, tiles_x, out_d, out_i);
    else if (mode == kIpNearest)
        hipLaunchKernelGGL((interp_search_kernel<1, kIpNearest>), grid, dim3(256), 0, s, unique, cell_offsets, M, xmin, ymin, h,
                           gx, gy, res, ny, nx, tiles_x, out_d, (int *)nullptr);
    else ip_launch<kIpIdw>(k, grid, s, unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, tiles_x, out_d, (int *)nullptr);
    note_kernel("interp_search_kernel");
    return check_launch(what);
}

}  // namespace t2h

using namespace t2h;

T2H_API int64_t t2h_interp_max_cells(int64_t N) { return N < 1 || N > kIpMaxPoints ? 0 : ip_cells_cap(N); }

T2H_API size_t t2h_interp_bounds_workspace_bytes(int64_t N) {
    return N < 1 || N > kIpMaxPoints ? 0 : (size_t)kIpPartials * 5 * sizeof(double);
}

T2H_API int t2h_interp_bounds(const double *points, int64_t N, double *table, void *workspace, size_t workspace_bytes,
                              t2h_stream_t stream) {
    if (!points || !table || !workspace) return fail(T2H_ERR_ARG, "interp_bounds: null pointer");
    if (N < 1 || N > kIpMaxPoints) return fail(T2H_ERR_ARG, "interp_bounds: N = %lld points (1 .. 2^31 - 1)", (long long)N);
    if (((uintptr_t)points & 7) || ((uintptr_t)table & 7) || ((uintptr_t)workspace & 7))
        return fail(T2H_ERR_ARG, "interp_bounds: points / table / workspace must be 8-byte aligned");
    const size_t need = t2h_interp_bounds_workspace_bytes(N);
    if (workspace_bytes < need) return fail(T2H_ERR_WORKSPACE, "interp_bounds: workspace %zu < %zu bytes", workspace_bytes, need);
    hipStream_t s = as_stream(stream);
    const int nb = (int)((N + 255) / 256 < kIpPartials ? (N + 255) / 256 : kIpPartials);
    double *part = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(interp_bounds_partial_kernel, dim3(nb), dim3(256), 0, s, points, (long long)N, part);
    hipLaunchKernelGGL(interp_bounds_final_kernel, dim3(1), dim3(256), 0, s, (const double *)part, nb, (long long)N, table);
    note_kernel("interp_bounds_partial_kernel");
    return check_launch("interp_bounds");
}

T2H_API size_t t2h_interp_index_workspace_bytes(int64_t N) {
    if (N < 1 || N > kIpMaxPoints) return 0;
    return IpIndexLayout(N).end;
}

T2H_API int t2h_interp_index(const double *points, int64_t N, double *table, double *unique, int32_t *cell_offsets,
                             void *workspace, size_t workspace_bytes, t2h_stream_t stream) {
    if (!points || !table || !unique || !cell_offsets || !workspace) return fail(T2H_ERR_ARG, "interp_index: null pointer");
    if (N < 1 || N > kIpMaxPoints) return fail(T2H_ERR_ARG, "interp_index: N = %lld points (1 .. 2^31 - 1)", (long long)N);
    if (((uintptr_t)points & 7) || ((uintptr_t)table & 7) || ((uintptr_t)unique & 7) || ((uintptr_t)cell_offsets & 3) ||
        ((uintptr_t)workspace & 7))
        return fail(T2H_ERR_ARG, "interp_index: misaligned pointer (float64 arrays: 8 bytes, cell_offsets: 4)");
    const IpIndexLayout L(N);
    if (workspace_bytes < L.end) return fail(T2H_ERR_WORKSPACE, "interp_index: workspace %zu < %zu bytes", workspace_bytes, L.end);
    hipStream_t s = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    int *cnt = reinterpret_cast<int *>(ws + L.cnt), *bsum = reinterpret_cast<int *>(ws + L.bsum);
    int *pos = reinterpret_cast<int *>(ws + L.pos);
    double *tmp = reinterpret_cast<double *>(ws + L.tmp), *sorted = reinterpret_cast<double *>(ws + L.sorted);
    const int cap = (int)ip_cells_cap(N);
    if (hipMemsetAsync(cnt, 0, 4 * ((size_t)cap + 1), s) != hipSuccess) return check_launch("interp_index (clear)");
    const dim3 block(256), per_point(ip_wgs(N)), per_point1(ip_wgs(N + 1));
    hipLaunchKernelGGL(interp_count_kernel, per_point, block, 0, s, points, (long long)N, (const double *)table, cnt);
    ip_scan(cnt, (int64_t)cap + 1, bsum, cell_offsets, s);
    hipLaunchKernelGGL(interp_fill_kernel, per_point, block, 0, s, points, (long long)N, (const double *)table,
                       (const int *)cell_offsets, cnt, tmp);
    hipLaunchKernelGGL(interp_rank_kernel, per_point, block, 0, s, (const double *)tmp, (long long)N, cap, (const double *)table,
                       (const int *)cell_offsets, sorted);
    hipLaunchKernelGGL(interp_flag_kernel, per_point1, block, 0, s, (const double *)sorted, (long long)N, cap,
                       (const double *)table, (const int *)cell_offsets, pos);
    ip_scan(pos, N + 1, bsum, pos, s);
    hipLaunchKernelGGL(interp_emit_kernel, per_point, block, 0, s, (const double *)sorted, (long long)N, (const int *)pos, unique);
    hipLaunchKernelGGL(interp_celloff_kernel, dim3(ip_wgs((int64_t)cap + 1)), block, 0, s, cell_offsets, cap, (long long)N,
                       (const int *)pos, table);
    note_kernel("interp_rank_kernel");
    return check_launch("interp_index");
}

T2H_API int t2h_interp_knn(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                           int gy, double res, int ny, int nx, int k, double *d2, int32_t *idx, t2h_stream_t stream) {
    if (!idx || ((uintptr_t)idx & 3)) return fail(T2H_ERR_ARG, "interp_knn: idx is null or misaligned");
    return ip_search(kIpKnn, "interp_knn", unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, k, d2, idx, stream);
}

T2H_API int t2h_interp_nearest(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h,
                               int gx, int gy, double res, int ny, int nx, double *out, t2h_stream_t stream) {
    return ip_search(kIpNearest, "interp_nearest", unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, 1, out, nullptr,
                     stream);
}

T2H_API int t2h_interp_idw(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                           int gy, double res, int ny, int nx, int k, double *out, t2h_stream_t stream) {
    return ip_search(kIpIdw, "interp_idw", unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, k, out, nullptr, stream);
}
