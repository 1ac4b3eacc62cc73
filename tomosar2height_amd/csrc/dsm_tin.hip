// Delaunay-linear baseline on the device (reference: scripts/interpolate_bilinear.py; ABI in include/t2h_tin.h; predicates and
// per-node state in tin_core.h).  No triangulation is built.  A raster node needs only the one Delaunay
// triangle that contains it, and that triangle is the optimal basis of a three-variable linear program over the cloud:
// minimise sum lambda_i |p_i|^2 subject to sum lambda_i p_i = q, sum lambda_i = 1, lambda >= 0.  A basis is a triangle that
// contains q; a variable may enter where its point lies strictly inside the triangle's circumcircle; the vertex that leaves
// is the one whose replacement keeps q inside.  The lifted value at q falls with every pivot.
//
// HULL: which nodes have a triangle at all is decided here and nowhere else (outside the hull the program is infeasible, and
//   proving that by search would visit the whole cloud).  Extremes along T2H_TIN_DIRECTIONS directions (partial rows per
//   workgroup, ties to the smaller row, so the result does not depend on scheduling), made a strictly convex polygon by one
//   thread; every point not strictly inside it -- beyond the orientation's error bound, so a point is only ever discarded
//   when it cannot be a hull vertex -- is appended to a list (integer atomic: arrival order); ONE workgroup sorts the list by
//   (X, Y) (bitonic, in global memory: the list is short for any cloud with a few straight sides, and its length is only
//   bounded by M) and one thread runs Andrew's monotone chain on it.
//
// SEARCH: one workgroup per 16 x 16 tile of nodes, one node per thread, the ring walk and LDS staging of dsm_interp.hip (ring
//   0 = the cells under the tile, ring r the cells at Chebyshev distance r).  A node first collects a wedge of directions until
//   three offered points surround it (tin_wedge), then pivots on every offered point that lies inside its circumcircle.  The
//   walk of a tile ends when, for every node, each point inside its circumcircle has been offered ((2 R)^2 below the squared
//   distance of the nearest cell not yet staged) or the rings have covered the grid.  That alone proves nothing -- a point
//   offered before the last pivot was tested against another triangle -- so every node then VERIFIES: it scans the cells under
//   its circumcircle's box straight from global memory, pivots on the most violating point (largest determinant, ties to the
//   smaller (X, Y)) and repeats until no point is strictly inside, at most T2H_TIN_MAX_PIVOTS times.
//
// Compare results and vector selects: like dsm_interp.hip this runs after the cloud is loaded, never
// beside a training step, so the rule for kernels that share a CU with the split convolutions does not bind.
#include <math.h>

#include "dsm_common.h"
#include "tin_core.h"
#include "../../include/t2h_tin.h"

namespace t2h {

constexpr int kTinTile = T2H_INTERP_TILE;
constexpr int kTinChunk = T2H_INTERP_CHUNK;
constexpr int kTinDirs = T2H_TIN_DIRECTIONS;
constexpr int kTinCols = T2H_TIN_STATUS_COLS;
constexpr int kTinPartials = 256;                                // workgroups of the extremes pass
constexpr int kTinMaxPoints = 0x7fffffff;

// the same cell map as dsm_interp.hip's, on a coordinate that is already shifted: floor(s / h) clamped to 0 .. g - 1
__device__ inline int tin_cell(double s, double h, int g) {
    const double t = s / h;
    if (!(t >= 0.0)) return 0;
    if (t >= (double)(g - 1)) return g - 1;
    return (int)t;
}

// ------------------------------------------------------------------------------------------ hull
__device__ inline bool tin_better(double v, int i, double w, int k) { return v > w || (v == w && i < k); }

__global__ __launch_bounds__(256) void tin_extremes_partial_kernel(const double *__restrict__ U, int M, double xmin, double ymin,
                                                                   double *__restrict__ part_v, int *__restrict__ part_i) {
    __shared__ double rv[256];
    __shared__ int ri[256];
    const int t = threadIdx.x;
    double dx[kTinDirs], dy[kTinDirs], bv[kTinDirs];
    int bi[kTinDirs];
#pragma unroll
    for (int k = 0; k < kTinDirs; ++k) {
        dx[k] = cospi(2.0 * k / kTinDirs); dy[k] = sinpi(2.0 * k / kTinDirs);
        bv[k] = -INFINITY; bi[k] = kTinMaxPoints;
    }
    for (long long i = (long long)blockIdx.x * 256 + t; i < M; i += (long long)gridDim.x * 256) {
        const double x = U[3 * (size_t)i] - xmin, y = U[3 * (size_t)i + 1] - ymin;
#pragma unroll
        for (int k = 0; k < kTinDirs; ++k) {
            const double v = dx[k] * x + dy[k] * y;
            if (tin_better(v, (int)i, bv[k], bi[k])) { bv[k] = v; bi[k] = (int)i; }
        }
    }
#pragma unroll
    for (int k = 0; k < kTinDirs; ++k) {
        rv[t] = bv[k]; ri[t] = bi[k];
        __syncthreads();
        for (int off = 128; off >= 1; off >>= 1) {
            if (t < off && tin_better(rv[t + off], ri[t + off], rv[t], ri[t])) { rv[t] = rv[t + off]; ri[t] = ri[t + off]; }
            __syncthreads();
        }
        if (t == 0) { part_v[blockIdx.x * kTinDirs + k] = rv[0]; part_i[blockIdx.x * kTinDirs + k] = ri[0]; }
        __syncthreads();
    }
}

// ONE workgroup: the partial rows, then (one thread) the polygon: the extremes in the order of their directions, which is
// counter-clockwise, repeated ones dropped, and every vertex that does not turn left beyond the error bound popped.
// poly[0] = its vertex count (0 where fewer than 3 remain: nothing is filtered), poly[1 + 2 v], poly[2 + 2 v] = shifted (x, y).
__global__ __launch_bounds__(256) void tin_extremes_final_kernel(const double *__restrict__ U, double xmin, double ymin,
                                                                 const double *__restrict__ part_v, const int *__restrict__ part_i,
                                                                 int nb, double *__restrict__ poly, int *__restrict__ counter) {
    __shared__ int win[kTinDirs];
    const int t = threadIdx.x;
    if (t < kTinDirs) {
        double v = -INFINITY;
        int idx = kTinMaxPoints;
        for (int b = 0; b < nb; ++b)
            if (tin_better(part_v[b * kTinDirs + t], part_i[b * kTinDirs + t], v, idx)) { v = part_v[b * kTinDirs + t]; idx = part_i[b * kTinDirs + t]; }
        win[t] = idx;
    }
    __syncthreads();
    if (t != 0) return;
    *counter = 0;
    double px[kTinDirs], py[kTinDirs];
    int n = 0;
    auto turn = [&](int a, int b, double x, double y) {          // b turns left between a and (x, y), beyond the bound
        const double l = (px[b] - px[a]) * (y - py[a]), r = (py[b] - py[a]) * (x - px[a]);
        return l - r > kTinCcwErr * (fabs(l) + fabs(r));
    };
    int last = -1;
    for (int k = 0; k < kTinDirs; ++k) {
        const int idx = win[k];
        if (idx == last || idx == kTinMaxPoints || (n > 0 && idx == win[0] && k > 0)) continue;
        last = idx;
        const double x = U[3 * (size_t)idx] - xmin, y = U[3 * (size_t)idx + 1] - ymin;
        while (n >= 2 && !turn(n - 2, n - 1, x, y)) --n;
        px[n] = x; py[n] = y; ++n;
    }
    while (n >= 3 && !turn(n - 2, n - 1, px[0], py[0])) --n;
    while (n >= 3 && !turn(n - 1, 0, px[1], py[1])) {            // the first vertex itself
        for (int v = 0; v + 1 < n; ++v) { px[v] = px[v + 1]; py[v] = py[v + 1]; }
        --n;
    }
    for (int v = 0; v < n && n >= 3; ++v)                         // every corner once more; a polygon that is not convex filters nothing
        if (!turn(v, (v + 1) % n, px[(v + 2) % n], py[(v + 2) % n])) n = 0;
    if (n < 3) n = 0;
    poly[0] = (double)n;
    for (int v = 0; v < n; ++v) { poly[1 + 2 * v] = px[v]; poly[2 + 2 * v] = py[v]; }
}

__global__ __launch_bounds__(256) void tin_filter_kernel(const double *__restrict__ U, int M, double xmin, double ymin,
                                                         const double *__restrict__ poly, int *__restrict__ counter,
                                                         int *__restrict__ surv) {
    __shared__ double sp[1 + 2 * kTinDirs];
    if (threadIdx.x < 1 + 2 * kTinDirs) sp[threadIdx.x] = poly[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const int n = (int)sp[0];
    const double x = U[3 * (size_t)i] - xmin, y = U[3 * (size_t)i + 1] - ymin;
    bool inside = n >= 3;
    for (int v = 0; v < n && inside; ++v) {
        const int w = v + 1 == n ? 0 : v + 1;
        const double ax = sp[1 + 2 * v], ay = sp[2 + 2 * v];
        const double l = (sp[1 + 2 * w] - ax) * (y - ay), r = (sp[2 + 2 * w] - ay) * (x - ax);
        inside = l - r > kTinCcwErr * (fabs(l) + fabs(r));
    }
    if (inside) return;
    const int pos = atomicAdd(counter, 1);
    if (pos >= 0 && pos < M) surv[pos] = (int)i;
}

// (X, Y) of row a before that of row b; -1 (padding) comes after everything
__device__ inline bool tin_row_before(const double *__restrict__ U, int a, int b) {
    if (a < 0) return false;
    if (b < 0) return true;
    const double ax = U[3 * (size_t)a], bx = U[3 * (size_t)b];
    return ax < bx || (ax == bx && U[3 * (size_t)a + 1] < U[3 * (size_t)b + 1]);
}

// ONE workgroup: sort the survivors, then the monotone chain (one thread).  surv holds `cap` (a power of two >= M) words.
__global__ __launch_bounds__(256) void tin_chain_kernel(const double *__restrict__ U, int M, double xmin, double ymin,
                                                        const int *__restrict__ counter, int *surv, int cap,
                                                        int *__restrict__ hull, int *__restrict__ status) {
    const int t = threadIdx.x;
    int S = *counter;
    S = S < 0 ? 0 : S > M ? M : S;
    int P = 1;
    while (P < S) P <<= 1;
    if (P > cap) P = cap;                                        // (never: cap >= M >= S)
    for (int i = S + t; i < P; i += 256) surv[i] = -1;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = t; i < P; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const int a = surv[i], b = surv[l];
                    const bool up = (i & k) == 0;
                    if (up ? tin_row_before(U, b, a) : tin_row_before(U, a, b)) { surv[i] = b; surv[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    if (t != 0) return;
    auto X = [&](int row) { return U[3 * (size_t)row] - xmin; };
    auto Y = [&](int row) { return U[3 * (size_t)row + 1] - ymin; };
    int n = 0;
    if (S >= 3) {
        for (int pass = 0; pass < 2; ++pass) {                   // lower chain left to right, upper chain back
            const int floor_n = pass == 0 ? 1 : n;             // the upper chain never pops into the lower one
            for (int s = pass == 0 ? 0 : S - 2; pass == 0 ? s < S : s >= 0; s += pass == 0 ? 1 : -1) {
                const int row = surv[s];
                const double x = X(row), y = Y(row);
                while (n > floor_n && tin_cross(X(hull[n - 2]), Y(hull[n - 2]), X(hull[n - 1]), Y(hull[n - 1]), x, y) <= 0.0) --n;
                if (n <= M) hull[n++] = row;
            }
        }
        --n;                                                     // the first vertex closes the upper chain again
    }
    const bool degenerate = n < 3;
    for (int k = 0; k < kTinCols; ++k) status[k] = 0;
    status[T2H_TIN_HULL_COUNT] = degenerate ? 0 : n;
    status[T2H_TIN_HULL_DEGENERATE] = degenerate ? 1 : 0;
    status[T2H_TIN_HULL_SURVIVORS] = S;
}

// ------------------------------------------------------------------------------------------ search
enum { kTinSimplex = 0, kTinLinear = 1 };

template <int MODE>
__global__ __launch_bounds__(256) void tin_search_kernel(const double *__restrict__ U, const int *__restrict__ off, int M,
                                                         double xmin, double ymin, double h, int gx, int gy, double res, int ny,
                                                         int nx, int tiles_x, const int *__restrict__ hull, int nh,
                                                         int *__restrict__ tri, double *__restrict__ out, int *__restrict__ status) {
    __shared__ double2 sxy[kTinChunk];
    __shared__ int sid[kTinChunk];
    const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    const int i0 = tile_x * kTinTile, j0 = tile_y * kTinTile;
    const int i = i0 + (threadIdx.x & (kTinTile - 1)), j = j0 + (threadIdx.x / kTinTile);
    const bool valid = i < nx && j < ny;
    auto node = [&](int n, double vmin) { return __dadd_rn(__dmul_rn((double)n, res), vmin) - vmin; };     // shifted
    const int il = min(i0 + kTinTile, nx) - 1, jl = min(j0 + kTinTile, ny) - 1;
    const int cx0 = tin_cell(node(i0, xmin), h, gx), cx1 = tin_cell(node(il, xmin), h, gx);
    const int cy0 = tin_cell(node(j0, ymin), h, gy), cy1 = tin_cell(node(jl, ymin), h, gy);

    TinNode s;
    tin_node_init(s, node(i, xmin), node(j, ymin));

    // inside the hull: its vertices through LDS, kTinChunk - 1 edges at a time (the last staged vertex closes the chunk)
    bool act = valid;
    for (int base = 0; base < nh; base += kTinChunk - 1) {
        const int n = min(nh - base, kTinChunk - 1);
        for (int t = threadIdx.x; t <= n; t += 256) {
            const int row = hull[base + t == nh ? 0 : base + t];
            sxy[t] = make_double2(U[3 * (size_t)row] - xmin, U[3 * (size_t)row + 1] - ymin);
        }
        __syncthreads();
        if (act)
            for (int t = 0; t < n; ++t) {
                const double2 a = sxy[t], b = sxy[t + 1];
                if (tin_cross(a.x, a.y, b.x, b.y, s.qx, s.qy) < 0.0) { act = false; break; }
            }
        __syncthreads();
    }

    int walk_pivots = 0;
    auto offer = [&](int fill) {
        if (!act) return;
        for (int t = 0; t < fill; ++t) {
            const double2 p = sxy[t];                            // (every lane reads the same address: a broadcast)
            walk_pivots += tin_offer(s, p.x, p.y, sid[t]);
        }
    };

    for (int r = 0;; ++r) {
        const int ax0 = cx0 - r, ax1 = cx1 + r, ay0 = cy0 - r, ay1 = cy1 + r;
        int fill = 0;
        for (int cy = max(ay0, 0); cy <= min(ay1, gy - 1); ++cy) {
            const bool full = r == 0 || cy == ay0 || cy == ay1;   // a whole row of the ring's box, or its two end cells
            for (int e = 0; e < (full ? 1 : 2); ++e) {
                int ca, cb;
                if (full) { ca = max(ax0, 0); cb = min(ax1, gx - 1); }
                else if (e == 0) { if (ax0 < 0) continue; ca = cb = ax0; }
                else { if (ax1 >= gx) continue; ca = cb = ax1; }
                int a = __builtin_amdgcn_readfirstlane(off[cy * gx + ca]);
                int b = __builtin_amdgcn_readfirstlane(off[cy * gx + cb + 1]);
                a = max(a, 0);
                b = min(b, M);
                while (a < b) {
                    const int n = min(b - a, kTinChunk - fill);
                    for (int t = threadIdx.x; t < n; t += 256) {
                        sxy[fill + t] = make_double2(U[3 * (size_t)(a + t)] - xmin, U[3 * (size_t)(a + t) + 1] - ymin);
                        sid[fill + t] = a + t;
                    }
                    fill += n;
                    a += n;
                    if (fill == kTinChunk) {
                        __syncthreads();
                        offer(fill);
                        __syncthreads();
                        fill = 0;
                    }
                }
            }
        }
        if (fill) {
            __syncthreads();
            offer(fill);
            __syncthreads();
        }
        if (ax0 <= 0 && ay0 <= 0 && ax1 >= gx - 1 && ay1 >= gy - 1) break;      // every cell has been offered
        const double lim = (double)r * h * (1.0 - 0x1p-30);
        if (__syncthreads_and(!act || (s.have && tin_diameter2(s) < lim * lim))) break;
    }

    if (!valid) return;
    const size_t pix = (size_t)j * nx + i;
    bool capped = false;
    int pivots = 0;
    if (act && s.have) {
        for (;;) {
            double x0, x1, y0, y1;
            int ca = 0, cb = gx - 1, ra = 0, rb = gy - 1;
            if (tin_circle_box(s, &x0, &x1, &y0, &y1)) {
                ca = tin_cell(x0, h, gx); cb = tin_cell(x1, h, gx); ra = tin_cell(y0, h, gy); rb = tin_cell(y1, h, gy);
            }
            double best = 0.0, bx = 0.0, by = 0.0;
            int bid = -1;
            for (int cy = ra; cy <= rb; ++cy) {
                const int a = max(off[cy * gx + ca], 0), b = min(off[cy * gx + cb + 1], M);
                for (int t = a; t < b; ++t) {
                    if (t == s.ia || t == s.ib || t == s.ic) continue;
                    const double px = U[3 * (size_t)t] - xmin, py = U[3 * (size_t)t + 1] - ymin;
                    double det;
                    if (!tin_incircle(s.ax, s.ay, s.bx, s.by, s.cx, s.cy, px, py, &det)) continue;
                    if (bid < 0 || det > best || (det == best && (px < bx || (px == bx && py < by)))) { best = det; bx = px; by = py; bid = t; }
                }
            }
            if (bid < 0) break;
            if (pivots == T2H_TIN_MAX_PIVOTS || !tin_pivot(s, bx, by, bid)) { capped = true; break; }
            ++pivots;
        }
    }
    if (capped) atomicAdd(&status[T2H_TIN_CAPPED], 1);
    if (act && !s.have) atomicAdd(&status[T2H_TIN_UNRESOLVED], 1);
    if (pivots) atomicAdd(&status[T2H_TIN_PIVOTS], pivots);
    if (walk_pivots) atomicAdd(&status[T2H_TIN_WALK_PIVOTS], walk_pivots);

    const bool found = act && s.have;
    double l0 = NAN, l1 = NAN, l2 = NAN;
    if (found) {
        tin_sort_rows(s);
        tin_bary(s, &l0, &l1, &l2);
    }
    if (MODE == kTinSimplex) {
        tri[3 * pix] = found ? s.ia : -1; tri[3 * pix + 1] = found ? s.ib : -1; tri[3 * pix + 2] = found ? s.ic : -1;
        out[3 * pix] = l0; out[3 * pix + 1] = l1; out[3 * pix + 2] = l2;
    } else {
        double z = NAN;
        if (found)
            z = __dadd_rn(__dadd_rn(__dmul_rn(l0, U[3 * (size_t)s.ia + 2]), __dmul_rn(l1, U[3 * (size_t)s.ib + 2])),
                          __dmul_rn(l2, U[3 * (size_t)s.ic + 2]));
        out[pix] = z;
    }
}

// ------------------------------------------------------------------------------------------ host side

struct TinHullLayout {                                            // byte offsets into the workspace
    size_t counter, poly, part_v, part_i, surv, end;
    int cap;
    explicit TinHullLayout(int64_t M) {
        cap = 1;
        while (cap < M) cap <<= 1;                                // M <= 2^30
        counter = 0;
        poly = 256;
        part_v = poly + up256(8 * (1 + 2 * kTinDirs));
        part_i = part_v + up256((size_t)8 * kTinPartials * kTinDirs);
        surv = part_i + up256((size_t)4 * kTinPartials * kTinDirs);
        end = surv + up256((size_t)4 * cap);
    }
};
constexpr int64_t kTinMaxHullPoints = 1 << 30;

static int tin_search(int mode, const char *what, const double *unique, const int32_t *cell_offsets, int M, double xmin,
                      double ymin, double h, int gx, int gy, double res, int ny, int nx, const int32_t *hull, int n_hull,
                      int32_t *tri, double *out, int32_t *status, t2h_stream_t stream) {
    if (!unique || !cell_offsets || !hull || !out || !status || (mode == kTinSimplex && !tri))
        return fail(T2H_ERR_ARG, "%s: null pointer", what);
    if (((uintptr_t)unique & 7) || ((uintptr_t)out & 7) || ((uintptr_t)cell_offsets & 3) || ((uintptr_t)hull & 3) ||
        ((uintptr_t)status & 3) || ((uintptr_t)tri & 3))
        return fail(T2H_ERR_ARG, "%s: misaligned pointer (float64 arrays: 8 bytes, int32 arrays: 4)", what);
    if (M < 3) return fail(T2H_ERR_ARG, "%s: M = %d unique points (3 or more)", what, M);
    if (n_hull < 3 || n_hull > M) return fail(T2H_ERR_ARG, "%s: n_hull = %d (3 .. M = %d)", what, n_hull, M);
    if (!isfinite(xmin) || !isfinite(ymin) || !(h > 0.0) || !isfinite(h) || !(res > 0.0) || !isfinite(res))
        return fail(T2H_ERR_ARG, "%s: origin (%g, %g), cell edge %g and resolution %g must be finite, the last two positive", what,
                    xmin, ymin, h, res);
    if (gx < 1 || gy < 1 || (int64_t)gx * gy > (int64_t)kTinMaxPoints / 2 + 8)
        return fail(T2H_ERR_ARG, "%s: bad cell grid %d x %d", what, gx, gy);
    if (ny < 1 || nx < 1 || (int64_t)ny * nx > (int64_t)kTinMaxPoints)
        return fail(T2H_ERR_ARG, "%s: bad raster %d x %d (1 .. 2^31 - 1 nodes)", what, ny, nx);
    const int tiles_x = (nx + kTinTile - 1) / kTinTile, tiles_y = (ny + kTinTile - 1) / kTinTile;
    const dim3 grid((unsigned)((int64_t)tiles_x * tiles_y));
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(status, 0, sizeof(int32_t) * kTinCols, s) != hipSuccess) return check_launch(what);
    if (mode == kTinSimplex)
        hipLaunchKernelGGL((tin_search_kernel<kTinSimplex>), grid, dim3(256), 0, s, unique, cell_offsets, M, xmin, ymin, h, gx, gy,
                           res, ny, nx, tiles_x, hull, n_hull, tri, out, status);
    else
        hipLaunchKernelGGL((tin_search_kernel<kTinLinear>), grid, dim3(256), 0, s, unique, cell_offsets, M, xmin, ymin, h, gx, gy,
                           res, ny, nx, tiles_x, hull, n_hull, (int *)nullptr, out, status);
    note_kernel("tin_search_kernel");
    return check_launch(what);
}

}  // namespace t2h

using namespace t2h;

T2H_API size_t t2h_tin_hull_workspace_bytes(int64_t M) { return M < 1 || M > kTinMaxHullPoints ? 0 : TinHullLayout(M).end; }

T2H_API int t2h_tin_hull(const double *unique, int M, double xmin, double ymin, int32_t *hull, int32_t *status, void *workspace,
                         size_t workspace_bytes, t2h_stream_t stream) {
    if (!unique || !hull || !status || !workspace) return fail(T2H_ERR_ARG, "tin_hull: null pointer");
    if (M < 1 || M > kTinMaxHullPoints) return fail(T2H_ERR_ARG, "tin_hull: M = %d unique points (1 .. 2^30)", M);
    if (((uintptr_t)unique & 7) || ((uintptr_t)hull & 3) || ((uintptr_t)status & 3) || ((uintptr_t)workspace & 7))
        return fail(T2H_ERR_ARG, "tin_hull: misaligned pointer (float64 arrays and workspace: 8 bytes, int32 arrays: 4)");
    if (!isfinite(xmin) || !isfinite(ymin)) return fail(T2H_ERR_ARG, "tin_hull: origin (%g, %g) must be finite", xmin, ymin);
    const TinHullLayout L(M);
    if (workspace_bytes < L.end) return fail(T2H_ERR_WORKSPACE, "tin_hull: workspace %zu < %zu bytes", workspace_bytes, L.end);
    hipStream_t s = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    int *counter = reinterpret_cast<int *>(ws + L.counter), *part_i = reinterpret_cast<int *>(ws + L.part_i);
    int *surv = reinterpret_cast<int *>(ws + L.surv);
    double *poly = reinterpret_cast<double *>(ws + L.poly), *part_v = reinterpret_cast<double *>(ws + L.part_v);
    const int nb = (M + 255) / 256 < kTinPartials ? (M + 255) / 256 : kTinPartials;
    hipLaunchKernelGGL(tin_extremes_partial_kernel, dim3(nb), dim3(256), 0, s, unique, M, xmin, ymin, part_v, part_i);
    hipLaunchKernelGGL(tin_extremes_final_kernel, dim3(1), dim3(256), 0, s, unique, xmin, ymin, (const double *)part_v,
                       (const int *)part_i, nb, poly, counter);
    hipLaunchKernelGGL(tin_filter_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, unique, M, xmin, ymin,
                       (const double *)poly, counter, surv);
    hipLaunchKernelGGL(tin_chain_kernel, dim3(1), dim3(256), 0, s, unique, M, xmin, ymin, (const int *)counter, surv, L.cap, hull,
                       status);
    note_kernel("tin_chain_kernel");
    return check_launch("tin_hull");
}

T2H_API int t2h_tin_simplex(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                            int gy, double res, int ny, int nx, const int32_t *hull, int n_hull, int32_t *tri, double *bary,
                            int32_t *status, t2h_stream_t stream) {
    return tin_search(kTinSimplex, "tin_simplex", unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, hull, n_hull, tri,
                      bary, status, stream);
}

T2H_API int t2h_tin_linear(const double *unique, const int32_t *cell_offsets, int M, double xmin, double ymin, double h, int gx,
                           int gy, double res, int ny, int nx, const int32_t *hull, int n_hull, double *out, int32_t *status,
                           t2h_stream_t stream) {
    return tin_search(kTinLinear, "tin_linear", unique, cell_offsets, M, xmin, ymin, h, gx, gy, res, ny, nx, hull, n_hull, nullptr,
                      out, status, stream);
}
