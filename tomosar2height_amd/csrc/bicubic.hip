// sample_mode = 'bicubic' (r06): the one other interpolation torch accepts at the reference's two call sites
//
//   F.interpolate(c, size, mode='bicubic', align_corners=True)                                   decoder/pixel.py:107,110
//   F.grid_sample(c, vgrid, padding_mode='border', align_corners=True, mode='bicubic')           encoder/alto.py:95,204
//
// No shipped config selects it (tomosar2height.yaml:27 says bilinear), so these are plain kernels: one thread per output
// element, cubic convolution with A = -0.75 as ATen's upsample_bicubic2d / grid_sampler_2d, taps outside the plane clamped
// to the border pixel (upsample_get_value_bounded; grid_sampler's get_value_bounded with padding_mode = border).  The
// resampling backward is a gather (no atomics, deterministic); the point-sampling backward adds with atomics like
// t2h_sample_bwd_atomic (the order of the additions is not reproducible: documented in include/t2h.h).  The same two samplers on
// the rows of a tile index, regular or ragged (t2h_sample_rows_*, at the end of this file), have a gather adjoint instead.
// Layout: element (b, c, y, x) of a plane at b * sb + c * sc + y * sy + x * sx -- NCHW (sc = h w, sy = w, sx = 1) or NHWC
// (sc = 1, sy = w C, sx = C), chosen by `channels_last`.
#include "t2h_common.h"

namespace t2h {
namespace {

__device__ inline float cc1(float x) { const float A = -0.75f; return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
__device__ inline float cc2(float x) { const float A = -0.75f; return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
__device__ inline void cubic_coeffs(float t, float (&c)[4]) {
    c[0] = cc2(t + 1.f); c[1] = cc1(t); c[2] = cc1(1.f - t); c[3] = cc2(2.f - t);
}
__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct Lay { long long sb, sc, sy, sx; };
__host__ __device__ inline Lay layout(int C, int h, int w, int cl) {
    Lay l;
    l.sb = (long long)C * h * w;
    if (cl) { l.sc = 1; l.sx = C; l.sy = (long long)w * C; }
    else { l.sc = (long long)h * w; l.sx = 1; l.sy = w; }
    return l;
}

// one thread per output element; the fastest index follows the layout (x for NCHW, c for NHWC)
__global__ __launch_bounds__(256) void upsample_bicubic_fwd_kernel(const float *__restrict__ in, const float *__restrict__ addend,
                                                                  int B, int C, int h, int w, int H, int W, float sh, float sw,
                                                                  int cl, float *__restrict__ out) {
    const long long total = (long long)B * C * H * W;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    int b, c, y, x;
    if (cl) { c = (int)(t % C); x = (int)((t / C) % W); y = (int)((t / ((long long)C * W)) % H); b = (int)(t / ((long long)C * W * H)); }
    else { x = (int)(t % W); y = (int)((t / W) % H); c = (int)((t / ((long long)W * H)) % C); b = (int)(t / ((long long)W * H * C)); }
    const Lay li = layout(C, h, w, cl), lo = layout(C, H, W, cl);
    const float ry = sh * (float)y, rx = sw * (float)x;
    const int iy = (int)floorf(ry), ix = (int)floorf(rx);
    float cy[4], cx[4];
    cubic_coeffs(ry - (float)iy, cy);
    cubic_coeffs(rx - (float)ix, cx);
    const float *src = in + b * li.sb + c * li.sc;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float *row = src + clampi(iy - 1 + i, 0, h - 1) * li.sy;
        float r = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) r += row[clampi(ix - 1 + j, 0, w - 1) * li.sx] * cx[j];
        acc += r * cy[i];
    }
    const long long o = b * lo.sb + c * lo.sc + y * lo.sy + x * lo.sx;
    out[o] = addend ? acc + addend[o] : acc;
}

// gather form of the adjoint: input pixel (iy, ix) collects from every output pixel one of whose (clamped) taps is that pixel
__device__ inline void out_range(float scale, int i, int out_size, int &lo, int &hi) {
    if (scale <= 0.f) { lo = 0; hi = out_size - 1; return; }
    lo = max(0, (int)floorf((float)(i - 2) / scale) - 1);          // floor(scale * dst) in [i - 2, i + 1], generous by one
    hi = min(out_size - 1, (int)ceilf((float)(i + 2) / scale) + 1);
}
__device__ inline float tap_weight(float scale, int dst, int in_size, int i) {      // sum of dst's coefficients whose clamped tap is i
    const float r = scale * (float)dst;
    const int f = (int)floorf(r);
    if (f < i - 2 || f > i + 2) return 0.f;
    float c[4];
    cubic_coeffs(r - (float)f, c);
    float wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) wsum += clampi(f - 1 + k, 0, in_size - 1) == i ? c[k] : 0.f;
    return wsum;
}

__global__ __launch_bounds__(256) void upsample_bicubic_bwd_kernel(const float *__restrict__ gout, int B, int C, int h, int w, int H,
                                                                  int W, float sh, float sw, int cl, float *__restrict__ gin) {
    const long long total = (long long)B * C * h * w;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    int b, c, iy, ix;
    if (cl) { c = (int)(t % C); ix = (int)((t / C) % w); iy = (int)((t / ((long long)C * w)) % h); b = (int)(t / ((long long)C * w * h)); }
    else { ix = (int)(t % w); iy = (int)((t / w) % h); c = (int)((t / ((long long)w * h)) % C); b = (int)(t / ((long long)w * h * C)); }
    const Lay li = layout(C, h, w, cl), lo = layout(C, H, W, cl);
    int ylo, yhi, xlo, xhi;
    out_range(sh, iy, H, ylo, yhi);
    out_range(sw, ix, W, xlo, xhi);
    const float *src = gout + b * lo.sb + c * lo.sc;
    float acc = 0.f;
    for (int y = ylo; y <= yhi; ++y) {
        const float wy = tap_weight(sh, y, h, iy);
        if (wy == 0.f) continue;
        float r = 0.f;
        for (int x = xlo; x <= xhi; ++x) {
            const float wx = tap_weight(sw, x, w, ix);
            if (wx != 0.f) r += src[y * lo.sy + x * lo.sx] * wx;
        }
        acc += r * wy;
    }
    gin[b * li.sb + c * li.sc + iy * li.sy + ix * li.sx] = acc;
}

// points [B * N, dim] with x, y in the plane's [0, 1] coordinates (the reference's vgrid = 2 xy - 1 with align_corners=True:
// pixel coordinate = xy (r - 1)); out [B * N, C] point-major.  One thread per (point, channel).
__global__ __launch_bounds__(256) void sample_bicubic_fwd_kernel(const float *__restrict__ plane, const float *__restrict__ pts, int dim,
                                                                long long n_pts, int n_per_b, int r, int C, int cl,
                                                                float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pts * C) return;
    const long long n = t / C;
    const int c = (int)(t % C), b = (int)(n / n_per_b);
    const Lay l = layout(C, r, r, cl);
    const float fx = pts[n * dim] * (float)(r - 1), fy = pts[n * dim + 1] * (float)(r - 1);
    const int ix = (int)floorf(fx), iy = (int)floorf(fy);
    float cx[4], cy[4];
    cubic_coeffs(fx - (float)ix, cx);
    cubic_coeffs(fy - (float)iy, cy);
    const float *src = plane + b * l.sb + c * l.sc;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float *row = src + clampi(iy - 1 + i, 0, r - 1) * l.sy;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += row[clampi(ix - 1 + j, 0, r - 1) * l.sx] * cx[j];
        acc += s * cy[i];
    }
    out[t] = acc;
}

__global__ __launch_bounds__(256) void sample_bicubic_bwd_kernel(const float *__restrict__ gout, const float *__restrict__ pts, int dim,
                                                                long long n_pts, int n_per_b, int r, int C, int cl,
                                                                float *__restrict__ gplane) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pts * C) return;
    const long long n = t / C;
    const int c = (int)(t % C), b = (int)(n / n_per_b);
    const Lay l = layout(C, r, r, cl);
    const float fx = pts[n * dim] * (float)(r - 1), fy = pts[n * dim + 1] * (float)(r - 1);
    const int ix = (int)floorf(fx), iy = (int)floorf(fy);
    float cx[4], cy[4];
    cubic_coeffs(fx - (float)ix, cx);
    cubic_coeffs(fy - (float)iy, cy);
    float *dst = gplane + b * l.sb + c * l.sc;
    const float g = gout[t];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            atomicAdd(dst + clampi(iy - 1 + i, 0, r - 1) * l.sy + clampi(ix - 1 + j, 0, r - 1) * l.sx, g * cx[j] * cy[i]);
}

// mode = 'nearest' (grid_sampler_2d: coordinate clipped to the plane, then nearbyint -- round half to even)
template <bool BWD>
__global__ __launch_bounds__(256) void sample_nearest_kernel(const float *__restrict__ src, const float *__restrict__ pts, int dim,
                                                            long long n_pts, int n_per_b, int r, int C, int cl, float *__restrict__ dst) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pts * C) return;
    const long long n = t / C;
    const int c = (int)(t % C), b = (int)(n / n_per_b);
    const Lay l = layout(C, r, r, cl);
    const float fx = fminf(fmaxf(pts[n * dim] * (float)(r - 1), 0.f), (float)(r - 1));
    const float fy = fminf(fmaxf(pts[n * dim + 1] * (float)(r - 1), 0.f), (float)(r - 1));
    const long long at = b * l.sb + c * l.sc + (long long)rintf(fy) * l.sy + (long long)rintf(fx) * l.sx;
    if (BWD) atomicAdd(dst + at, src[t]);
    else dst[t] = src[at];
}

// ---- the same two samplers on the rows of a tile index, regular or ragged, with a gather adjoint (include/t2h.h) ----------
// tile of sorted row n, from the index: the int bits in the last float of a ragged row, clamped before they address anything; for a
// regular index the b with off0[b M0] <= n < off0[(b + 1) M0] (M0 = 4^nbits)
__device__ inline int tile_of_row(const float *__restrict__ pts, int dim, const int32_t *__restrict__ off0, int B, int ragged, int M0,
                                  long long n) {
    if (ragged) return clampi(__float_as_int(pts[n * dim + dim - 1]), 0, B - 1);
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)off0[(size_t)mid * M0] <= n) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// floor(f) as an int after bounding it AS A FLOAT to [-4, r + 3]: the clamped taps bounded - 1 .. bounded + 2 are those of the
// unbounded index, and no conversion is out of range (NaN: fmaxf returns -4)
__device__ inline int bounded_index(float floor_f, int r) { return (int)fminf(fmaxf(floor_f, -4.f), (float)(r + 3)); }

template <int MODE>
__global__ __launch_bounds__(256) void sample_rows_fwd_kernel(const float *__restrict__ plane, const float *__restrict__ pts, int dim,
                                                             const int32_t *__restrict__ off0, int B, int ragged, int M0,
                                                             long long n_pts, int r, int C, int cl, float *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_pts * C) return;
    const long long n = t / C;
    const int c = (int)(t % C), b = tile_of_row(pts, dim, off0, B, ragged, M0, n);
    const Lay l = layout(C, r, r, cl);
    const float *src = plane + b * l.sb + c * l.sc;
    if (MODE == 0) {                                                   // sample_nearest_kernel<false>
        const float fx = fminf(fmaxf(pts[n * dim] * (float)(r - 1), 0.f), (float)(r - 1));
        const float fy = fminf(fmaxf(pts[n * dim + 1] * (float)(r - 1), 0.f), (float)(r - 1));
        out[t] = src[(long long)rintf(fy) * l.sy + (long long)rintf(fx) * l.sx];
        return;
    }
    const float fx = pts[n * dim] * (float)(r - 1), fy = pts[n * dim + 1] * (float)(r - 1);      // sample_bicubic_fwd_kernel
    const float flx = floorf(fx), fly = floorf(fy);
    const int ix = bounded_index(flx, r), iy = bounded_index(fly, r);
    float cx[4], cy[4];
    cubic_coeffs(fx - flx, cx);
    cubic_coeffs(fy - fly, cy);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float *row = src + clampi(iy - 1 + i, 0, r - 1) * l.sy;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += row[clampi(ix - 1 + j, 0, r - 1) * l.sx] * cx[j];
        acc += s * cy[i];
    }
    out[t] = acc;
}

// cells of pixel p's window on one axis (include/t2h.h); scalar arithmetic on wave-uniform values
__device__ inline void cell_window(int p, int r, int &lo, int &hi) {
    const int q = max(r - 1, 1);
    lo = max(max(p - 2, 0) * r / q - 1, 0);
    hi = min((p + 2) * r / q + 1, r - 1);
}

// "tap hits this pixel" by arithmetic on small integers held as floats: 1 - |tap - pixel| is 1 on the pixel and <= 0 off it.  The
// coefficient is kept or dropped by an AND with 0 / ~0 made from that number -- no compare result, no select
__device__ inline float hits(float tap, float pixel) { return fmaxf(1.f - fabsf(tap - pixel), 0.f); }
__device__ inline float keep_if(float a, float hit) { return __int_as_float(__float_as_int(a) & -(int)hit); }

// weight of pixel (px, py) in the sample of the point (x, y): the forward's taps, recomputed
template <int MODE>
__device__ inline float pixel_weight(float x, float y, int px, int py, int r) {
    if (MODE == 0) {
        const float fx = fminf(fmaxf(x * (float)(r - 1), 0.f), (float)(r - 1));
        const float fy = fminf(fmaxf(y * (float)(r - 1), 0.f), (float)(r - 1));
        // integers as floats: 1 - |rounded - pixel| is 1 on the pixel and <= 0 off it, so the product is exactly 1 or 0
        return hits(rintf(fx), (float)px) * hits(rintf(fy), (float)py);
    }
    const float fx = x * (float)(r - 1), fy = y * (float)(r - 1);
    const float flx = floorf(fx), fly = floorf(fy);
    const float bx = fminf(fmaxf(flx, -4.f), (float)(r + 3)), by = fminf(fmaxf(fly, -4.f), (float)(r + 3));      // bounded_index, as floats
    float cx[4], cy[4];
    cubic_coeffs(fx - flx, cx);
    cubic_coeffs(fy - fly, cy);
    float wx = 0.f, wy = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        wx += keep_if(cx[k], hits(fminf(fmaxf(bx + (float)(k - 1), 0.f), (float)(r - 1)), (float)px));
        wy += keep_if(cy[k], hits(fminf(fmaxf(by + (float)(k - 1), 0.f), (float)(r - 1)), (float)py));
    }
    return wx * wy;
}

// One wave per (tile, pixel, chunk of 64 channels); lanes are channels.  The candidate rows -- the level cells of the pixel's
// window, row by row, each cell's rows ascending -- are visited wave-uniformly; a row's weight is the same in every lane and a row
// of weight zero is skipped by a uniform branch.  Every element of gplane is written once.
// The window holds at most 8 x 8 cells (include/t2h.h): lane 8 jy + jx first loads the row range of window cell (jx, jy), all 64
// ranges in one round trip, and the walk reads them back lane by lane.
template <int MODE>
__global__ __launch_bounds__(64) void sample_rows_bwd_kernel(const float *__restrict__ gout, const float *__restrict__ pts, int dim,
                                                            const int32_t *__restrict__ off0, int n_rows, int nbits, int r, int C,
                                                            int chunks, int cl, float *__restrict__ gplane) {
    const int lane = threadIdx.x;
    const unsigned unit = blockIdx.x;
    const int chunk = (int)(unit % (unsigned)chunks);
    const unsigned pix_all = unit / (unsigned)chunks;
    const int pix = (int)(pix_all % (unsigned)(r * r)), b = (int)(pix_all / (unsigned)(r * r));
    const int px = pix % r, py = pix / r;
    const int shift = 2 * (nbits - (31 - __clz(r)));                  // 2k: a level cell spans 4^k finest cells
    const int32_t *tile_off = off0 + ((size_t)b << (2 * nbits));
    int xlo, xhi, ylo, yhi;
    cell_window(px, r, xlo, xhi);
    cell_window(py, r, ylo, yhi);
    const int nx = min(xhi - xlo + 1, 8), ny = min(yhi - ylo + 1, 8);
    // lanes past the window repeat its last column / row; the walk never reads them
    const unsigned m = morton2((unsigned)(xlo + min(lane & 7, nx - 1)), (unsigned)(ylo + min(lane >> 3, ny - 1)));
    const int first = tile_off[(size_t)m << shift], last = tile_off[(size_t)(m + 1) << shift];
    const int c = chunk * 64 + lane, cr = min(c, C - 1);              // lanes past C read channel C - 1 and store nothing
    float acc = 0.f;
    for (int jy = 0; jy < ny; ++jy)
        for (int jx = 0; jx < nx; ++jx) {
            const int s = max(__builtin_amdgcn_readlane(first, 8 * jy + jx), 0);
            const int e = min(__builtin_amdgcn_readlane(last, 8 * jy + jx), n_rows);
            for (int n = s; n < e; ++n) {
                const float w = pixel_weight<MODE>(pts[(size_t)n * dim], pts[(size_t)n * dim + 1], px, py, r);
                if ((__builtin_amdgcn_readfirstlane(__float_as_int(w)) & 0x7fffffff) != 0)          // w is not +-0
                    acc += gout[(size_t)n * C + cr] * w;
            }
        }
    const Lay l = layout(C, r, r, cl);
    if (c < C) gplane[b * l.sb + c * l.sc + py * l.sy + px * l.sx] = acc;
}

}  // namespace
}  // namespace t2h

using namespace t2h;

T2H_API int t2h_sample_nearest_fwd(const float *plane, const float *pts, int dim, int B, int64_t N, int r, int C, int channels_last,
                                   float *out, t2h_stream_t stream) {
    if (!plane || !pts || !out) return fail(T2H_ERR_ARG, "sample_nearest_fwd: null pointer");
    if (B < 1 || N < 0 || r < 1 || C < 1 || dim < 2) return fail(T2H_ERR_ARG, "sample_nearest_fwd: bad shape");
    if (N == 0) return T2H_OK;
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(sample_nearest_kernel<false>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), plane, pts,
                       dim, (long long)B * N, (int)N, r, C, channels_last, out);
    return check_launch("sample_nearest_fwd");
}

T2H_API int t2h_sample_nearest_bwd(const float *gout, const float *pts, int dim, int B, int64_t N, int r, int C, int channels_last,
                                   float *gplane, t2h_stream_t stream) {
    if (!gout || !pts || !gplane) return fail(T2H_ERR_ARG, "sample_nearest_bwd: null pointer");
    if (B < 1 || N < 0 || r < 1 || C < 1 || dim < 2) return fail(T2H_ERR_ARG, "sample_nearest_bwd: bad shape");
    if (hipMemsetAsync(gplane, 0, (size_t)B * C * r * r * sizeof(float), as_stream(stream)) != hipSuccess)
        return fail(T2H_ERR_LAUNCH, "sample_nearest_bwd: memset failed");
    if (N == 0) return T2H_OK;
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(sample_nearest_kernel<true>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), gout, pts, dim,
                       (long long)B * N, (int)N, r, C, channels_last, gplane);
    return check_launch("sample_nearest_bwd");
}

static int check_planes(const char *what, int B, int C, int h, int w, int H, int W) {
    if (B < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail(T2H_ERR_ARG, "%s: bad shape", what);
    if ((long long)B * C * H * W >= ((long long)1 << 40)) return fail(T2H_ERR_ARG, "%s: too many elements", what);
    return T2H_OK;
}

T2H_API int t2h_upsample_bicubic_fwd(const float *in, const float *addend, int B, int C, int h, int w, int H, int W, int channels_last,
                                     float *out, t2h_stream_t stream) {
    if (!in || !out) return fail(T2H_ERR_ARG, "upsample_bicubic_fwd: null pointer");
    if (int rc = check_planes("upsample_bicubic_fwd", B, C, h, w, H, W)) return rc;
    const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const long long total = (long long)B * C * H * W;
    hipLaunchKernelGGL(upsample_bicubic_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), in, addend,
                       B, C, h, w, H, W, sh, sw, channels_last, out);
    return check_launch("upsample_bicubic_fwd");
}

T2H_API int t2h_upsample_bicubic_bwd(const float *gout, int B, int C, int h, int w, int H, int W, int channels_last, float *gin,
                                     t2h_stream_t stream) {
    if (!gout || !gin) return fail(T2H_ERR_ARG, "upsample_bicubic_bwd: null pointer");
    if (int rc = check_planes("upsample_bicubic_bwd", B, C, h, w, H, W)) return rc;
    const float sh = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sw = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const long long total = (long long)B * C * h * w;
    hipLaunchKernelGGL(upsample_bicubic_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), gout, B, C,
                       h, w, H, W, sh, sw, channels_last, gin);
    return check_launch("upsample_bicubic_bwd");
}

T2H_API int t2h_sample_bicubic_fwd(const float *plane, const float *pts, int dim, int B, int64_t N, int r, int C, int channels_last,
                                   float *out, t2h_stream_t stream) {
    if (!plane || !pts || !out) return fail(T2H_ERR_ARG, "sample_bicubic_fwd: null pointer");
    if (B < 1 || N < 0 || r < 1 || C < 1 || dim < 2) return fail(T2H_ERR_ARG, "sample_bicubic_fwd: bad shape");
    if (N == 0) return T2H_OK;
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(sample_bicubic_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), plane, pts,
                       dim, (long long)B * N, (int)N, r, C, channels_last, out);
    return check_launch("sample_bicubic_fwd");
}

T2H_API int t2h_sample_bicubic_bwd(const float *gout, const float *pts, int dim, int B, int64_t N, int r, int C, int channels_last,
                                   float *gplane, t2h_stream_t stream) {
    if (!gout || !pts || !gplane) return fail(T2H_ERR_ARG, "sample_bicubic_bwd: null pointer");
    if (B < 1 || N < 0 || r < 1 || C < 1 || dim < 2) return fail(T2H_ERR_ARG, "sample_bicubic_bwd: bad shape");
    if (hipMemsetAsync(gplane, 0, (size_t)B * C * r * r * sizeof(float), as_stream(stream)) != hipSuccess)
        return fail(T2H_ERR_LAUNCH, "sample_bicubic_bwd: memset failed");
    if (N == 0) return T2H_OK;
    const long long total = (long long)B * N * C;
    hipLaunchKernelGGL(sample_bicubic_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), gout, pts, dim,
                       (long long)B * N, (int)N, r, C, channels_last, gplane);
    return check_launch("sample_bicubic_bwd");
}

// shared refusals of the two t2h_sample_rows_* entry points (include/t2h.h), before any launch
static int check_rows(const char *what, int dim, int B, int64_t N, int nbits, int r, int C, int mode) {
    if (mode != 0 && mode != 1) return fail(T2H_ERR_ARG, "%s: mode must be 0 (nearest) or 1 (bicubic), got %d", what, mode);
    if (B < 1 || C < 1) return fail(T2H_ERR_ARG, "%s: bad shape (B=%d C=%d)", what, B, C);
    if (N < 0 && B > T2H_MAX_RAGGED_TILES)
        return fail(T2H_ERR_ARG, "%s: a ragged batch holds at most %d tiles (B=%d)", what, T2H_MAX_RAGGED_TILES, B);
    if (dim < (N < 0 ? 3 : 2))
        return fail(T2H_ERR_ARG, "%s: dim=%d: a row holds x, y%s", what, dim, N < 0 ? " and, in a ragged batch, its tile" : "");
    if (nbits < 1 || nbits > T2H_MAX_NBITS) return fail(T2H_ERR_ARG, "%s: nbits=%d outside [1, %d]", what, nbits, T2H_MAX_NBITS);
    if (r < 1 || (r & (r - 1)) || r > (1 << nbits))
        return fail(T2H_ERR_ARG, "%s: r=%d must be a power of two in [1, 2^nbits=%d]", what, r, 1 << nbits);
    const long long rows = N >= 0 ? (long long)B * N : -(long long)N;
    const long long units = (long long)B * r * r * ((C + 63) / 64);
    if (rows >= (1LL << 31) || units >= (1LL << 31) || (rows * C + 255) / 256 >= (1LL << 31))
        return fail(T2H_ERR_ARG, "%s: too many elements (rows=%lld, B r r C/64=%lld)", what, rows, units);
    return T2H_OK;
}

T2H_API int t2h_sample_rows_fwd(const float *plane, const float *pts, int dim, const int32_t *off0, int B, int64_t N, int nbits, int r,
                                int C, int channels_last, int mode, float *out, t2h_stream_t stream) {
    if (!plane || !pts || !off0 || !out) return fail(T2H_ERR_ARG, "sample_rows_fwd: null pointer");
    if (int rc = check_rows("sample_rows_fwd", dim, B, N, nbits, r, C, mode)) return rc;
    const long long rows = N >= 0 ? (long long)B * N : -(long long)N;
    if (rows == 0) return T2H_OK;
    const dim3 grid((unsigned)((rows * C + 255) / 256));
    auto kernel = mode ? sample_rows_fwd_kernel<1> : sample_rows_fwd_kernel<0>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), plane, pts, dim, off0, B, N < 0 ? 1 : 0, 1 << (2 * nbits), rows, r,
                       C, channels_last, out);
    return check_launch("sample_rows_fwd");
}

T2H_API int t2h_sample_rows_bwd(const float *gout, const float *pts, int dim, const int32_t *off0, int B, int64_t N, int nbits, int r,
                                int C, int channels_last, int mode, float *gplane, t2h_stream_t stream) {
    if (!gout || !pts || !off0 || !gplane) return fail(T2H_ERR_ARG, "sample_rows_bwd: null pointer");
    if (int rc = check_rows("sample_rows_bwd", dim, B, N, nbits, r, C, mode)) return rc;
    const long long rows = N >= 0 ? (long long)B * N : -(long long)N;
    if (rows == 0) {                                                  // no index to walk: the gradient is all +0.0
        if (hipMemsetAsync(gplane, 0, (size_t)B * C * r * r * sizeof(float), as_stream(stream)) != hipSuccess)
            return fail(T2H_ERR_LAUNCH, "sample_rows_bwd: memset failed");
        return T2H_OK;
    }
    const int chunks = (C + 63) / 64;
    const dim3 grid((unsigned)((long long)B * r * r * chunks));
    auto kernel = mode ? sample_rows_bwd_kernel<1> : sample_rows_bwd_kernel<0>;
    hipLaunchKernelGGL(kernel, grid, dim3(64), 0, as_stream(stream), gout, pts, dim, off0, (int)rows, nbits, r, C, chunks, channels_last,
                       gplane);
    return check_launch("sample_rows_bwd");
}
