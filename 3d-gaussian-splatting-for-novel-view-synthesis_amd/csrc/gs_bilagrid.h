// gs_bilagrid.h -- per-view bilateral grids (not in the reference): a low-resolution grid of affine colour transforms per
// training image, sliced at (pixel x, pixel y, pixel luminance) and applied to the rendered frame before the loss, with the gradients
// of the frame and of the grid, and the total variation of a table of grids with its gradient.
//
//   A grid is G[12, L, Y, X] (channel 4 r + k = entry (r, k) of a 3 x 4 affine [M | t], as in gs_exposure.h).  Pixel (i, j) of an
//   H x W image with colour c:
//     u = (j + 0.5) / W (X - 1)        v = (i + 0.5) / H (Y - 1)        z = clamp(lum(c), 0, 1) (L - 1)
//     lum(c) = fma(0.299, c0, fma(0.587, c1, 0.114 c2))
//     x0 = min(floor(u), X - 2), fx = u - x0     (likewise y0, fy and z0, fz)
//     A   = the 12 channels interpolated over the 8 vertices as nested lerps fma(f, b - a, a): along x, then y, then z
//     o_r = fma(A_r0, c0, fma(A_r1, c1, fma(A_r2, c2, A_r3)))                                   (no clamp)
//   A grid that is constant along an axis is reproduced exactly along it (b - a = 0), so the identity grid returns every finite c bit
//   for bit.  Gradients, with T = g_o (x) [c, 1] and D = (the y-lerp at z0 + 1) - (the y-lerp at z0), which is dA/dfz:
//     g_G[vertex] += w_x w_y w_z T                                  (the 8 vertices of the pixel's cell)
//     g_c[k] = fma(A_0k, g_o0, fma(A_1k, g_o1, A_2k g_o2)) + dz lumcoef_k
//     dz     = (L - 1) sum_r g_o[r] (D_r . [c, 1]),   and 0 where the unclamped luminance is <= 0 or >= 1
//   At the identity D is exactly 0, the affine of D is +-0 for every finite c, and g_c is g_o bit for bit.
//
// The per-pixel arithmetic is `GS_HD`: the kernels below inline it and g++ compiles it into a host test library
// (csrc/host_bilagrid_check.cpp).  The host build is a TEST of this file, never a fallback.
//
// Kernels (no float atomics anywhere; nothing depends on which workgroup ran first, on the stream or on the launch):
//   bilagrid_pixel_kernel<BACKWARD>   one thread per pixel over the flat pixel index of ONE image (grid.y = the image): out = A c, or
//                                     g_image.  A wave spans BILAGRID_WAVE_PIX pixels, a workgroup BILAGRID_BLOCK_PIX.  The pixels of a
//                                     workgroup lie in very few (y0, x0) cells: the workgroup first copies the block of vertices they can
//                                     touch -- [12][L][rows y][columns x], the order of the grid itself, a level padded to an odd number
//                                     of floats -- into LDS where it has at most
//                                     BILAGRID_STAGE_FLOATS floats (3 KiB at 1920 x 1080 under the default grid), and every pixel reads its
//                                     96 floats from there; a larger block (a coarse image under a fine grid) is read straight from global
//                                     memory.  The same values through the same arithmetic either way: the same bits.
//   bilagrid_gather_kernel            ONE workgroup per spatial vertex (gy, gx) of one image (grid = (X, Y, images)).  It walks the
//                                     pixels of the vertex's support rectangle -- the pixels whose cell has the vertex as a corner, found
//                                     from integer bounds widened by two pixels and then decided per pixel by the SAME locate() the
//                                     forward uses -- and owns its 12 L outputs: no partial rows, no finish launch, no race under
//                                     ACCUMULATE.  Levels are handled BILAGRID_LEVEL_GROUP at a time (compile-time indices: the
//                                     accumulators stay in registers), one walk of the rectangle per group.  BILAGRID_GATHER_THREADS
//                                     threads: wave w takes the rows w, w + 8, ... of the rectangle as one row-major run of pixels, lane
//                                     l the pixels l, l + 64, ... of that run.
//   bilagrid_tv_kernel / bilagrid_tv_finish_kernel   one thread per grid element (grid.x = the plane (image, channel), grid.y = the plane's
//                                     chunk of 256 elements): the element GATHERS its gradient from its at most six
//                                     neighbours; the loss is per-workgroup partial sums in double, added by one workgroup in a fixed order.
//
// The order of the sums of the grid gradient: a thread adds its pixels in the order of its wave's run, each as ONE
// fma(w, T, sum) onto a rounded weight w = (w_x w_y) w_z and a rounded product T -- gather_thread_pixels() additions at the most; the
// wave adds its 64 lanes through the __shfl_xor ladder (6 additions); one thread per output adds the eight waves' sums from LDS in
// wave order (7 additions): BILAGRID_SUM_DEPTH_FIXED = 13 additions above the thread's own.
#pragma once
#include "gs_math.h"
#if defined(__HIPCC__)
#include "gs_blocksum.h"
#endif

namespace gsbila {

constexpr int BILAGRID_THREADS = 256;
constexpr int BILAGRID_WAVE_PIX = 64;                       // pixels a wave of the per-pixel kernels spans
constexpr int BILAGRID_BLOCK_PIX = BILAGRID_THREADS;        // pixels a workgroup of the per-pixel kernels spans
constexpr int BILAGRID_CHANNELS = 12;
constexpr int BILAGRID_LEVEL_GROUP = 8;                     // luminance levels the gather kernel accumulates in one walk
constexpr int BILAGRID_GATHER_THREADS = 512;                // the gather kernel: eight waves, one row of the rectangle each at a time
constexpr int BILAGRID_SUM_DEPTH_FIXED = 13;                // fp32 additions between a thread's sum and the workgroup's (ladder 6 + waves 7)
constexpr int BILAGRID_STAGE_FLOATS = 8192;                 // the per-pixel kernels stage a block of vertices in LDS up to this size (32 KiB)
constexpr int BILAGRID_MIN = 2, BILAGRID_MAX_XY = 64, BILAGRID_MAX_L = 16;
constexpr int BILAGRID_SUPPORT_SLACK = 2;                   // pixels the integer bounds of a support rectangle are widened by

struct Cell {
    int x0, y0, z0;
    float fx, fy, fz;
    int inside;                                             // the unclamped luminance lies in (0, 1): the luminance derivative is live
};

GS_HD float lerp(float f, float a, float b) { return __builtin_fmaf(f, b - a, a); }

// one axis: position t >= 0 on n vertices -> (cell, fraction)
GS_HD void split_axis(float t, int n, int& k0, float& f) {
    int k = (int)t;                                         // floor: t >= 0
    k0 = k < n - 2 ? k : n - 2;
    f = t - (float)k0;
}

GS_HD float luminance(const float* c) { return __builtin_fmaf(0.299f, c[0], __builtin_fmaf(0.587f, c[1], 0.114f * c[2])); }

// pixel k of n along an image axis, on m vertices: (cell, fraction).  The cell never decreases with k.
GS_HD void locate_axis(int k, int n, int m, int& k0, float& f) { split_axis(((float)k + 0.5f) / (float)n * (float)(m - 1), m, k0, f); }

// the luminance axis; returns whether the unclamped luminance lies in (0, 1)
GS_HD int locate_level(const float* c, int L, int& z0, float& fz) {
    const float lum = luminance(c);
    const float cl = lum > 0.f ? (lum < 1.f ? lum : 1.f) : 0.f;            // (a NaN luminance: 0)
    split_axis(cl * (float)(L - 1), L, z0, fz);
    return lum > 0.f && lum < 1.f;
}

GS_HD Cell locate(int i, int j, int H, int W, int X, int Y, int L, const float* c) {
    Cell q;
    locate_axis(j, W, X, q.x0, q.fx);
    locate_axis(i, H, Y, q.y0, q.fy);
    q.inside = locate_level(c, L, q.z0, q.fz);
    return q;
}

// A[12] (and D[12] = dA/dfz unless NULL) of one pixel; g: the corner (z0, y0, x0) of channel 0 in an array [12][L][rows][columns] with
// the strides sy (a row), sz (a level), sc (a channel)
template <typename P>
GS_HD void slice_at(P g, int64_t sy, int64_t sz, int64_t sc, const Cell& q, float* A, float* D) {
    for (int ch = 0; ch < BILAGRID_CHANNELS; ++ch, g += sc) {
        const float b0 = lerp(q.fy, lerp(q.fx, g[0], g[1]), lerp(q.fx, g[sy], g[sy + 1]));
        const float b1 = lerp(q.fy, lerp(q.fx, g[sz], g[sz + 1]), lerp(q.fx, g[sz + sy], g[sz + sy + 1]));
        A[ch] = __builtin_fmaf(q.fz, b1 - b0, b0);
        if (D) D[ch] = b1 - b0;
    }
}

// ... from a whole grid G[12, L, Y, X]
GS_HD void slice(const float* G, int X, int Y, int L, const Cell& q, float* A, float* D) {
    const int64_t sy = X, sz = (int64_t)Y * X, sc = (int64_t)L * Y * X;
    slice_at(G + q.z0 * sz + q.y0 * sy + q.x0, sy, sz, sc, q, A, D);
}

// o = A c (the nesting of gs_exposure.h)
GS_HD void apply_affine(const float* A, const float* c, float* o) {
    for (int r = 0; r < 3; ++r)
        o[r] = __builtin_fmaf(A[r * 4], c[0], __builtin_fmaf(A[r * 4 + 1], c[1], __builtin_fmaf(A[r * 4 + 2], c[2], A[r * 4 + 3])));
}

// g_c of one pixel
GS_HD void backward_pixel(const float* A, const float* D, const Cell& q, int L, const float* c, const float* go, float* gc) {
    for (int k = 0; k < 3; ++k) gc[k] = __builtin_fmaf(A[k], go[0], __builtin_fmaf(A[4 + k], go[1], A[8 + k] * go[2]));
    if (!q.inside) return;
    float d[3];
    apply_affine(D, c, d);
    const float dz = (float)(L - 1) * __builtin_fmaf(go[0], d[0], __builtin_fmaf(go[1], d[1], go[2] * d[2]));
    gc[0] = __builtin_fmaf(dz, 0.299f, gc[0]);
    gc[1] = __builtin_fmaf(dz, 0.587f, gc[1]);
    gc[2] = __builtin_fmaf(dz, 0.114f, gc[2]);
}

// T = g_o (x) [c, 1]
GS_HD void outer(const float* c, const float* go, float* T) {
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) T[r * 4 + k] = go[r] * c[k];
        T[r * 4 + 3] = go[r];
    }
}

// the weight of vertex k on an axis for a pixel in cell k0 with fraction f (0 unless the vertex is a corner of the cell)
GS_HD float axis_weight(int k, int k0, float f) { return k == k0 ? 1.f - f : (k == k0 + 1 ? f : 0.f); }

// the pixels [lo, hi] of an axis of n pixels over m vertices that may have vertex g as a corner of their cell (a superset)
GS_HD void support(int g, int n, int m, int& lo, int& hi) {
    const int64_t a = ((int64_t)(g - 1) * n) / (m - 1) - BILAGRID_SUPPORT_SLACK, b = ((int64_t)(g + 1) * n) / (m - 1) + BILAGRID_SUPPORT_SLACK;
    lo = (int)(a > 0 ? a : 0);
    hi = (int)(b < n - 1 ? b : n - 1);
}

// the most pixels one thread of the gather kernel adds into one sum: the depth of its own part of the fp32 chain
inline int64_t gather_thread_pixels(int H, int W, int X, int Y) {
    int64_t most = 0;
    for (int gy = 0; gy < Y; ++gy) {
        int ilo, ihi;
        support(gy, H, Y, ilo, ihi);
        for (int gx = 0; gx < X; ++gx) {
            int jlo, jhi;
            support(gx, W, X, jlo, jhi);
            const int64_t rows = (ihi - ilo + 1 + BILAGRID_GATHER_THREADS / 64 - 1) / (BILAGRID_GATHER_THREADS / 64);      // of wave 0: the most
            const int64_t n = (rows * (jhi - jlo + 1) + 63) / 64;
            most = n > most ? n : most;
        }
    }
    return most;
}

// one element of the TV gradient: k[axis] (d_prev - d_next) over the three axes (L, Y, X); *loss += c[axis] d_next^2 (double)
GS_HD float tv_element(const float* g, int x, int y, int l, int X, int Y, int L, const float* k, const double* c, double* loss) {
    const int64_t st[3] = {(int64_t)Y * X, X, 1};
    const int pos[3] = {l, y, x}, len[3] = {L, Y, X};
    float out = 0.f;
    for (int a = 0; a < 3; ++a) {
        float d = 0.f;
        if (pos[a] > 0) d = g[0] - g[-st[a]];
        if (pos[a] + 1 < len[a]) {
            const float dn = g[st[a]] - g[0];
            d -= dn;
            *loss += c[a] * (double)dn * (double)dn;
        }
        out = __builtin_fmaf(k[a], d, out);
    }
    return out;
}

#if defined(__HIPCC__)

// n: pixels of ONE image; grid = (workgroups per image, images).  BACKWARD: dst = g_image (g_out read), else dst = out.
template <bool BACKWARD>
__global__ __launch_bounds__(BILAGRID_THREADS) void bilagrid_pixel_kernel(const float* __restrict__ image, const float* __restrict__ grids,
                                                                           const float* __restrict__ g_out, int H, int W, int X, int Y, int L,
                                                                           float* __restrict__ dst) {
    __shared__ float tile[BILAGRID_STAGE_FLOATS];
    const int tid = threadIdx.x;
    const uint32_t n = (uint32_t)H * (uint32_t)W, first = blockIdx.x * BILAGRID_THREADS, p = first + tid;      // (H W < 2^31: the host checks)
    const uint32_t last = first + BILAGRID_THREADS - 1 < n - 1 ? first + BILAGRID_THREADS - 1 : n - 1;
    const float* G = grids + (int64_t)blockIdx.y * BILAGRID_CHANNELS * L * Y * X;
    // the vertices the workgroup's pixels can touch (the cell of a pixel never decreases along an axis): rows ylo .. ylo + ny - 1,
    // columns xlo .. xlo + nx - 1 -- every column where the pixels span more than one image row.  Uniform over the workgroup.
    const uint32_t uw = (uint32_t)W;
    const int i_first = (int)(first / uw), i_last = (int)(last / uw);
    int ylo, yhi, xlo = 0, xhi = X - 2;
    float unused;
    locate_axis(i_first, H, Y, ylo, unused);
    locate_axis(i_last, H, Y, yhi, unused);
    if (i_first == i_last) {
        locate_axis((int)(first - i_first * uw), W, X, xlo, unused);
        locate_axis((int)(last - i_last * uw), W, X, xhi, unused);
    }
    const int ny = yhi - ylo + 2, nx = xhi - xlo + 2;
    // a level's rows x columns, padded to an odd stride: the lanes of a wave differ mostly in their level, and an even stride (8 at
    // 1920 x 1080 under the default grid) would put levels z and z + 4 on one LDS bank
    const int lz = (ny * nx) | 1;
    const int need = BILAGRID_CHANNELS * L * lz;                               // (at most 12 * 16 * 4097: fits an int)
    const bool staged = need <= BILAGRID_STAGE_FLOATS;
    if (staged) {
        // tile[(ch L + l)][row][column] (a plane lz floats apart), the order of the grid.  The threads count (plane, row, column) with the two inner extents rounded
        // up to powers of two -- shifts and masks where a division by nx and ny would cost more than the slice itself; the counts beyond
        // nx and ny do nothing
        const int bx = 32 - __clz(nx - 1), by = 32 - __clz(ny - 1);           // (nx, ny >= 2)
        const int count = (BILAGRID_CHANNELS * L) << (bx + by);
        for (int e = tid; e < count; e += BILAGRID_THREADS) {
            const int lx = e & ((1 << bx) - 1), ly = (e >> bx) & ((1 << by) - 1), plane = e >> (bx + by);
            if (lx < nx && ly < ny) tile[plane * lz + ly * nx + lx] = G[((int64_t)plane * Y + (ylo + ly)) * X + (xlo + lx)];
        }
        __syncthreads();
    }
    if (p >= n) return;
    const int64_t at = ((int64_t)blockIdx.y * n + p) * 3;
    const float c[3] = {image[at], image[at + 1], image[at + 2]};
    // (row, column) of the pixel from the workgroup's first: a division only where the workgroup's pixels leave that row
    uint32_t i = (uint32_t)i_first, j = first - (uint32_t)i_first * uw + tid;
    if (j >= uw) {
        const uint32_t rows = j / uw;
        i += rows;
        j -= rows * uw;
    }
    const Cell q = locate((int)i, (int)j, H, W, X, Y, L, c);
    float A[BILAGRID_CHANNELS], D[BILAGRID_CHANNELS], o[3];
    if (staged)
        slice_at((const float*)tile + q.z0 * lz + (q.y0 - ylo) * nx + (q.x0 - xlo), nx, lz, L * lz, q, A, BACKWARD ? D : nullptr);
    else
        slice(G, X, Y, L, q, A, BACKWARD ? D : nullptr);
    if (BACKWARD) {
        const float go[3] = {g_out[at], g_out[at + 1], g_out[at + 2]};
        backward_pixel(A, D, q, L, c, go, o);
    } else {
        apply_affine(A, c, o);
    }
    dst[at] = o[0]; dst[at + 1] = o[1]; dst[at + 2] = o[2];
}

// grid = (X, Y, images); row_index / add as in gs_exposure.h's finish kernel; dest is [V, 12, L, Y, X]
__global__ __launch_bounds__(BILAGRID_GATHER_THREADS) void bilagrid_gather_kernel(const float* __restrict__ image, const float* __restrict__ g_out,
                                                                                   int H, int W, int X, int Y, int L,
                                                                                   const int32_t* __restrict__ row_index, int add,
                                                                                   float* __restrict__ dest) {
    constexpr int LG = BILAGRID_LEVEL_GROUP, NS = LG * BILAGRID_CHANNELS, WAVES = BILAGRID_GATHER_THREADS / 64;
    __shared__ float red[WAVES][NS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, gx = blockIdx.x, gy = blockIdx.y;
    const int64_t row = row_index ? (int64_t)row_index[blockIdx.z] : (int64_t)blockIdx.z;
    if (row < 0) return;                                                        // (uniform over the workgroup)
    const int64_t base = (int64_t)blockIdx.z * H * W * 3;
    int ilo, ihi, jlo, jhi;
    support(gy, H, Y, ilo, ihi);
    support(gx, W, X, jlo, jhi);
    const int rw = jhi - jlo + 1;                                               // (>= 1: support() never returns an empty range)
    for (int l0 = 0; l0 < L; l0 += LG) {
        float s[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = 0.f;
        // wave w walks the rows w, w + 8, ... of the rectangle as ONE row-major run of pixels, lane l the pixels l, l + 64, ... of it; the
        // next pixel's colour and gradient are loaded before this one's are used (both loads at once, neither waits for a luminance)
        int i = ilo + wave, j = jlo + lane;
        while (j > jhi) { j -= rw; i += WAVES; }
        float c[3] = {0.f, 0.f, 0.f}, go[3] = {0.f, 0.f, 0.f};
        if (i <= ihi) {
            const int64_t at = base + ((int64_t)i * W + j) * 3;
            c[0] = image[at]; c[1] = image[at + 1]; c[2] = image[at + 2];
            go[0] = g_out[at]; go[1] = g_out[at + 1]; go[2] = g_out[at + 2];
        }
        while (i <= ihi) {
            int i2 = i, j2 = j + 64;
            while (j2 > jhi) { j2 -= rw; i2 += WAVES; }
            float c2[3] = {0.f, 0.f, 0.f}, go2[3] = {0.f, 0.f, 0.f};
            if (i2 <= ihi) {
                const int64_t at = base + ((int64_t)i2 * W + j2) * 3;
                c2[0] = image[at]; c2[1] = image[at + 1]; c2[2] = image[at + 2];
                go2[0] = g_out[at]; go2[1] = g_out[at + 1]; go2[2] = g_out[at + 2];
            }
            int x0, y0, z0;
            float fx, fy, fz;
            locate_axis(j, W, X, x0, fx);
            locate_axis(i, H, Y, y0, fy);
            const float wxy = axis_weight(gx, x0, fx) * axis_weight(gy, y0, fy);
            locate_level(c, L, z0, fz);
            if (wxy != 0.f && z0 + 1 >= l0 && z0 < l0 + LG) {
                float T[BILAGRID_CHANNELS];
                outer(c, go, T);
#pragma unroll
                for (int lg = 0; lg < LG; ++lg) {
                    const float w = wxy * axis_weight(l0 + lg, z0, fz);
                    if (w != 0.f) {
#pragma unroll
                        for (int k = 0; k < BILAGRID_CHANNELS; ++k) s[lg * BILAGRID_CHANNELS + k] = __builtin_fmaf(w, T[k], s[lg * BILAGRID_CHANNELS + k]);
                    }
                }
            }
            i = i2; j = j2;
#pragma unroll
            for (int k = 0; k < 3; ++k) { c[k] = c2[k]; go[k] = go2[k]; }
        }
        // the workgroup's sums, in a fixed order
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = gsblk::ladder(s[k]);
        __syncthreads();                                                        // (the last group's readers are done with red)
        gsblk::stage(s, red);
        __syncthreads();
        const int lg = tid / BILAGRID_CHANNELS, ch = tid % BILAGRID_CHANNELS;
        if (tid < NS && l0 + lg < L) {
            const float x = gsblk::column<WAVES>(red, tid);
            float* d = dest + ((row * BILAGRID_CHANNELS + ch) * L + (l0 + lg)) * Y * X + (int64_t)gy * X + gx;
            *d = add ? *d + x : x;
        }
    }
}

// One thread per element of grids[V, 12, L, Y, X]: blockIdx.x = the plane (image, channel) of L Y X elements, blockIdx.y = the plane's
// chunk of 256.  grad (may be NULL) = or += the element's gradient; partial (may be NULL): the workgroup's share of the loss, in
// double, to partial[blockIdx.x * gridDim.y + blockIdx.y].
__global__ __launch_bounds__(BILAGRID_THREADS) void bilagrid_tv_kernel(const float* __restrict__ grids, int X, int Y, int L, float k0, float k1,
                                                                        float k2, double c0, double c1, double c2, int add,
                                                                        float* __restrict__ grad, double* __restrict__ partial) {
    __shared__ double red[BILAGRID_THREADS / 64];
    const int tid = threadIdx.x, in_plane = blockIdx.y * BILAGRID_THREADS + tid, plane = L * Y * X;
    double loss = 0.0;
    if (in_plane < plane) {
        const int64_t e = (int64_t)blockIdx.x * plane + in_plane;
        const float k[3] = {k0, k1, k2};
        const double c[3] = {c0, c1, c2};
        const float g = tv_element(grids + e, in_plane % X, in_plane / X % Y, in_plane / (X * Y), X, Y, L, k, c, &loss);
        if (grad) grad[e] = add ? grad[e] + g : g;
    }
    if (!partial) return;
    gsblk::sum(loss, red);
    if (tid == 0) partial[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = gsblk::column<BILAGRID_THREADS / 64>(red);
}

// ONE workgroup adds the partial sums in a fixed order, in double; loss_out = (float)(scale * the sum)
__global__ __launch_bounds__(BILAGRID_THREADS) void bilagrid_tv_finish_kernel(const double* __restrict__ partial, int64_t n_blocks, double scale,
                                                                               float* __restrict__ loss_out) {
    __shared__ double red[BILAGRID_THREADS / 64];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int64_t b = tid; b < n_blocks; b += BILAGRID_THREADS) s += partial[b];
    gsblk::sum(s, red);
    if (tid == 0) *loss_out = (float)(scale * gsblk::column<BILAGRID_THREADS / 64>(red));
}

#endif  // __HIPCC__

}  // namespace gsbila
