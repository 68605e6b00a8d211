// gsplat_metrics.hip -- image quality metrics of held-out views (not in the reference): per-image PSNR, SSIM, L1 and
// MSE of a rendered frame against its photograph over a validity mask, optionally after a per-image affine colour correction.
//
// The definitions and the per-pixel / per-image arithmetic are gs_metrics.h (shared with the host test build).  Four kernels:
//   metrics_moments_kernel   (correction only) workgroups of 1024 pixels x images: a thread forms the 21 products of its valid pixels -- in
//                            double, where they are exact -- and counts them, the wave adds its lanes through the __shfl_xor ladder,
//                            the workgroup its four waves in wave order -> one partial row of 22 x 8 bytes in scratch
//   metrics_solve_kernel     (correction only) ONE workgroup per image adds that image's rows in a fixed order in double and thread 0
//                            solves the 4 x 4 normal equations by Cholesky -> the twelve floats of the affine
//   metrics_stats_kernel     the value-only sibling of loss_stats_kernel (gsplat_loss.hip): 32 x 16 tiles x images; x (corrected and
//                            clamped first when asked; zero outside the image, NOT t) and y with a 5-pixel halo in LDS, the three
//                            channels one after the other through the same buffers; the five planes x, y, x^2, y^2, (x - y)^2 filtered
//                            separably; S per pixel and channel; the tile's masked sums of |d|, d^2, S and its number of valid pixels
//                            (in double) -> one partial row of 4 x 8 bytes in scratch.  No derivative maps, no per-pixel scratch.
//   metrics_finish_kernel    ONE workgroup per image adds that image's tile rows in a fixed order in double -> psnr, ssim, l1, mse
// No float atomics and no waiting on another workgroup anywhere: every sum is formed in an order that depends on the image's shape
// alone, so the values are the same bits on every call, stream and rank, and an image of a batch gets the bits it gets alone.
// Pixel counts are integers (int32 inside a workgroup, int64 from there on).  The mask is read at pixels inside the image only.
#include <cstdint>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_blocksum.h"
#include "gs_entry.h"
#include "gs_metrics.h"
#include "gs_ssim_tile.h"

namespace {

using namespace gsmet;

// ---- the fit
constexpr int MOM_PIX = 4;                                   // pixels per thread
constexpr int MOM_BLOCK_PIX = THREADS * MOM_PIX;             // 1024 pixels per workgroup

// n: pixels of ONE image; grid = (workgroups per image, images); partial[(image * gridDim.x + block) * 22] = 21 doubles and the count
__global__ __launch_bounds__(THREADS) void metrics_moments_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  const uint8_t* __restrict__ mask, int64_t n, double* __restrict__ partial) {
    __shared__ double red[THREADS / 64][METRICS_MOMENTS];
    __shared__ int redn[THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.y * n;
    double s[METRICS_MOMENTS];
#pragma unroll
    for (int k = 0; k < METRICS_MOMENTS; ++k) s[k] = 0.0;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < MOM_PIX; ++k) {                        // (a thread's pixels in index order: consecutive lanes, consecutive pixels)
        const int64_t i = (int64_t)blockIdx.x * MOM_BLOCK_PIX + k * THREADS + tid;
        if (i < n && (!mask || mask[base + i])) {
            const float* px = pred + (base + i) * 3;
            const float* py = target + (base + i) * 3;
            const float x[3] = {px[0], px[1], px[2]}, y[3] = {py[0], py[1], py[2]};
            accumulate_moments(x, y, s);
            ++cnt;
        }
    }
#pragma unroll
    for (int k = 0; k < METRICS_MOMENTS; ++k) s[k] = gsblk::ladder(s[k]);
    cnt = gsblk::ladder(cnt);
    gsblk::stage(s, red);
    gsblk::stage(cnt, redn);
    __syncthreads();
    double* row = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * METRICS_ROW;
    if (tid < METRICS_MOMENTS) {
        row[tid] = gsblk::column<THREADS / 64>(red, tid);
    } else if (tid == METRICS_MOMENTS) {
        const long long n = gsblk::column<THREADS / 64>(redn);             // (four waves' counts added in 32 bits: at most 1024)
        row[METRICS_MOMENTS] = __longlong_as_double(n);                     // (the count travels as the 64 bits it is)
    }
}

// One workgroup per image: its n_blocks rows in a fixed order; thread 0 solves.
__global__ __launch_bounds__(THREADS) void metrics_solve_kernel(const double* __restrict__ partial, int n_blocks, float* __restrict__ affine) {
    __shared__ double red[THREADS / 64][METRICS_MOMENTS];
    __shared__ long long redn[THREADS / 64];
    const int tid = threadIdx.x;
    const double* rows = partial + (int64_t)blockIdx.x * n_blocks * METRICS_ROW;
    double s[METRICS_MOMENTS];
#pragma unroll
    for (int k = 0; k < METRICS_MOMENTS; ++k) s[k] = 0.0;
    long long cnt = 0;
    for (int b = tid; b < n_blocks; b += THREADS) {
        const double* row = rows + (int64_t)b * METRICS_ROW;
#pragma unroll
        for (int k = 0; k < METRICS_MOMENTS; ++k) s[k] += row[k];
        cnt += __double_as_longlong(row[METRICS_MOMENTS]);
    }
#pragma unroll
    for (int k = 0; k < METRICS_MOMENTS; ++k) s[k] = gsblk::ladder(s[k]);
    cnt = gsblk::ladder(cnt);
    gsblk::stage(s, red);
    gsblk::stage(cnt, redn);
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < METRICS_MOMENTS; ++k) s[k] = gsblk::column<THREADS / 64>(red, k);
        cnt = gsblk::column<THREADS / 64>(redn);
        float E[12];
        solve_affine(s, (int64_t)cnt, E);
#pragma unroll
        for (int k = 0; k < 12; ++k) affine[(int64_t)blockIdx.x * 12 + k] = E[k];
    }
}

// ---- the statistics
// partial: [image][tile row][tile column][4] (doubles; the count as an int64) = the tile's sums of |x - y|, (x - y)^2 and S over its valid pixels, and their number
// (three waves per SIMD = the three workgroups per CU the LDS allows: left alone the allocator takes 183 VGPRs and falls to two
//  for nothing; asked for three it fits in 168 without scratch)
template <bool CC>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void metrics_stats_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                const uint8_t* __restrict__ mask, const float* __restrict__ affine, int H, int W,
                                                                double* __restrict__ partial) {
    __shared__ StatsLds s;
    __shared__ double red[THREADS / 64][3];
    __shared__ int redn[THREADS / 64];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t plane = (int64_t)H * W;
    const int64_t img = (int64_t)blockIdx.z * plane * 3;
    float g[TAPS];
    gauss_taps(g);
    float E[12];
    if (CC) {
#pragma unroll
        for (int k = 0; k < 12; ++k) E[k] = affine[(int64_t)blockIdx.z * 12 + k];          // (wave-uniform: scalar loads)
    }
    {   // the region of all three channels at once, loaded in one walk and stored in a second (RegionWalk, as loss_stats_kernel)
        float ra[REGION_SLOTS][3], rb[REGION_SLOTS][3];
        bool inside[REGION_SLOTS];
        RegionWalk p(tid);
#pragma unroll
        for (int k = 0; k < REGION_SLOTS; ++k, p.next()) {
            const int gy = y0 - R + p.r, gx = x0 - R + p.c;
            const bool in = p.r < H1 && gy >= 0 && gy < H && gx >= 0 && gx < W;    // zero outside the image = the zero padding
            const int64_t o = img + ((int64_t)gy * W + gx) * 3;
            inside[k] = in;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { ra[k][ch] = in ? pred[o + ch] : 0.f; rb[k][ch] = in ? target[o + ch] : 0.f; }
        }
        RegionWalk q(tid);
#pragma unroll
        for (int k = 0; k < REGION_SLOTS; ++k, q.next()) {
            if (q.r < H1) {
                float v[3] = {ra[k][0], ra[k][1], ra[k][2]};
                if (CC && inside[k]) correct_pixel(E, ra[k], v);                       // (outside the image x stays 0: the padding is of the corrected image)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) { s.x[ch][q.r][q.c] = v[ch]; s.y[ch][q.r][q.c] = rb[k][ch]; }
            }
        }
    }
    // this thread's GV output pixels (rows r0, r0 + 1 of column c): inside the image and valid?  (the mask is read there only)
    const int rg = tid / TW, c = tid - rg * TW, r0 = rg * GV;
    bool valid[GV];
    int cnt = 0;
#pragma unroll
    for (int o = 0; o < GV; ++o) {
        const int gy = y0 + r0 + o, gx = x0 + c;
        valid[o] = gy < H && gx < W;
        if (valid[o] && mask) valid[o] = mask[(int64_t)blockIdx.z * plane + (int64_t)gy * W + gx] != 0;
        cnt += valid[o] ? 1 : 0;
    }
    // (the three sums in double from the first term on: x - y and its square are then exact, and a metric of two fp32 images carries
    //  no more error than its own rounding to fp32 -- 18 double additions per thread beside 2 x 230 FMAs per value)
    double l1_acc = 0.0, sq_acc = 0.0, ssim_acc = 0.0;
#pragma unroll 1                                                           // (one copy: three do not fit in 168 VGPRs without scratch)
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();                                                   // the region is staged / the previous channel's h is read
        // horizontal pass of the five products: G outputs per thread from G + 10 inputs
        for (int i = tid; i < H1 * (TW / G); i += THREADS) {
            const int r = i % H1, cc = (i / H1) * G;
            float v[5][G + 10];
            load14(&s.x[ch][r][cc], v[0]);
            load14(&s.y[ch][r][cc], v[1]);
            stats_planes(v);
            filter_row<5>(g, v, s.h, r, cc);
        }
        __syncthreads();
        // vertical pass -> the SSIM value on the tile: GV rows per thread; the L1 and squared-error terms ride along
        {
            float v[5][GV + 10];
            gather_column(&s.h[0][r0][c], v);
#pragma unroll
            for (int o = 0; o < GV; ++o) {
                if (valid[o]) {
                    float f[5];                                            // mu1, mu2, e11, e22, edd
                    filter_column(g, v, o, f);
                    ssim_acc += (double)ssim_value(f[0], f[1], f[2], f[3], f[4]);
                    const double d = (double)s.x[ch][r0 + o + R][c + R] - (double)s.y[ch][r0 + o + R][c + R];
                    l1_acc += fabs(d);
                    sq_acc += d * d;
                }
            }
        }
    }
    // the tile's four sums (fixed order inside the workgroup)
    // (none of the three can be -0.0: |d| and d d are not negative, and S joins its sum by a plain addition that started at +0.0)
    const double acc[3] = {gsblk::ladder(l1_acc), gsblk::ladder(sq_acc), gsblk::ladder(ssim_acc)};
    cnt = gsblk::ladder(cnt);
    gsblk::stage(acc, red);
    gsblk::stage(cnt, redn);
    __syncthreads();
    if (tid == 0) {
        const int64_t blk = blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
        double* row = partial + blk * METRICS_STATS_ROW;
#pragma unroll
        for (int k = 0; k < 3; ++k) row[k] = gsblk::column<THREADS / 64>(red, k);
        const long long n = gsblk::column<THREADS / 64>(redn);             // (four waves' counts added in 32 bits: at most 512)
        row[3] = __longlong_as_double(n);                                   // (the count travels as the 64 bits it is)
    }
}

// One workgroup per image: its n_tiles rows in a fixed order, in double -> out[image][4] = psnr, ssim, l1, mse
__global__ __launch_bounds__(THREADS) void metrics_finish_kernel(const double* __restrict__ partial, int n_tiles, float* __restrict__ out) {
    __shared__ double red[THREADS / 64][3];
    __shared__ long long redn[THREADS / 64];
    const int tid = threadIdx.x;
    const double* rows = partial + (int64_t)blockIdx.x * n_tiles * METRICS_STATS_ROW;
    double a = 0.0, b = 0.0, e = 0.0;
    long long cnt = 0;
    for (int k = tid; k < n_tiles; k += THREADS) {
        const double* row = rows + (int64_t)k * METRICS_STATS_ROW;
        a += row[0]; b += row[1]; e += row[2];
        cnt += __double_as_longlong(row[3]);
    }
    // (plain additions from +0.0 on: none of the three can be -0.0)
    const double abe[3] = {gsblk::ladder(a), gsblk::ladder(b), gsblk::ladder(e)};
    cnt = gsblk::ladder(cnt);
    gsblk::stage(abe, red);
    gsblk::stage(cnt, redn);
    __syncthreads();
    if (tid == 0) {
        a = gsblk::column<THREADS / 64>(red, 0); b = gsblk::column<THREADS / 64>(red, 1); e = gsblk::column<THREADS / 64>(red, 2);
        cnt = gsblk::column<THREADS / 64>(redn);
        float v[4];
        finish_values(a, b, e, (int64_t)cnt, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) out[(int64_t)blockIdx.x * 4 + k] = v[k];
    }
}

// ---- host side
constexpr int64_t MAX_GRID_YZ = 65535;

int64_t tiles_x(int32_t W) { return ((int64_t)W + TW - 1) / TW; }
int64_t tiles_y(int32_t H) { return ((int64_t)H + TH - 1) / TH; }
int64_t image_tiles(int32_t H, int32_t W) { return tiles_x(W) * tiles_y(H); }
int64_t moment_blocks(int32_t H, int32_t W) { return ((int64_t)H * W + MOM_BLOCK_PIX - 1) / MOM_BLOCK_PIX; }
int64_t round256(int64_t bytes) { return 256 * ((bytes + 255) / 256); }
// scratch = [stats rows: B x tiles x 4 x 8 bytes, rounded up to 256 bytes | with correction: moment rows: B x ceil(H W / 1024) x 22 x 8 bytes, likewise]
int64_t stats_bytes(int64_t B, int32_t H, int32_t W) { return round256(B * image_tiles(H, W) * METRICS_STATS_ROW * 8); }
int64_t moments_bytes(int64_t B, int32_t H, int32_t W) { return round256(B * moment_blocks(H, W) * METRICS_ROW * 8); }

// NULL when the shape is good
const char* shape_error(int32_t B, int32_t H, int32_t W) {
    if (B < 1) return "B must be >= 1";
    if (H < 1) return "H must be >= 1";
    if (W < 1) return "W must be >= 1";
    if (B > MAX_GRID_YZ) return "B must be <= 65535 (the grid's z extent)";
    if (tiles_y(H) > MAX_GRID_YZ || (int64_t)H * W >= ((int64_t)1 << 38)) return "the image is too large";      // (rows per image: an int)
    return nullptr;
}

void launch_fit(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, float* affine, void* scratch,
                hipStream_t st) {
    double* rows = (double*)((char*)scratch + stats_bytes(B, H, W));
    const int64_t blocks = moment_blocks(H, W);
    hipLaunchKernelGGL(metrics_moments_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(THREADS), 0, st, pred, target, mask, (int64_t)H * W, rows);
    hipLaunchKernelGGL(metrics_solve_kernel, dim3((unsigned)B), dim3(THREADS), 0, st, (const double*)rows, (int)blocks, affine);
}

}  // namespace

extern "C" {

int64_t gsplat_metrics_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t flags) {
    if (shape_error(B, H, W) || (flags & ~GSPLAT_METRICS_COLOUR_CORRECT)) return -1;
    return stats_bytes(B, H, W) + ((flags & GSPLAT_METRICS_COLOUR_CORRECT) ? moments_bytes(B, H, W) : 0);
}

int gsplat_metrics_fit_affine(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, float* affine,
                              void* scratch, void* stream) {
    const char* E = "gsplat_metrics_fit_affine";
    if (const char* what = shape_error(B, H, W)) return bad_arg(E, what);
    if (!pred) return bad_arg(E, "pred is NULL");
    if (!target) return bad_arg(E, "target is NULL");
    if (!affine) return bad_arg(E, "affine is NULL");
    if (!scratch) return bad_arg(E, "scratch is NULL");
    if (!aligned(scratch, 8)) return bad_arg(E, "scratch must be 8-byte aligned");
    launch_fit(pred, target, mask, B, H, W, affine, scratch, (hipStream_t)stream);
    return launch_err("gsplat_metrics_fit_affine launch");
}

int gsplat_metrics_forward(const float* pred, const float* target, const uint8_t* mask, int32_t B, int32_t H, int32_t W, int32_t flags,
                           float* affine, float* out, void* scratch, void* stream) {
    const char* E = "gsplat_metrics_forward";
    if (flags & ~GSPLAT_METRICS_COLOUR_CORRECT) return bad_arg(E, "unknown flag");
    if (const char* what = shape_error(B, H, W)) return bad_arg(E, what);
    if (!pred) return bad_arg(E, "pred is NULL");
    if (!target) return bad_arg(E, "target is NULL");
    if (!out) return bad_arg(E, "out is NULL");
    if (!scratch) return bad_arg(E, "scratch is NULL");
    const bool cc = flags & GSPLAT_METRICS_COLOUR_CORRECT;
    if (cc && !affine) return bad_arg(E, "affine is NULL (GSPLAT_METRICS_COLOUR_CORRECT writes the fitted transforms there)");
    if (!aligned(scratch, 8)) return bad_arg(E, "scratch must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* rows = (double*)scratch;
    const dim3 grid((unsigned)tiles_x(W), (unsigned)tiles_y(H), (unsigned)B);
    if (cc) {
        launch_fit(pred, target, mask, B, H, W, affine, scratch, st);
        hipLaunchKernelGGL(metrics_stats_kernel<true>, grid, dim3(THREADS), 0, st, pred, target, mask, (const float*)affine, (int)H, (int)W, rows);
    } else {
        hipLaunchKernelGGL(metrics_stats_kernel<false>, grid, dim3(THREADS), 0, st, pred, target, mask, (const float*)nullptr, (int)H, (int)W, rows);
    }
    hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)B), dim3(THREADS), 0, st, (const double*)rows, (int)image_tiles(H, W), out);
    return launch_err("gsplat_metrics_forward launch");
}

}  // extern "C"
