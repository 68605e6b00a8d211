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
#include "gs_entry.h"
#include "gs_metrics.h"

namespace {

using namespace gsmet;

// ---- the tile geometry, the taps and the LDS pitches of gsplat_loss.hip (its own copy: see there for the bank arithmetic)
constexpr int TW = 32, TH = 16, R = 5, TAPS = 11;
constexpr int W1 = TW + 2 * R, H1 = TH + 2 * R;      // region with one halo   42 x 26
constexpr int THREADS = 256;
constexpr int G = 4;                                 // outputs per thread along a row in the horizontal pass
constexpr int GV = 2;                                // rows per thread in the vertical pass
static_assert(TW % G == 0 && TH % GV == 0 && (TH / GV) * TW == THREADS, "tile shape vs register blocking");
constexpr int XP = 44;           // pitch of the input planes (W1 = 42 columns)
constexpr int HP = 36;           // pitch of the horizontally filtered planes (TW = 32 columns)
static_assert(XP >= W1 && XP % 4 == 0 && HP >= TW && HP % 4 == 0, "row pitches: 16-byte rows");

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
// 14 consecutive floats of an LDS row from a 16-byte aligned position
__device__ __forceinline__ void load14(const float* p, float (&a)[G + 10]) {
    const f4v v0 = *reinterpret_cast<const f4v*>(p), v1 = *reinterpret_cast<const f4v*>(p + 4), v2 = *reinterpret_cast<const f4v*>(p + 8);
    const f2v v3 = *reinterpret_cast<const f2v*>(p + 12);
    a[0] = v0.x; a[1] = v0.y; a[2] = v0.z; a[3] = v0.w; a[4] = v1.x; a[5] = v1.y; a[6] = v1.z; a[7] = v1.w;
    a[8] = v2.x; a[9] = v2.y; a[10] = v2.z; a[11] = v2.w; a[12] = v3.x; a[13] = v3.y;
}
static_assert(G == 4, "load14 / the 16-byte stores assume four outputs per thread");

__device__ __forceinline__ void gauss_taps(float g[TAPS]) {
    // exp(-(i - 5)^2 / (2 * 1.5^2)), normalised
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < TAPS; ++i) { const float d = (float)(i - R); g[i] = expf(-(d * d) / 4.5f); s += g[i]; }
    const float inv = 1.0f / s;
    // (the same eleven values in every lane: kept in SGPRs, they cost no vector register)
#pragma unroll
    for (int i = 0; i < TAPS; ++i) g[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g[i] * inv)));
}

struct alignas(16) StatsLds {
    float x[3][H1][XP], y[3][H1][XP];     // the three channels of the region, de-interleaved
    float h[5][H1][HP];                   // horizontally filtered x, y, xx, yy, (x - y)^2 of the channel being processed
};
static_assert(sizeof(StatsLds) <= 52 * 1024, "three workgroups per CU");

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
    for (int k = 0; k < METRICS_MOMENTS; ++k)
        for (int sft = 32; sft > 0; sft >>= 1) s[k] += __shfl_xor(s[k], sft);
    for (int sft = 32; sft > 0; sft >>= 1) cnt += __shfl_xor(cnt, sft);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < METRICS_MOMENTS; ++k) red[tid >> 6][k] = s[k];
        redn[tid >> 6] = cnt;
    }
    __syncthreads();
    double* row = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * METRICS_ROW;
    if (tid < METRICS_MOMENTS) {
        double v = red[0][tid];
        for (int w = 1; w < THREADS / 64; ++w) v += red[w][tid];
        row[tid] = v;
    } else if (tid == METRICS_MOMENTS) {
        long long v = redn[0];
        for (int w = 1; w < THREADS / 64; ++w) v += redn[w];
        row[METRICS_MOMENTS] = __longlong_as_double(v);                     // (the count travels as the 64 bits it is)
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
    for (int k = 0; k < METRICS_MOMENTS; ++k)
        for (int sft = 32; sft > 0; sft >>= 1) s[k] += __shfl_xor(s[k], sft);
    for (int sft = 32; sft > 0; sft >>= 1) cnt += __shfl_xor(cnt, sft);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < METRICS_MOMENTS; ++k) red[tid >> 6][k] = s[k];
        redn[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < METRICS_MOMENTS; ++k) {
            s[k] = red[0][k];
#pragma unroll
            for (int w = 1; w < THREADS / 64; ++w) s[k] += red[w][k];
        }
        cnt = redn[0];
        for (int w = 1; w < THREADS / 64; ++w) cnt += redn[w];
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
    __shared__ double red[3][THREADS / 64];
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
    {   // the region of all three channels at once, every load of the workgroup in flight together (see loss_stats_kernel); pixel
        // e = tid + 256 k of the region as (row, column): stepped, not divided -- 256 = 6 * 42 + 4
        constexpr int N = H1 * W1, SLOTS = (N + THREADS - 1) / THREADS;
        static_assert(THREADS == 6 * W1 + 4, "the stepping below");
        float ra[SLOTS][3], rb[SLOTS][3];
        bool inside[SLOTS];
        const int r_first = tid / W1, c_first = tid - r_first * W1;
        {
            int r = r_first, c = c_first;
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                const int gy = y0 - R + r, gx = x0 - R + c;
                const bool in = r < H1 && gy >= 0 && gy < H && gx >= 0 && gx < W;      // zero outside the image = the zero padding
                const int64_t o = img + ((int64_t)gy * W + gx) * 3;
                inside[k] = in;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) { ra[k][ch] = in ? pred[o + ch] : 0.f; rb[k][ch] = in ? target[o + ch] : 0.f; }
                r += 6; c += 4;
                if (c >= W1) { c -= W1; ++r; }
            }
        }
        {
            int r = r_first, c = c_first;
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) {
                if (r < H1) {
                    float v[3] = {ra[k][0], ra[k][1], ra[k][2]};
                    if (CC && inside[k]) correct_pixel(E, ra[k], v);                   // (outside the image x stays 0: the padding is of the corrected image)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) { s.x[ch][r][c] = v[ch]; s.y[ch][r][c] = rb[k][ch]; }
                }
                r += 6; c += 4;
                if (c >= W1) { c -= W1; ++r; }
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
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();                                                   // the region is staged / the previous channel's h is read
        // horizontal pass of the five products: G outputs per thread from G + 10 inputs (the products formed once per input)
        for (int i = tid; i < H1 * (TW / G); i += THREADS) {
            const int r = i % H1, cc = (i / H1) * G;                       // rows fastest across lanes
            float a[G + 10], b[G + 10], aa[G + 10], bb[G + 10], dd[G + 10];
            load14(&s.x[ch][r][cc], a);
            load14(&s.y[ch][r][cc], b);
#pragma unroll
            for (int t = 0; t < G + 10; ++t) { const float d = a[t] - b[t]; aa[t] = a[t] * a[t]; bb[t] = b[t] * b[t]; dd[t] = d * d; }
            f4v o0, o1, o2, o3, o4;
#pragma unroll
            for (int o = 0; o < G; ++o) {
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    const float w = g[t];
                    a0 += w * a[o + t]; a1 += w * b[o + t]; a2 += w * aa[o + t]; a3 += w * bb[o + t]; a4 += w * dd[o + t];
                }
                o0[o] = a0; o1[o] = a1; o2[o] = a2; o3[o] = a3; o4[o] = a4;
            }
            *reinterpret_cast<f4v*>(&s.h[0][r][cc]) = o0; *reinterpret_cast<f4v*>(&s.h[1][r][cc]) = o1; *reinterpret_cast<f4v*>(&s.h[2][r][cc]) = o2;
            *reinterpret_cast<f4v*>(&s.h[3][r][cc]) = o3; *reinterpret_cast<f4v*>(&s.h[4][r][cc]) = o4;
        }
        __syncthreads();
        // vertical pass -> the SSIM value on the tile: GV rows per thread; the L1 and squared-error terms ride along
        {
            float v[5][GV + 10];
#pragma unroll
            for (int k = 0; k < 5; ++k)
#pragma unroll
                for (int t = 0; t < GV + 10; ++t) v[k][t] = s.h[k][r0 + t][c];
#pragma unroll
            for (int o = 0; o < GV; ++o) {
                if (valid[o]) {
                    float mu1 = 0.f, mu2 = 0.f, e11 = 0.f, e22 = 0.f, edd = 0.f;
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) {
                        const float w = g[t];
                        mu1 += w * v[0][o + t]; mu2 += w * v[1][o + t]; e11 += w * v[2][o + t]; e22 += w * v[3][o + t];
                        edd += w * v[4][o + t];
                    }
                    ssim_acc += (double)ssim_value(mu1, mu2, e11, e22, edd);
                    const double d = (double)s.x[ch][r0 + o + R][c + R] - (double)s.y[ch][r0 + o + R][c + R];
                    l1_acc += fabs(d);
                    sq_acc += d * d;
                }
            }
        }
    }
    // the tile's four sums (fixed order inside the workgroup)
    for (int sft = 32; sft > 0; sft >>= 1) {
        l1_acc += __shfl_xor(l1_acc, sft); sq_acc += __shfl_xor(sq_acc, sft); ssim_acc += __shfl_xor(ssim_acc, sft);
        cnt += __shfl_xor(cnt, sft);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = l1_acc; red[1][tid >> 6] = sq_acc; red[2][tid >> 6] = ssim_acc; redn[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0, e = 0.0;
        long long n = 0;
        for (int k = 0; k < THREADS / 64; ++k) { a += red[0][k]; b += red[1][k]; e += red[2][k]; n += redn[k]; }
        const int64_t blk = blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
        double* row = partial + blk * METRICS_STATS_ROW;
        row[0] = a; row[1] = b; row[2] = e; row[3] = __longlong_as_double(n);                 // (the count travels as the 64 bits it is)
    }
}

// One workgroup per image: its n_tiles rows in a fixed order, in double -> out[image][4] = psnr, ssim, l1, mse
__global__ __launch_bounds__(THREADS) void metrics_finish_kernel(const double* __restrict__ partial, int n_tiles, float* __restrict__ out) {
    __shared__ double red[3][THREADS / 64];
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
    for (int sft = 32; sft > 0; sft >>= 1) {
        a += __shfl_xor(a, sft); b += __shfl_xor(b, sft); e += __shfl_xor(e, sft); cnt += __shfl_xor(cnt, sft);
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = a; red[1][tid >> 6] = b; red[2][tid >> 6] = e; redn[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        a = 0.0; b = 0.0; e = 0.0; cnt = 0;
        for (int k = 0; k < THREADS / 64; ++k) { a += red[0][k]; b += red[1][k]; e += red[2][k]; cnt += redn[k]; }
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
