// gsplat_loss.hip -- fused L1 + SSIM training loss (value AND gradient w.r.t. the prediction in one pass).
//
// SURVEY.md §8(f) "next" row 1: reference gaussian_splatting/losses.py:27-185 (l1_loss, ssim_loss, _ssim_single_channel,
// _create_gaussian_window, compute_loss).  The reference runs 15 conv2d calls on permuted copies per view and autograd
// replays them; here two kernels (value + partial-derivative maps, then the gradient) read pred/target twice and write the gradient once.
//
//   L = l1w * mean|x - y| + sw * (1 - mean SSIM),      SSIM per channel with an 11 x 11 Gaussian window (sigma 1.5),
//   zero padding, C1 = 0.01^2, C2 = 0.03^2; the 2-D window is the outer product of a normalised 1-D Gaussian, so every
//   convolution is done separably.
//
// Gradient: with mu1 = w*x, mu2 = w*y, E11 = w*x^2, E22 = w*y^2, E12 = w*xy (w* = windowed sum) and
//   S = A1 A2 / (B1 B2),  A1 = 2 mu1 mu2 + C1, A2 = 2 (E12 - mu1 mu2) + C2, B1 = mu1^2 + mu2^2 + C1,
//   B2 = E11 - mu1^2 + E22 - mu2^2 + C2:
//   dS/dmu1 = 2 mu2 (A2 - A1) / (B1 B2) - 2 mu1 S / B1 + 2 mu1 S / B2,   dS/dE11 = -S / B2,   dS/dE12 = 2 A1 / (B1 B2),
//   d(sum S)/dx(q) = (w * dS/dmu1)(q) + 2 x(q) (w * dS/dE11)(q) + y(q) (w * dS/dE12)(q)     (w is symmetric).
//
// Arithmetic near convergence.  Training ends with x ~ y on smooth images: B2 -> C2 = 9e-4, every sigma^2 = E - mu^2 is the difference
// of two numbers near 1 (1e-7 absolute in fp32 = 1e-4 of B2), and 1 - S ~ (B2 - A2) / B2 is made of what three such differences leave.
// So the fifth filtered plane is (x - y)^2, not x y:  sd = w*(x - y)^2 - (mu1 - mu2)^2 = s11 + s22 - 2 s12 is formed directly
// (it is exactly 0 for x == y),  A2 = B2 - sd,  and the maps are written in terms of dm = mu1 - mu2 and sd, which both vanish at x == y:
//   dS/dmu1           = 2 / (B1 B2) * [ A2 (mu2 dm^2 - dm A1) / B1  -  A1 (mu2 sd - dm A2) / B2 ]      (the same expression, regrouped)
//   u = dS/dE11 + dS/dE12 / 2 = A1 sd / (B1 B2^2)                                                   (stored instead of dS/dE11)
//   d(sum S)/dx(q) = (w * dS/dmu1)(q) + 2 x(q) (w * u)(q) + (y(q) - x(q)) (w * dS/dE12)(q)
// instead of three terms of size 1 / C2 that cancel (a 1-ulp reciprocal alone left 2e-4 of them on an image equal to its target).
//
// TWO kernels per call, 32 x 16 output tiles, the three channels one after the other through the same LDS buffers:
//   loss_stats_kernel   x, y with a 5-pixel halo -> five horizontally filtered planes -> the SSIM value (summed) and the three
//                       partial-derivative maps dS/dmu1, u, dS/dE12 of the tile, written to scratch (planar, 36 B per pixel);
//   loss_grad_kernel    the three maps with a 5-pixel halo -> horizontal, vertical filter -> the gradient (+ the L1 term), written as
//                       whole 12-byte pixels.
// One kernel per 16 x 16 tile with BOTH halos (a 36 x 36 input region, round 2) filtered 3.7 / 2.6 / 1.6 times as many values as
// the tile holds in its three first passes: 432 FMAs per value, 0.24 ms at 1080p, VALU-bound.  Cut in two at the maps, each half
// has one 5-pixel halo: 230 FMAs per value for 72 B per pixel of extra traffic that stays in the 256 MB cache.
// Sums: one pair per workgroup, added up in a fixed order by block 0 of the second kernel (no atomics: the value is reproducible).
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_aux_loss.h"
#include "gs_blocksum.h"
#include "gs_entry.h"
#include "gs_ssim_tile.h"

namespace {

// Sum of the blocks' partial sums in a fixed order (double), by one workgroup: -> values[3] = (l1, 1 - ssim, total)
__device__ __forceinline__ void finish_sums(const float* __restrict__ partial, int n_blocks, double inv_n, float l1w, float sw,
                                            float* __restrict__ values, double (*red)[2], double scale = 1.0,
                                            float* __restrict__ total_out = nullptr) {
    const int tid = threadIdx.x;
    double ab[2] = {0.0, 0.0};                                             // (additions from +0.0 on: neither sum can be -0.0)
    for (int k = tid; k < n_blocks; k += THREADS) { ab[0] += (double)partial[2 * k]; ab[1] += (double)partial[2 * k + 1]; }
    gsblk::sum(ab, red);
    if (tid == 0) {
        const double a = gsblk::column<THREADS / 64>(red, 0), b = gsblk::column<THREADS / 64>(red, 1);
        const double l1 = a * inv_n, sl = 1.0 - b * inv_n;
        values[0] = (float)(scale * l1); values[1] = (float)(scale * sl); values[2] = (float)(scale * (l1w * l1 + sw * sl));
        if (total_out) *total_out = values[2];
    }
}

// maps: [image][channel][3][H][W] (planar: the halo reads of loss_grad_kernel are rows of consecutive floats)
// partial: [block][2] = the block's sums of |x - y| and of the SSIM values (no atomics: the total is formed in a fixed order)
__global__ __launch_bounds__(THREADS) void loss_stats_kernel(const float* __restrict__ pred, const float* __restrict__ target, int H, int W,
                                                             float* __restrict__ partial, float* __restrict__ maps) {
    __shared__ StatsLds s;
    __shared__ float red[THREADS / 64][2];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t img = (int64_t)blockIdx.z * H * W * 3;
    const int64_t plane = (int64_t)H * W;
    float g[TAPS];
    gauss_taps(g);
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float acc[2] = {0.f, 0.f};                                             // the sums of |x - y| and of S
    {   // the region of all three channels at once: rows of 3 * 42 consecutive floats of the interleaved image (the three channels of
        // a pixel are 12 consecutive bytes: one address per pixel and image), loaded in one walk and stored in a second (RegionWalk)
        float ra[REGION_SLOTS][3], rb[REGION_SLOTS][3];
        RegionWalk p(tid);
#pragma unroll
        for (int k = 0; k < REGION_SLOTS; ++k, p.next()) {
            const int gy = y0 - R + p.r, gx = x0 - R + p.c;
            const bool in = p.r < H1 && gy >= 0 && gy < H && gx >= 0 && gx < W;    // zero outside the image = the reference's zero padding
            const int64_t o = img + ((int64_t)gy * W + gx) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { ra[k][ch] = in ? pred[o + ch] : 0.f; rb[k][ch] = in ? target[o + ch] : 0.f; }
        }
        RegionWalk q(tid);
#pragma unroll
        for (int k = 0; k < REGION_SLOTS; ++k, q.next()) {
            if (q.r < H1) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) { s.x[ch][q.r][q.c] = ra[k][ch]; s.y[ch][q.r][q.c] = rb[k][ch]; }
            }
        }
    }
#pragma unroll                                                             // (three copies, as the compiler made of it unasked)
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();                                                   // the region is staged / the previous channel's h is read
        // horizontal pass of the five products: G outputs per thread from G + 10 inputs
        for (int i = tid; i < H1 * (TW / G); i += THREADS) {
            const int r = i % H1, c = (i / H1) * G;
            float v[5][G + 10];
            load14(&s.x[ch][r][c], v[0]);
            load14(&s.y[ch][r][c], v[1]);
            stats_planes(v);
            filter_row<5>(g, v, s.h, r, c);
        }
        __syncthreads();
        // vertical pass -> SSIM value and its partial derivatives on the tile: GV rows per thread; the L1 term rides along
        {
            const int rg = tid / TW, c = tid - rg * TW, r0 = rg * GV;
            float v[5][GV + 10];
            gather_column(&s.h[0][r0][c], v);
#pragma unroll
            for (int o = 0; o < GV; ++o) {
                const int gy = y0 + r0 + o, gx = x0 + c;
                if (gy < H && gx < W) {
                    float f[5];
                    filter_column(g, v, o, f);
                    const float mu1 = f[0], mu2 = f[1], e11 = f[2], e22 = f[3], edd = f[4];
                    const float dm = mu1 - mu2, sd = edd - dm * dm;          // variance of x - y = s11 + s22 - 2 s12: 0 for x == y
                    const float A1 = 2.f * mu1 * mu2 + C1, B1 = mu1 * mu1 + mu2 * mu2 + C1;
                    const float B2 = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2, A2 = B2 - sd;
                    // (B1 >= C1, B2 >= C2 up to rounding: reciprocals by v_rcp_f32, 1 ulp, instead of three IEEE divisions)
                    const float rb1 = __builtin_amdgcn_rcpf(B1), rb2 = __builtin_amdgcn_rcpf(B2);
                    const float ib = rb1 * rb2;
                    const float S = A1 * A2 * ib;
                    acc[1] += S;
                    acc[0] += fabsf(s.x[ch][r0 + o + R][c + R] - s.y[ch][r0 + o + R][c + R]);
                    if (maps) {
                        float* m = maps + ((int64_t)blockIdx.z * 3 + ch) * 3 * plane + (int64_t)gy * W + gx;
                        const float t1 = A2 * rb1 * (mu2 * dm * dm - dm * A1), t2 = A1 * rb2 * (mu2 * sd - dm * A2);
                        m[0] = 2.f * ib * (t1 - t2);
                        m[plane] = A1 * ib * sd * rb2;
                        m[2 * plane] = 2.f * A1 * ib;
                    }
                }
            }
        }
    }
    // the block's two sums (fixed order inside the block)
    gsblk::sum(acc, red);
    if (tid == 0) {
        const int64_t blk = blockIdx.x + (int64_t)gridDim.x * (blockIdx.y + (int64_t)gridDim.y * blockIdx.z);
        partial[2 * blk] = gsblk::column<THREADS / 64>(red, 0);                     // (a sum of |d|: never -0.0)
        // (S may ride an fma into its sum, and a product that underflows from below leaves -0.0 there: "0 +" keeps a tile of
        //  nothing but such values at the +0.0 it has always been, and changes no other sum)
        partial[2 * blk + 1] = 0.f + gsblk::column<THREADS / 64>(red, 1);
    }
}

struct alignas(16) GradLds {
    float p[3][3][H1][XP];       // per channel: dS/dmu1, u = dS/dE11 + dS/dE12 / 2, dS/dE12 with the halo (zero outside the image)
    float q[3][H1][HP];          // horizontally filtered maps of the channel being processed
};
static_assert(sizeof(GradLds) <= 52 * 1024 + 256, "three workgroups per CU");

// d(sum S)/dx(q) = (w * dS/dmu1)(q) + 2 x(q) (w * u)(q) + (y(q) - x(q)) (w * dS/dE12)(q); with the L1 term and the weights -> grad.
// Block (0, 0, 0) also adds up the partial sums loss_stats_kernel left (values[3]).
__global__ __launch_bounds__(THREADS) void loss_grad_kernel(const float* __restrict__ pred, const float* __restrict__ target, int H, int W,
                                                            float l1w, float sw, float inv_n_, double inv_n_d, const float* __restrict__ maps,
                                                            const float* __restrict__ partial, float* __restrict__ values,
                                                            float* __restrict__ grad, const float* __restrict__ upstream) {
    // upstream (nullable device scalar): d L / d total of the caller's graph -- multiplied in here, not by a pass over the gradient
    const float inv_n = upstream ? inv_n_ * *upstream : inv_n_;
    __shared__ GradLds s;
    __shared__ double red[THREADS / 64][2];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t img = (int64_t)blockIdx.z * H * W * 3;
    const int64_t plane = (int64_t)H * W;
    float g[TAPS];
    gauss_taps(g);
    // this thread's GV pixels (rows r0, r0 + 1 of column c): x, y of the three channels, and the gradient as it comes
    const int rg = tid / TW, c = tid - rg * TW, r0 = rg * GV;
    float px[GV][3], py[GV][3], out[GV][3];
    {   // the nine map planes of the region at once (one address per pixel, the nine planes at constant distances), then this
        // thread's pixels, then the stores (RegionWalk, as in loss_stats_kernel)
        const float* m = maps + (int64_t)blockIdx.z * 9 * plane;
        float rp[REGION_SLOTS][9];
        RegionWalk p(tid);
#pragma unroll
        for (int k = 0; k < REGION_SLOTS; ++k, p.next()) {
            const int gy = y0 - R + p.r, gx = x0 - R + p.c;
            const bool in = p.r < H1 && gy >= 0 && gy < H && gx >= 0 && gx < W;
            const float* mp = m + (int64_t)gy * W + gx;
#pragma unroll
            for (int pl = 0; pl < 9; ++pl) rp[k][pl] = in ? mp[pl * plane] : 0.f;
        }
#pragma unroll
        for (int o = 0; o < GV; ++o) {
            const int gy = y0 + r0 + o, gx = x0 + c;
            const bool in = gy < H && gx < W;
            const int64_t a = img + ((int64_t)gy * W + gx) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { px[o][ch] = in ? pred[a + ch] : 0.f; py[o][ch] = in ? target[a + ch] : 0.f; out[o][ch] = 0.f; }
        }
        RegionWalk q(tid);
#pragma unroll
        for (int k = 0; k < REGION_SLOTS; ++k, q.next()) {
            if (q.r < H1) {
#pragma unroll
                for (int pl = 0; pl < 9; ++pl) s.p[pl / 3][pl % 3][q.r][q.c] = rp[k][pl];
            }
        }
    }
    if (values && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        finish_sums(partial, (int)(gridDim.x * gridDim.y * gridDim.z), inv_n_d, l1w, sw, values, red);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        __syncthreads();
        for (int i = tid; i < H1 * (TW / G); i += THREADS) {
            const int r = i % H1, cc = (i / H1) * G;                       // rows fastest across lanes
            float v[3][G + 10];
#pragma unroll
            for (int k = 0; k < 3; ++k) load14(&s.p[ch][k][r][cc], v[k]);
            filter_row<3>(g, v, s.q, r, cc);
        }
        __syncthreads();
        {
            float v[3][GV + 10];
            gather_column(&s.q[0][r0][c], v);
#pragma unroll
            for (int o = 0; o < GV; ++o) {
                float f[3];
                filter_column(g, v, o, f);
                const float cm = f[0], cu = f[1], c12 = f[2];
                const float a = px[o][ch], b = py[o][ch];
                const float d = a - b;
                const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
                out[o][ch] = inv_n * (l1w * sgn - sw * (cm + 2.f * a * cu - d * c12));
            }
        }
    }
#pragma unroll
    for (int o = 0; o < GV; ++o) {
        const int gy = y0 + r0 + o, gx = x0 + c;
        if (gy < H && gx < W) {
            float* gp = grad + img + ((int64_t)gy * W + gx) * 3;
            gp[0] = out[o][0]; gp[1] = out[o][1]; gp[2] = out[o][2];
        }
    }
}

// value only (no gradient asked for): the sums by a kernel of their own
__global__ __launch_bounds__(THREADS) void loss_finish_kernel(const float* __restrict__ partial, int n_blocks, double inv_n, float l1w, float sw,
                                                              float* __restrict__ values, double scale, float* __restrict__ total_out) {
    __shared__ double red[THREADS / 64][2];
    finish_sums(partial, n_blocks, inv_n, l1w, sw, values, red, scale, total_out);
}

}  // namespace

extern "C" {

// scratch = [per block of loss_stats_kernel: 2 partial sums | the three partial-derivative maps of every channel: batch x 3 x 3 x H x W floats]
static int64_t loss_blocks(int64_t batch, int32_t H, int32_t W) { return batch * ((W + TW - 1) / TW) * ((H + TH - 1) / TH); }
static int64_t loss_sums_bytes(int64_t batch, int32_t H, int32_t W) { return 256 * ((loss_blocks(batch, H, W) * 2 * (int64_t)sizeof(float) + 255) / 256); }
int64_t gsplat_loss_scratch_bytes(int64_t batch, int32_t H, int32_t W, int32_t with_grad) {
    if (batch <= 0 || H <= 0 || W <= 0) return -1;
    return loss_sums_bytes(batch, H, W) + (with_grad ? batch * 9 * (int64_t)H * W * (int64_t)sizeof(float) : 0);
}

int gsplat_loss(const float* pred, const float* target, int64_t batch, int32_t H, int32_t W, float lambda_l1, float lambda_ssim,
                float* values, float* grad_pred, void* scratch, void* stream_) {
    if (!pred || !target || !values || !scratch || batch <= 0 || H <= 0 || W <= 0 || batch > 65535 || loss_blocks(batch, H, W) > 0x3FFFFFFF)
        return bad_arg("gsplat_loss", "bad argument");
    hipStream_t st = (hipStream_t)stream_;
    float* partial = (float*)scratch;
    const double n = (double)batch * H * W * 3;
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, (unsigned)batch);
    float* maps = grad_pred ? (float*)((char*)scratch + loss_sums_bytes(batch, H, W)) : nullptr;
    hipLaunchKernelGGL(loss_stats_kernel, grid, dim3(THREADS), 0, st, pred, target, (int)H, (int)W, partial, maps);
    if (grad_pred)
        hipLaunchKernelGGL(loss_grad_kernel, grid, dim3(THREADS), 0, st, pred, target, (int)H, (int)W, lambda_l1, lambda_ssim, (float)(1.0 / n),
                           1.0 / n, (const float*)maps, (const float*)partial, values, grad_pred, (const float*)nullptr);
    else
        hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(THREADS), 0, st, (const float*)partial, (int)loss_blocks(batch, H, W), 1.0 / n,
                           lambda_l1, lambda_ssim, values, 1.0, (float*)nullptr);
    return launch_err("gsplat_loss launch");
}

/* The same loss in two calls, for a caller whose graph supplies d L / d total only later (an autograd node): the forward leaves the
 * partial-derivative maps in scratch, the backward multiplies the upstream scalar and `scale` into the gradient it writes -- no pass
 * over the gradient afterwards, no gradient computed for a value nobody differentiates.                                          */
int gsplat_loss_forward(const float* pred, const float* target, int64_t batch, int32_t H, int32_t W, float lambda_l1, float lambda_ssim,
                        float scale, float* values, float* total, void* scratch, int32_t keep_maps, void* stream_) {
    if (!pred || !target || !values || !scratch || batch <= 0 || H <= 0 || W <= 0 || batch > 65535 || loss_blocks(batch, H, W) > 0x3FFFFFFF)
        return bad_arg("gsplat_loss_forward", "bad argument");
    hipStream_t st = (hipStream_t)stream_;
    float* partial = (float*)scratch;
    const double n = (double)batch * H * W * 3;
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, (unsigned)batch);
    float* maps = keep_maps ? (float*)((char*)scratch + loss_sums_bytes(batch, H, W)) : nullptr;
    hipLaunchKernelGGL(loss_stats_kernel, grid, dim3(THREADS), 0, st, pred, target, (int)H, (int)W, partial, maps);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(THREADS), 0, st, (const float*)partial, (int)loss_blocks(batch, H, W), 1.0 / n,
                       lambda_l1, lambda_ssim, values, (double)scale, total);
    return launch_err("gsplat_loss_forward launch");
}

int gsplat_loss_backward(const float* pred, const float* target, int64_t batch, int32_t H, int32_t W, float lambda_l1, float lambda_ssim,
                         float scale, const float* upstream, float* grad_pred, void* scratch, void* stream_) {
    if (!pred || !target || !grad_pred || !scratch || batch <= 0 || H <= 0 || W <= 0 || batch > 65535 || loss_blocks(batch, H, W) > 0x3FFFFFFF)
        return bad_arg("gsplat_loss_backward", "bad argument");
    const double n = (double)batch * H * W * 3;
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, (unsigned)batch);
    const float* maps = (const float*)((char*)scratch + loss_sums_bytes(batch, H, W));
    hipLaunchKernelGGL(loss_grad_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream_, pred, target, (int)H, (int)W, lambda_l1, lambda_ssim,
                       (float)((double)scale / n), 1.0 / n, maps, (const float*)scratch, (float*)nullptr, grad_pred, upstream);
    return launch_err("gsplat_loss_backward launch");
}

/* ---- the auxiliary loss on the depth / opacity maps, and a target over a background (gs_aux_loss.h) ---- */
// scratch = [256 bytes: n_v = max(1, number of valid target depths) as a double, left by the forward for the backward |
//            three partial sums (|A - M|, v |D - A Z|, v) per workgroup of 1024 pixels, rounded up to 256 bytes]
static int64_t aux_blocks(int64_t batch, int32_t H, int32_t W) { return (batch * (int64_t)H * W + AUX_BLOCK_PIX - 1) / AUX_BLOCK_PIX; }
static bool aux_shape_ok(int64_t batch, int32_t H, int32_t W) {
    return batch > 0 && H > 0 && W > 0 && batch <= 65535 && aux_blocks(batch, H, W) <= 0x3FFFFFFF;
}
static int aux_aligned(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if ((uintptr_t)q % 16) return 0;
    return 1;
}
int64_t gsplat_aux_loss_scratch_bytes(int64_t batch, int32_t H, int32_t W) {
    if (batch <= 0 || H <= 0 || W <= 0) return -1;
    return AUX_HEADER_BYTES + 256 * ((aux_blocks(batch, H, W) * 3 * (int64_t)sizeof(float) + 255) / 256);
}

int gsplat_aux_loss_forward(const float* depth, const float* alpha, const float* target_depth, const float* target_alpha, int64_t batch,
                            int32_t H, int32_t W, float lambda_depth, float lambda_alpha, float scale, float* values, float* total,
                            void* scratch, void* stream_) {
    if (!alpha || !values || !scratch || (target_depth && !depth) || !aux_shape_ok(batch, H, W))
        return bad_arg("gsplat_aux_loss_forward", "bad argument");
    hipStream_t st = (hipStream_t)stream_;
    const int64_t n = batch * (int64_t)H * W, blocks = aux_blocks(batch, H, W);
    float* partial = (float*)((char*)scratch + AUX_HEADER_BYTES);
    const int vec = aux_aligned({depth, alpha, target_depth, target_alpha});
    hipLaunchKernelGGL(aux_loss_sums_kernel, dim3((unsigned)blocks), dim3(AUX_THREADS), 0, st, depth, alpha, target_depth, target_alpha, n, vec,
                       partial);
    hipLaunchKernelGGL(aux_loss_finish_kernel, dim3(1), dim3(AUX_THREADS), 0, st, (const float*)partial, (int)blocks, 1.0 / (double)n,
                       lambda_depth, lambda_alpha, (double)scale, values, total, (double*)scratch);
    return launch_err("gsplat_aux_loss_forward launch");
}

int gsplat_aux_loss_backward(const float* depth, const float* alpha, const float* target_depth, const float* target_alpha, int64_t batch,
                             int32_t H, int32_t W, float lambda_depth, float lambda_alpha, float scale, const float* upstream,
                             float* grad_depth, float* grad_alpha, void* scratch, void* stream_) {
    if (!alpha || !grad_alpha || !scratch || (target_depth && (!depth || !grad_depth)) || !aux_shape_ok(batch, H, W))
        return bad_arg("gsplat_aux_loss_backward", "bad argument");
    const int64_t n = batch * (int64_t)H * W, blocks = aux_blocks(batch, H, W);
    const int vec = aux_aligned({depth, alpha, target_depth, target_alpha, grad_depth, grad_alpha});
    hipLaunchKernelGGL(aux_loss_grad_kernel, dim3((unsigned)blocks), dim3(AUX_THREADS), 0, (hipStream_t)stream_, depth, alpha, target_depth,
                       target_alpha, n, vec, (double)scale * (double)lambda_alpha / (double)n, (double)scale * (double)lambda_depth,
                       (const double*)scratch, upstream, grad_depth, grad_alpha);
    return launch_err("gsplat_aux_loss_backward launch");
}

int gsplat_composite_target(const float* rgb, const float* alpha, const float* background, int64_t batch, int32_t H, int32_t W, float* out,
                            void* stream_) {
    if (!rgb || !alpha || !background || !out || !aux_shape_ok(batch, H, W))
        return bad_arg("gsplat_composite_target", "bad argument");
    const int64_t n = batch * (int64_t)H * W;
    const AuxBackground bg{{background[0], background[1], background[2]}};
    hipLaunchKernelGGL(composite_target_kernel, dim3((unsigned)aux_blocks(batch, H, W)), dim3(AUX_THREADS), 0, (hipStream_t)stream_, rgb, alpha, bg,
                       n, aux_aligned({rgb, alpha, out}), out);
    return launch_err("gsplat_composite_target launch");
}

}  // extern "C"
