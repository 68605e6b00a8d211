// gs_aux_loss.h -- the auxiliary loss on the depth / opacity maps of a render, and a target image over a background.
// Part of the translation unit gsplat_loss.hip.
//
//   D = depth [B,H,W], A = alpha [B,H,W] of the render;  Z = target depth (camera-space z), M = target opacity, either may be absent.
//   v_p = [Z_p finite and > 0],  n = B H W,  n_v = max(1, sum v_p):
//     L_alpha = (1 / n)   sum |A - M|
//     L_depth = (1 / n_v) sum v |D - A Z|          (= |sum_i w_i (z_i - Z)|: no division by A, exactly 0 on an empty pixel)
//     total   = scale (l_a L_alpha + l_d L_depth),    values[3] = scale (L_alpha, L_depth, l_a L_alpha + l_d L_depth)
//     g_D = scale up l_d v sign(D - A Z) / n_v,   g_A = scale up (l_a sign(A - M) / n - l_d v Z sign(D - A Z) / n_v),   sign(0) = 0.
//
// Streaming kernels over the flat pixel index (an image boundary means nothing to them): thread i of the launch owns pixels
// 4 i .. 4 i + 3 -- one 16-byte access per array where every array is 16-byte aligned and the four pixels exist, element by
// element otherwise (an unaligned pointer, the ragged end).  Either way a thread adds its four pixels in index order, so the
// alignment of a buffer changes no bit of the result.
//   aux_loss_sums_kernel     the workgroup's three sums (|A - M|, v |D - A Z|, v) -> partial[block][3]; no atomics
//   aux_loss_finish_kernel   ONE workgroup adds the partials in a fixed order, in double -> values, total, and n_v into the header
//                            of scratch, where the backward finds it
//   aux_loss_grad_kernel     g_D, g_A; the upstream scalar is multiplied in here, not by a pass over the gradient
//   composite_target_kernel  out = rgb a + (1 - a) bg   (straight colour; over_background's fma on the rounded product; no clamp)
#pragma once
#include <hip/hip_runtime.h>

#include "gs_blocksum.h"

namespace {

constexpr int AUX_THREADS = 256;
constexpr int AUX_PIX = 4;                                        // pixels per thread
constexpr int AUX_BLOCK_PIX = AUX_THREADS * AUX_PIX;              // 1024 pixels per workgroup
constexpr int64_t AUX_HEADER_BYTES = 256;                         // scratch: [n_v as a double, padded | partial[block][3] floats]

typedef float aux_f4 __attribute__((ext_vector_type(4)));

// four consecutive floats from element `i` of p (n elements in all): one 16-byte load, or what exists of them one by one
__device__ __forceinline__ void aux_load4(const float* __restrict__ p, int64_t i, int64_t n, bool vec, float (&v)[AUX_PIX]) {
    if (vec && i + AUX_PIX <= n) {
        const aux_f4 t = *reinterpret_cast<const aux_f4*>(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < AUX_PIX; ++k) v[k] = i + k < n ? p[i + k] : 0.f;
    }
}

__device__ __forceinline__ void aux_store4(float* __restrict__ p, int64_t i, int64_t n, bool vec, const float (&v)[AUX_PIX]) {
    if (vec && i + AUX_PIX <= n) {
        *reinterpret_cast<aux_f4*>(p + i) = aux_f4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < AUX_PIX; ++k)
            if (i + k < n) p[i + k] = v[k];
    }
}

__device__ __forceinline__ float aux_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
// a target depth counts iff it is finite and > 0 (NaN fails both comparisons)
__device__ __forceinline__ bool aux_valid(float z) { return z > 0.f && z < __builtin_inff(); }
// the composited depth residual D - A Z, the product unrounded
__device__ __forceinline__ float aux_residual(float d, float a, float z) { return __builtin_fmaf(-a, z, d); }

__global__ __launch_bounds__(AUX_THREADS) void aux_loss_sums_kernel(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                                    const float* __restrict__ tdepth, const float* __restrict__ talpha,
                                                                    int64_t n, int vec, float* __restrict__ partial) {
    __shared__ float red[AUX_THREADS / 64][3];
    const int tid = threadIdx.x;
    const int64_t i = ((int64_t)blockIdx.x * AUX_THREADS + tid) * AUX_PIX;
    float sa = 0.f, sd = 0.f, sv = 0.f;
    if (i < n) {
        float a[AUX_PIX];
        aux_load4(alpha, i, n, vec, a);
        if (talpha) {
            float m[AUX_PIX];
            aux_load4(talpha, i, n, vec, m);
#pragma unroll
            for (int k = 0; k < AUX_PIX; ++k) sa += i + k < n ? fabsf(a[k] - m[k]) : 0.f;
        }
        if (tdepth) {
            float d[AUX_PIX], z[AUX_PIX];
            aux_load4(depth, i, n, vec, d);
            aux_load4(tdepth, i, n, vec, z);                       // (past the end: 0 = no data)
#pragma unroll
            for (int k = 0; k < AUX_PIX; ++k) {
                const bool ok = aux_valid(z[k]);
                sd += ok ? fabsf(aux_residual(d[k], a[k], z[k])) : 0.f;
                sv += ok ? 1.f : 0.f;
            }
        }
    }
    // the workgroup's three sums, in a fixed order (the count is exact: at most 1024)
    // (two sums of absolute values and a count: none can be -0.0)
    const float sums[3] = {sa, sd, sv};
    gsblk::sum(sums, red);
    if (tid == 0) {
        float* out = partial + (int64_t)blockIdx.x * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = gsblk::column<AUX_THREADS / 64>(red, k);
    }
}

__global__ __launch_bounds__(AUX_THREADS) void aux_loss_finish_kernel(const float* __restrict__ partial, int n_blocks, double inv_n,
                                                                      float lambda_depth, float lambda_alpha, double scale,
                                                                      float* __restrict__ values, float* __restrict__ total,
                                                                      double* __restrict__ n_valid) {
    __shared__ double red[AUX_THREADS / 64][3];
    const int tid = threadIdx.x;
    double x = 0.0, y = 0.0, c = 0.0;
    for (int k = tid; k < n_blocks; k += AUX_THREADS) {
        x += (double)partial[3 * (int64_t)k]; y += (double)partial[3 * (int64_t)k + 1]; c += (double)partial[3 * (int64_t)k + 2];
    }
    const double sums[3] = {x, y, c};                                       // (of partials that are not negative: none can be -0.0)
    gsblk::sum(sums, red);
    if (tid == 0) {
        x = gsblk::column<AUX_THREADS / 64>(red, 0); y = gsblk::column<AUX_THREADS / 64>(red, 1); c = gsblk::column<AUX_THREADS / 64>(red, 2);
        const double nv = c > 1.0 ? c : 1.0;
        const double la = x * inv_n, ld = y / nv;
        values[0] = (float)(scale * la); values[1] = (float)(scale * ld);
        values[2] = (float)(scale * ((double)lambda_alpha * la + (double)lambda_depth * ld));
        if (total) *total = values[2];
        *n_valid = nv;
    }
}

__global__ __launch_bounds__(AUX_THREADS) void aux_loss_grad_kernel(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                                    const float* __restrict__ tdepth, const float* __restrict__ talpha,
                                                                    int64_t n, int vec, double scale_alpha, double scale_depth,
                                                                    const double* __restrict__ n_valid, const float* __restrict__ upstream,
                                                                    float* __restrict__ grad_depth, float* __restrict__ grad_alpha) {
    // scale_alpha = scale l_a / n, scale_depth = scale l_d: the two per-pixel coefficients, the same in every lane
    const float up = upstream ? *upstream : 1.f;
    const float ca = (float)scale_alpha * up;
    const float cd = tdepth ? (float)(scale_depth / *n_valid) * up : 0.f;
    const int64_t i = ((int64_t)blockIdx.x * AUX_THREADS + threadIdx.x) * AUX_PIX;
    if (i >= n) return;
    float a[AUX_PIX], ga[AUX_PIX], gd[AUX_PIX];
    aux_load4(alpha, i, n, vec, a);
#pragma unroll
    for (int k = 0; k < AUX_PIX; ++k) { ga[k] = 0.f; gd[k] = 0.f; }
    if (talpha) {
        float m[AUX_PIX];
        aux_load4(talpha, i, n, vec, m);
#pragma unroll
        for (int k = 0; k < AUX_PIX; ++k) ga[k] = ca * aux_sign(a[k] - m[k]);
    }
    if (tdepth) {
        float d[AUX_PIX], z[AUX_PIX];
        aux_load4(depth, i, n, vec, d);
        aux_load4(tdepth, i, n, vec, z);
#pragma unroll
        for (int k = 0; k < AUX_PIX; ++k) {
            // (selected, not multiplied by v: a NaN or Inf in Z is "no data", not poison)
            const float s = aux_valid(z[k]) ? cd * aux_sign(aux_residual(d[k], a[k], z[k])) : 0.f;
            gd[k] = s;
            ga[k] -= aux_valid(z[k]) ? s * z[k] : 0.f;
        }
    }
    aux_store4(grad_alpha, i, n, vec, ga);
    if (grad_depth) aux_store4(grad_depth, i, n, vec, gd);
}

struct AuxBackground { float c[3]; };

__global__ __launch_bounds__(AUX_THREADS) void composite_target_kernel(const float* __restrict__ rgb, const float* __restrict__ alpha,
                                                                       AuxBackground bg, int64_t n, int vec, float* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * AUX_THREADS + threadIdx.x) * AUX_PIX;
    if (i >= n) return;
    float a[AUX_PIX], c[3 * AUX_PIX], o[3 * AUX_PIX];
    aux_load4(alpha, i, n, vec, a);
    if (vec && i + AUX_PIX <= n) {                                 // four pixels = 48 bytes of colour, 16-byte aligned with the base
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const aux_f4 t = *reinterpret_cast<const aux_f4*>(rgb + i * 3 + q * 4);
            c[q * 4] = t.x; c[q * 4 + 1] = t.y; c[q * 4 + 2] = t.z; c[q * 4 + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * AUX_PIX; ++k) c[k] = i + k / 3 < n ? rgb[i * 3 + k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 3 * AUX_PIX; ++k) o[k] = __builtin_fmaf(1.0f - a[k / 3], bg.c[k % 3], c[k] * a[k / 3]);
    if (vec && i + AUX_PIX <= n) {
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<aux_f4*>(out + i * 3 + q * 4) = aux_f4{o[q * 4], o[q * 4 + 1], o[q * 4 + 2], o[q * 4 + 3]};
    } else {
#pragma unroll
        for (int k = 0; k < 3 * AUX_PIX; ++k)
            if (i + k / 3 < n) out[i * 3 + k] = o[k];
    }
}

}  // namespace
