// gs_pose_delta.h -- per-view camera-pose corrections (not in the reference): a learned rigid correction per training
// camera, composed with the given pose before the render, with the gradients of the pose and of the nine parameters.
//
//   delta = (d[3], p[3], s[3]), nine floats, zero = the identity: a translation d and the 6-D rotation of Zhou et al. (gsplat's
//   pose_opt parametrisation): no trigonometry, no singularity at the identity.  With c2w = [[R, e], [r3]]:
//     a1 = p + (1,0,0)        a2 = s + (0,1,0)
//     n1 = max(|a1|, 1e-12)   b1 = a1 / n1
//     u2 = a2 - (b1.a2) b1    n2 = max(|u2|, 1e-12)   b2 = u2 / n2      b3 = b1 x b2
//     D  = the 3 x 3 with ROWS b1, b2, b3
//     out[:3,:3] = R D        out[:3,3] = R d + e     out[3,:] = c2w[3,:]
//   An active clamp treats its denominator as a constant in the backward (as F.normalize does).
//   Every product is an fma chain whose innermost term is a lone product (R D) or the addend (R d + e).  With delta = 0, D is exactly
//   I -- 1 / 1, 0 / 1 and 0 - 0 are exact --, two of the three terms of an element of R D are +-0 and the third is R_ik * 1, and the
//   terms of R d are +-0: out equals c2w as numbers for every finite c2w (a -0 may come back as +0).
//
//   Backward, G = grad_out:  g_d = R^T G[:3,3];  G_D = R^T G[:3,:3] goes back through b3 = b1 x b2, the two normalisations and the
//   projection to g_p, g_s;  grad_c2w[:3,:3] = G[:3,:3] D^T + G[:3,3] d^T,  grad_c2w[:3,3] = G[:3,3],  grad_c2w[3,:] = G[3,:].
//
// The per-view arithmetic is `GS_HD`: the kernels below inline it and g++ compiles it into a host test library
// (csrc/host_pose_delta_check.cpp).  The host build is a TEST of this file, never a fallback.
//
// Kernels: ONE lane per view, 64 views per workgroup, one launch per entry; no LDS, no scratch, no atomics.  Every sum is written as
// an explicit fma chain and contraction is off inside the bodies, so a call that skips one half of the backward forms the other half
// with the same instructions: the same bits.
//   pose_delta_forward_kernel    out = compose(c2w, delta)
//   pose_delta_backward_kernel   grad_c2w (if asked for) and the nine floats of grad_delta (if asked for) -> row b, or row row_index[b]
//                                (negative: dropped), stored or added
//   pose_delta_decay_kernel      grad += reg delta   (the table's once-per-iteration L2 term)
#pragma once
#include <cmath>
#include <cstdint>

#include "gs_math.h"

namespace gspd {

constexpr int POSE_DELTA_THREADS = 64;
constexpr int POSE_DELTA_PARAMS = 9;
#define GS_POSE_DELTA_EPS 1e-12f

GS_HD float pd_dot(const float* a, const float* b) { return __builtin_fmaf(a[0], b[0], __builtin_fmaf(a[1], b[1], a[2] * b[2])); }

// c = a x b
GS_HD void pd_cross(const float* a, const float* b, float* c) {
    c[0] = __builtin_fmaf(a[1], b[2], -(a[2] * b[1]));
    c[1] = __builtin_fmaf(a[2], b[0], -(a[0] * b[2]));
    c[2] = __builtin_fmaf(a[0], b[1], -(a[1] * b[0]));
}

// what the backward needs of the forward's rotation: the rows of D, the first factor of u2 and the two (clamped) norms
struct PoseDeltaMid {
    float D[9];          // rows b1, b2, b3
    float a2[3];
    float dot;           // b1 . a2
    float n1, n2;        // after the clamp
    bool c1, c2;         // clamp active?
};

GS_HD void pose_delta_rotation(const float* delta, PoseDeltaMid& m) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float a1[3] = {delta[3] + 1.0f, delta[4], delta[5]};
    m.a2[0] = delta[6]; m.a2[1] = delta[7] + 1.0f; m.a2[2] = delta[8];
    const float l1 = sqrtf(pd_dot(a1, a1));
    m.c1 = l1 < GS_POSE_DELTA_EPS;
    m.n1 = m.c1 ? GS_POSE_DELTA_EPS : l1;
    float* b1 = m.D; float* b2 = m.D + 3; float* b3 = m.D + 6;
    for (int k = 0; k < 3; ++k) b1[k] = a1[k] / m.n1;
    m.dot = pd_dot(b1, m.a2);
    float u2[3];
    for (int k = 0; k < 3; ++k) u2[k] = __builtin_fmaf(-m.dot, b1[k], m.a2[k]);
    const float l2 = sqrtf(pd_dot(u2, u2));
    m.c2 = l2 < GS_POSE_DELTA_EPS;
    m.n2 = m.c2 ? GS_POSE_DELTA_EPS : l2;
    for (int k = 0; k < 3; ++k) b2[k] = u2[k] / m.n2;
    pd_cross(b1, b2, b3);
}

// out[16] = compose(c2w[16], delta[9])
GS_HD void pose_delta_forward_view(const float* c2w, const float* delta, float* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PoseDeltaMid m;
    pose_delta_rotation(delta, m);
    for (int i = 0; i < 3; ++i) {
        const float* R = c2w + i * 4;
        for (int j = 0; j < 3; ++j)
            out[i * 4 + j] = __builtin_fmaf(R[0], m.D[j], __builtin_fmaf(R[1], m.D[3 + j], R[2] * m.D[6 + j]));
        out[i * 4 + 3] = __builtin_fmaf(R[0], delta[0], __builtin_fmaf(R[1], delta[1], __builtin_fmaf(R[2], delta[2], R[3])));
    }
    for (int j = 0; j < 4; ++j) out[12 + j] = c2w[12 + j];
}

// g_c2w[16] and / or g_delta[9] (either may be NULL: not formed) of G[16] = grad_out
GS_HD void pose_delta_backward_view(const float* c2w, const float* delta, const float* G, float* g_c2w, float* g_delta) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    PoseDeltaMid m;
    pose_delta_rotation(delta, m);
    if (g_c2w) {
        for (int i = 0; i < 3; ++i) {
            const float* g = G + i * 4;
            // sum_j G_ij D_kj + G_i3 d_k
            for (int k = 0; k < 3; ++k)
                g_c2w[i * 4 + k] = __builtin_fmaf(g[0], m.D[k * 3], __builtin_fmaf(g[1], m.D[k * 3 + 1], __builtin_fmaf(g[2], m.D[k * 3 + 2], g[3] * delta[k])));
            g_c2w[i * 4 + 3] = g[3];
        }
        for (int j = 0; j < 4; ++j) g_c2w[12 + j] = G[12 + j];
    }
    if (!g_delta) return;
    // R^T G: column 3 is g_d, columns 0..2 are the gradients of the rows of D
    float gD[9];
    for (int k = 0; k < 3; ++k) {
        for (int j = 0; j < 3; ++j) gD[k * 3 + j] = __builtin_fmaf(c2w[k], G[j], __builtin_fmaf(c2w[4 + k], G[4 + j], c2w[8 + k] * G[8 + j]));
        g_delta[k] = __builtin_fmaf(c2w[k], G[3], __builtin_fmaf(c2w[4 + k], G[7], c2w[8 + k] * G[11]));
    }
    const float* b1 = m.D; const float* b2 = m.D + 3;
    float* gb1 = gD; float* gb2 = gD + 3; const float* gb3 = gD + 6;
    // b3 = b1 x b2:  gb1 += b2 x gb3,  gb2 += gb3 x b1
    float t[3];
    pd_cross(b2, gb3, t);
    for (int k = 0; k < 3; ++k) gb1[k] += t[k];
    pd_cross(gb3, b1, t);
    for (int k = 0; k < 3; ++k) gb2[k] += t[k];
    // b2 = u2 / n2
    float gu2[3];
    const float p2 = m.c2 ? 0.0f : pd_dot(gb2, b2);
    for (int k = 0; k < 3; ++k) gu2[k] = __builtin_fmaf(-p2, b2[k], gb2[k]) / m.n2;
    // u2 = a2 - (b1 . a2) b1
    const float q = pd_dot(gu2, b1);
    for (int k = 0; k < 3; ++k) {
        g_delta[6 + k] = __builtin_fmaf(-q, b1[k], gu2[k]);
        gb1[k] -= __builtin_fmaf(q, m.a2[k], m.dot * gu2[k]);
    }
    // b1 = a1 / n1
    const float p1 = m.c1 ? 0.0f : pd_dot(gb1, b1);
    for (int k = 0; k < 3; ++k) g_delta[3 + k] = __builtin_fmaf(-p1, b1[k], gb1[k]) / m.n1;
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(POSE_DELTA_THREADS) void pose_delta_forward_kernel(const float* __restrict__ c2w, const float* __restrict__ delta,
                                                                                int64_t batch, float* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * POSE_DELTA_THREADS + threadIdx.x;
    if (b >= batch) return;
    float c[16], d[POSE_DELTA_PARAMS], o[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) c[k] = c2w[b * 16 + k];
#pragma unroll
    for (int k = 0; k < POSE_DELTA_PARAMS; ++k) d[k] = delta[b * POSE_DELTA_PARAMS + k];
    pose_delta_forward_view(c, d, o);
#pragma unroll
    for (int k = 0; k < 16; ++k) out[b * 16 + k] = o[k];
}

// C2W: write grad_c2w[b]; DEL: write the nine floats to row b of grad_delta, or to row row_index[b] (negative: dropped); add: +=
template <bool C2W, bool DEL>
__global__ __launch_bounds__(POSE_DELTA_THREADS) void pose_delta_backward_kernel(const float* __restrict__ c2w, const float* __restrict__ delta,
                                                                                 const float* __restrict__ grad_out, int64_t batch,
                                                                                 float* __restrict__ grad_c2w, float* __restrict__ grad_delta,
                                                                                 const int32_t* __restrict__ row_index, int add) {
    const int64_t b = (int64_t)blockIdx.x * POSE_DELTA_THREADS + threadIdx.x;
    if (b >= batch) return;
    float c[16], d[POSE_DELTA_PARAMS], g[16], gc[16], gd[POSE_DELTA_PARAMS];
#pragma unroll
    for (int k = 0; k < 16; ++k) { c[k] = c2w[b * 16 + k]; g[k] = grad_out[b * 16 + k]; }
#pragma unroll
    for (int k = 0; k < POSE_DELTA_PARAMS; ++k) d[k] = delta[b * POSE_DELTA_PARAMS + k];
    pose_delta_backward_view(c, d, g, C2W ? gc : nullptr, DEL ? gd : nullptr);
    if (C2W) {
#pragma unroll
        for (int k = 0; k < 16; ++k) grad_c2w[b * 16 + k] = gc[k];
    }
    if (DEL) {
        const int64_t row = row_index ? (int64_t)row_index[b] : b;
        if (row < 0) return;
        float* dst = grad_delta + row * POSE_DELTA_PARAMS;
#pragma unroll
        for (int k = 0; k < POSE_DELTA_PARAMS; ++k) dst[k] = add ? dst[k] + gd[k] : gd[k];
    }
}

__global__ __launch_bounds__(POSE_DELTA_THREADS) void pose_delta_decay_kernel(const float* __restrict__ delta, int64_t n_views, float reg,
                                                                              float* __restrict__ grad) {
    const int64_t v = (int64_t)blockIdx.x * POSE_DELTA_THREADS + threadIdx.x;
    if (v >= n_views) return;
#pragma unroll
    for (int k = 0; k < POSE_DELTA_PARAMS; ++k)
        grad[v * POSE_DELTA_PARAMS + k] = __builtin_fmaf(reg, delta[v * POSE_DELTA_PARAMS + k], grad[v * POSE_DELTA_PARAMS + k]);
}

#endif  // __HIPCC__

}  // namespace gspd
