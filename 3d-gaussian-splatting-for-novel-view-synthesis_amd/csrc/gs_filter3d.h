// gs_filter3d.h -- per-row arithmetic of the Mip-Splatting 3D smoothing filter: the sampling interval a camera takes of
// a Gaussian, and the filter applied to the RAW scale and opacity, forward and backward.
//
// Product code in the style of gs_mcmc.h: `GS_HD` bodies that the kernels of gsplat_filter3d.hip inline and that g++ compiles into a
// host test library (csrc/host_filter3d_check.cpp).  The host build is a TEST of this file, never a fallback.
//
// Not in the reference.  Yu et al., "Mip-Splatting: Alias-free 3D Gaussian Splatting" (CVPR 2024), §5.1.
#pragma once
#include "gs_math.h"

namespace gsf3 {

// ---- cameras ---------------------------------------------------------------------------------------------------------------
// What the caller passes, one record per camera (GSPLAT_FILTER3D_CAMERA_FLOATS floats):
//   [0..11] c2w[:3, :4] row-major, [12] fx, [13] fy, [14] cx, [15] cy, [16] W, [17] H, [18..23] padding (not read)
constexpr int CAMERA_FLOATS = 24;
// What the kernel stages per camera (also 24 floats, so that a record is six 16-byte reads):
//   [0..8] R^T row-major (x = r[0] dx + r[1] dy + r[2] dz, ...), [9..11] camera centre, [12] fx, [13] (-m W - cx), [14] ((1 + m) W - cx),
//   [15] fy, [16] (-m H - cy), [17] ((1 + m) H - cy), [18] near, [19] 1 / max(fx, fy)
constexpr int STAGED_FLOATS = 24;
constexpr uint32_t UNSEEN = 0xffffffffu;          // above the bits of every float: the minimum over no camera

GS_HD uint32_t float_bits(float x) { uint32_t u; __builtin_memcpy(&u, &x, 4); return u; }
GS_HD float bits_float(uint32_t u) { float x; __builtin_memcpy(&x, &u, 4); return x; }
GS_HD bool finite_bits(float x) { return (float_bits(x) & 0x7f800000u) != 0x7f800000u; }

// A camera whose focal lengths are not positive finite numbers sees nothing (its near plane is put at +inf).
GS_HD void stage_camera(const float* rec, float near, float margin, float* out) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = rec[j * 4 + i];
    for (int i = 0; i < 3; ++i) out[9 + i] = rec[i * 4 + 3];
    const float fx = rec[12], fy = rec[13], cx = rec[14], cy = rec[15], W = rec[16], H = rec[17];
    const float F = fx > fy ? fx : fy;
    const bool ok = fx > 0.f && fy > 0.f && finite_bits(fx) && finite_bits(fy);
    out[12] = fx; out[13] = -margin * W - cx; out[14] = (1.f + margin) * W - cx;
    out[15] = fy; out[16] = -margin * H - cy; out[17] = (1.f + margin) * H - cy;
    out[18] = ok ? near : INFINITY;
    out[19] = ok ? 1.0f / F : 0.f;
    for (int i = 20; i < STAGED_FLOATS; ++i) out[i] = 0.f;
}

// The bits of z / max(fx, fy) if the staged camera sees the FINITE point p, else UNSEEN.  With z > 0 the bounds on
// u = fx x / z + cx are tested as (lo - cx) z <= fx x <= (hi - cx) z: no division per pair.
GS_HD uint32_t camera_interval(const float* c, float px, float py, float pz) {
    const float dx = px - c[9], dy = py - c[10], dz = pz - c[11];
    const float x = c[0] * dx + c[1] * dy + c[2] * dz;
    const float y = c[3] * dx + c[4] * dy + c[5] * dz;
    const float z = c[6] * dx + c[7] * dy + c[8] * dz;
    const float ux = c[12] * x, vy = c[15] * y;
    const bool seen = z > c[18] && ux >= c[13] * z && ux <= c[14] * z && vy >= c[16] * z && vy <= c[17] * z;
    const uint32_t b = float_bits(z * c[19]);
    return (seen && b != 0u && b < 0x7f800000u) ? b : UNSEEN;
}

// ---- the filter in raw-parameter space -------------------------------------------------------------------------------------
// With s_j = max(exp(scale_raw_j), 1e-6) (the render's activation), sigma = sigmoid(opacity_raw), f the filter's standard deviation:
//   scale_raw'_j = log sqrt(s_j^2 + f^2) = log s_j + L_j / 2,   L_j = log1p(f^2 / s_j^2)
//   log c        = -(L_0 + L_1 + L_2) / 2                        c = sqrt(prod s_j^2 / prod (s_j^2 + f^2)) in (0, 1]
//   opacity_raw' = logit(c sigma) = o + log c - log1p((1 - c) e^o)            (o < 0)
//                                 = log c - log((1 - c) + e^-o)               (o >= 0: e^o may overflow)
// 1 - c is formed from the ratios f^2 / s_j^2 without a difference, so nothing cancels; c itself is never formed and may underflow
// freely.  Reciprocals and the one square root are the 1-ulp device instructions (GS_RCP_FAST): no IEEE division per row.
// A row with f == 0 (or a NaN f) is the identity, bit for bit; so is the opacity of a row whose 1 - c is below 1e-30.
// log1p(q) for q >= 0 from ONE logf: from 1 on, log(fl(1 + q)) is off by the rounding of the sum alone (6e-8 absolute); below, Kahan's
// log(u) q / (u - 1) with u = fl(1 + q) cancels that rounding (u - 1 is exact).  Half the instructions of log1pf, which bounded the
// forward kernel.  An infinite q gives +inf, a NaN a NaN.
GS_HD float log1p_pos(float q) {
    const float u = 1.0f + q, l = logf(u);
    if (!(q < 1.0f)) return l;
    const float d = u - 1.0f;
    return d == 0.f ? q : l * (q / d);
}

struct Row {
    float w[3];        // d scale_raw'_j / d scale_raw_j = s_j^2 / (s_j^2 + f^2); 0 where the 1e-6 clamp is active
    float qw[3];       // d log c / d scale_raw_j = f^2 / (s_j^2 + f^2); 0 where the clamp is active
    float half_l[3];   // L_j / 2
    float log_s[3];    // log s_j: scale_raw_j, or log 1e-6 under the clamp
    float log_c, omc;  // log c, 1 - c
    bool identity;     // f == 0
};

GS_HD void row_terms(const float scale_raw[3], float f, Row& r) {
    r.identity = !(f > 0.f);
    r.log_c = 0.f;
    float q[3];
    for (int j = 0; j < 3; ++j) {
        const float e = expf(scale_raw[j]);
        const bool clamped = e < 1e-6f;
        const float s = clamped ? 1e-6f : e;
        r.log_s[j] = clamped ? -13.815510557964274f : scale_raw[j];
        const float t = f * GS_RCP_FAST(s);
        float l, w, qw;
        if (t < 1e18f) {
            q[j] = t * t;
            l = log1p_pos(q[j]); w = GS_RCP_FAST(1.0f + q[j]); qw = q[j] * w;
        } else {                                           // f^2 / s^2 overflows (or s is a NaN): log(f^2 / s^2), all of the filter
            q[j] = INFINITY;
            l = 2.0f * (logf(f) - r.log_s[j]); w = 0.f; qw = 1.f;
        }
        r.half_l[j] = 0.5f * l;
        r.w[j] = clamped ? 0.f : w;
        r.qw[j] = clamped ? 0.f : qw;
        r.log_c -= r.half_l[j];
    }
    // 1 - c = 1 - (1 + P)^-1/2 = P / (sqrt(1 + P) (sqrt(1 + P) + 1)) with 1 + P = prod (1 + q_j): P is a sum of positive terms
    const float P = (q[0] + q[1] + q[2]) + (q[0] * q[1] + q[0] * q[2] + q[1] * q[2]) + q[0] * q[1] * q[2];
    if (P < 1e30f) {
        const float root = GS_SQRT_FAST(1.0f + P);
        r.omc = P * GS_RCP_FAST(root * (root + 1.0f));
    } else {
        r.omc = 1.0f;                                      // (also where a product is inf x 0: some q_j is infinite, c = 0)
    }
}

GS_HD void apply_row(const float scale_raw[3], float opacity_raw, float f, float scale_out[3], float& opacity_out) {
    Row r;
    row_terms(scale_raw, f, r);
    if (r.identity) {
        for (int j = 0; j < 3; ++j) scale_out[j] = scale_raw[j];
        opacity_out = opacity_raw;
        return;
    }
    for (int j = 0; j < 3; ++j) scale_out[j] = r.log_s[j] + r.half_l[j];
    const float o = opacity_raw;
    if (!(r.omc > 1e-30f)) opacity_out = o + r.log_c;
    else if (o < 0.f) opacity_out = o + r.log_c - log1p_pos(r.omc * expf(o));
    else opacity_out = r.log_c - logf(r.omc + expf(-o));
}

// (g_scale_raw, g_opacity_raw) = J^T (g_scale_out, g_opacity_out); filt gets no gradient.  c and sigma are recomputed.
//   d opacity_raw' / d opacity_raw = (1 - sigma) / (1 - c sigma) = A,   d opacity_raw' / d log c = 1 / (1 - c sigma) = B
//   o >= 0, e = e^-o:  1 - c sigma = (e + 1 - c) / (1 + e);   o < 0, E = e^o:  1 - c sigma = (1 + (1 - c) E) / (1 + E)
GS_HD void apply_row_backward(const float scale_raw[3], float opacity_raw, float f, const float g_scale_out[3], float g_opacity_out,
                              float g_scale_raw[3], float& g_opacity_raw) {
    Row r;
    row_terms(scale_raw, f, r);
    if (r.identity) {
        for (int j = 0; j < 3; ++j) g_scale_raw[j] = g_scale_out[j];
        g_opacity_raw = g_opacity_out;
        return;
    }
    float A = 1.f, B = 0.f;
    if (r.omc > 1e-30f) {
        if (opacity_raw < 0.f) {
            const float E = expf(opacity_raw), d = GS_RCP_FAST(1.0f + r.omc * E);
            A = d; B = (1.0f + E) * d;
        } else {
            const float e = expf(-opacity_raw), d = GS_RCP_FAST(e + r.omc);
            A = e * d; B = (1.0f + e) * d;
        }
    }
    g_opacity_raw = g_opacity_out * A;
    const float g_log_c = g_opacity_out * B;
    for (int j = 0; j < 3; ++j) g_scale_raw[j] = g_scale_out[j] * r.w[j] + g_log_c * r.qw[j];
}

}  // namespace gsf3
