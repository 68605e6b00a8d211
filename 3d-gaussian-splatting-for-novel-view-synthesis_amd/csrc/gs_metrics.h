// gs_metrics.h -- image quality metrics of held-out views (not in the reference): per-image PSNR, SSIM, L1 and MSE of a
// rendered frame against its photograph, optionally after a per-image affine colour correction fitted by least squares.
//
// Per image, over its n valid pixels (a validity mask, nonzero = valid; without one every pixel is valid):
//     l1   = sum |x - y| / (3 n)        mse = sum (x - y)^2 / (3 n)        psnr = -10 log10(mse)   (+inf for mse == 0)
//     ssim = the SSIM map of the training loss (11 x 11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2, per
//            channel, computed from the WHOLE images: the mask does not alter the window statistics), averaged over the valid pixels
//            and the three channels
//     n == 0: NaN in all four, and in the affine.
// Colour correction: [M | t], twelve floats row-major 3 x 4 (the layout of gs_exposure.h), minimises sum_valid |M x + t - y|^2.
//     With xt = [x; 1]:  A = sum_valid xt xt^T (10 distinct sums),  C = sum_valid xt y^T (12 sums);
//     (A + lambda n D) P = C + lambda n [I3; 0],  D = diag(1, 1, 1, 0),  lambda = 1e-8  (a ridge toward the identity: a constant-colour
//     image has a defined answer);  [M | t] = P^T.  The metrics are then taken between clamp(M x + t, 0, 1) and y.
//
// Everything here is `GS_HD`: the kernels of gsplat_metrics.hip inline it and g++ compiles it into a host test library
// (csrc/host_metrics_check.cpp).  The host build is a TEST of this file, never a fallback.
#pragma once
#include "gs_math.h"

namespace gsmet {

constexpr int METRICS_MOMENTS = 21;          // the sums of the fit (the 22nd, the number of valid pixels, is an integer)
constexpr int METRICS_ROW = 22;              // 8-byte words of a workgroup's partial row of the fit: 21 doubles and the int64 count
constexpr int METRICS_STATS_ROW = 4;         // 8-byte words of a tile's partial row: sum |d|, sum d^2, sum S (doubles) and the int64 count
constexpr double METRICS_RIDGE = 1e-8;

#if defined(__HIPCC__)
#define GSMET_UNROLL _Pragma("unroll")
#else
#define GSMET_UNROLL
#endif

// clamp(M c + t, 0, 1): the nesting of gsexp::apply_pixel (the same bits before the clamp), then the clamp
GS_HD void correct_pixel(const float* E, const float* c, float* o) {
    for (int r = 0; r < 3; ++r) {
        const float v = __builtin_fmaf(E[r * 4], c[0], __builtin_fmaf(E[r * 4 + 1], c[1], __builtin_fmaf(E[r * 4 + 2], c[2], E[r * 4 + 3])));
        o[r] = __builtin_fminf(__builtin_fmaxf(v, 0.f), 1.f);
    }
}

// One valid pixel joins a thread's 21 sums:
//   s[0..5] = x0x0 x0x1 x0x2 x1x1 x1x2 x2x2,  s[6..8] = x,  s[9..17] = x_i y_j (i * 3 + j),  s[18..20] = y
// In double from the first product on.  The product of two floats is exact in double, so A stays a sum of exact outer products: the
// ridge (1e-8 of A's scale) is what decides a constant-colour or a one-pixel image, and products rounded to fp32 (6e-8) would bury it --
// the rounded A of a constant colour is indefinite as often as not.
GS_HD void accumulate_moments(const float* xf, const float* yf, double* s) {
    const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]}, y[3] = {(double)yf[0], (double)yf[1], (double)yf[2]};
    s[0] += x[0] * x[0]; s[1] += x[0] * x[1]; s[2] += x[0] * x[2];
    s[3] += x[1] * x[1]; s[4] += x[1] * x[2]; s[5] += x[2] * x[2];
    for (int i = 0; i < 3; ++i) {
        s[6 + i] += x[i];
        for (int j = 0; j < 3; ++j) s[9 + i * 3 + j] += x[i] * y[j];
        s[18 + i] += y[i];
    }
}

// The affine of one image from its 21 sums (double) and its count: Cholesky on the 4 x 4 system (symmetric positive definite for
// n > 0: v^T A v = sum (m . x + c)^2 >= 0, the ridge adds lambda n |m|^2, and for m = 0 what is left is n c^2), three right-hand sides.
// Every index below is a constant after unrolling: the arrays stay in registers.  n == 0: NaN.
GS_HD void solve_affine(const double* s, int64_t n, float* affine) {
    if (n <= 0) {
        for (int k = 0; k < 12; ++k) affine[k] = __builtin_nanf("");
        return;
    }
    const double ridge = METRICS_RIDGE * (double)n;
    double a[4][4], c[4][3], l[4][4];
    a[0][0] = s[0] + ridge; a[1][0] = s[1]; a[2][0] = s[2];
    a[1][1] = s[3] + ridge; a[2][1] = s[4]; a[2][2] = s[5] + ridge;
    a[3][3] = (double)n;
    GSMET_UNROLL
    for (int i = 0; i < 3; ++i) {
        a[3][i] = s[6 + i];
        GSMET_UNROLL
        for (int j = 0; j < 3; ++j) c[i][j] = s[9 + i * 3 + j] + (i == j ? ridge : 0.0);
        c[3][i] = s[18 + i];
    }
    GSMET_UNROLL
    for (int j = 0; j < 4; ++j) {                                // A = L L^T, the lower triangle only
        double d = a[j][j];
        GSMET_UNROLL
        for (int k = 0; k < j; ++k) d -= l[j][k] * l[j][k];
        l[j][j] = sqrt(d);
        const double inv = 1.0 / l[j][j];
        GSMET_UNROLL
        for (int i = j + 1; i < 4; ++i) {
            double v = a[i][j];
            GSMET_UNROLL
            for (int k = 0; k < j; ++k) v -= l[i][k] * l[j][k];
            l[i][j] = v * inv;
        }
    }
    GSMET_UNROLL
    for (int j = 0; j < 3; ++j) {                                // L z = c_j, L^T p = z: column j of P is row j of [M | t]
        double z[4], p[4];
        GSMET_UNROLL
        for (int k = 0; k < 4; ++k) {
            double v = c[k][j];
            GSMET_UNROLL
            for (int q = 0; q < k; ++q) v -= l[k][q] * z[q];
            z[k] = v / l[k][k];
        }
        GSMET_UNROLL
        for (int k = 3; k >= 0; --k) {
            double v = z[k];
            GSMET_UNROLL
            for (int q = k + 1; q < 4; ++q) v -= l[q][k] * p[q];
            p[k] = v / l[k][k];
        }
        GSMET_UNROLL
        for (int k = 0; k < 4; ++k) affine[j * 4 + k] = (float)p[k];
    }
}

// The SSIM value of one pixel and channel from its five windowed sums mu1 = w*x, mu2 = w*y, e11 = w*x^2, e22 = w*y^2,
// edd = w*(x - y)^2: the training loss's formulation (gsplat_loss.hip) -- sd = edd - (mu1 - mu2)^2 is exactly 0 for x == y.
// Unlike the loss, which only needs 1 - S small there, a metric of an image against itself must be EXACTLY 1: no contraction into
// fused multiply-adds (2 mu mu + C1 and mu mu + mu mu + C1 are then the same bits) and one IEEE division of two equal products
// instead of two 1-ulp reciprocals.  On the device the pragma below switches contraction off; g++ has no such pragma, so the host
// builds of this header (csrc/Makefile, `make check-asan-metrics`) pass -ffp-contract=off -- with that, host and device compute the
// same bits; a host build without it, for a target that has FMA instructions, may lose the exact 1.
GS_HD float ssim_value(float mu1, float mu2, float e11, float e22, float edd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float dm = mu1 - mu2, sd = edd - dm * dm;
    const float A1 = 2.f * mu1 * mu2 + C1, B1 = mu1 * mu1 + mu2 * mu2 + C1;
    const float B2 = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2, A2 = B2 - sd;
    return (A1 * A2) / (B1 * B2);
}

// out[4] = psnr, ssim, l1, mse of one image from its sums (double) and its count
GS_HD void finish_values(double sum_abs, double sum_sq, double sum_s, int64_t n, float* out) {
    if (n <= 0) {
        for (int k = 0; k < 4; ++k) out[k] = __builtin_nanf("");
        return;
    }
    const double n3 = 3.0 * (double)n;                         // (divisions: an image against itself has ssim == 1.0 exactly)
    const double mse = sum_sq / n3;
    out[0] = mse > 0.0 ? (float)(-10.0 * log10(mse)) : __builtin_inff();
    out[1] = (float)(sum_s / n3);
    out[2] = (float)(sum_abs / n3);
    out[3] = (float)mse;
}

}  // namespace gsmet
