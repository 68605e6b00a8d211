// gs_mcmc.h -- per-row arithmetic of the MCMC density control: counter-based random numbers, the integer sampling
// weight, the relocation coefficient and the position noise.
//
// Product code in the style of gs_math.h: `GS_HD` bodies that the kernels of gsplat_mcmc.hip inline and that g++ compiles into a host
// test library (csrc/host_mcmc_check.cpp).  The host build is a TEST of this file, never a fallback.
//
// Not in the reference.  Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo" (2024); Salmon et al., "Parallel
// Random Numbers: As Easy as 1, 2, 3" (2011) for Philox4x32-10.
#pragma once
#include "gs_math.h"

namespace gsmc {

// ---- Philox4x32-10 ---------------------------------------------------------------------------------------------------------
constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;
enum : uint32_t { STREAM_NOISE = 0u, STREAM_RELOCATE = 1u };

GS_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four words of row `row` in iteration `iteration` of stream `stream`: key = the halves of the seed, counter = (row, iteration, stream)
GS_HD void row_random(uint64_t seed, int64_t row, uint32_t iteration, uint32_t stream, uint32_t out[4]) {
    const uint32_t ctr[4] = {(uint32_t)((uint64_t)row & 0xffffffffu), (uint32_t)((uint64_t)row >> 32), iteration, stream};
    const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
    philox4x32_10(ctr, key, out);
}

// the top 23 bits as the centre of their cell of (0, 1): exact in float32, never 0 or 1
GS_HD float unit_open(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// three standard normals from four words (Box-Muller; the second sine is not used)
GS_HD void normals3(const uint32_t x[4], float z[3]) {
    const float two_pi = 6.283185307179586f;
    const float r0 = sqrtf(-2.0f * logf(unit_open(x[0]))), a0 = two_pi * unit_open(x[1]);
    const float r1 = sqrtf(-2.0f * logf(unit_open(x[2]))), a1 = two_pi * unit_open(x[3]);
    z[0] = r0 * cosf(a0); z[1] = r0 * sinf(a0); z[2] = r1 * cosf(a1);
}

// ---- sampling weight -------------------------------------------------------------------------------------------------------
// 0 for a dead row, else the opacity in units of 2^-24, at least 1.  Dead is decided on the opacity the renderer sees: float32
// sigmoidf_ <= min_opacity (a NaN counts as dead).  The weight itself is taken from a double sigmoid: sigmoidf_ is good to ~2.5
// 2^-24 of its value, which above 1/2 is two units -- the weight would be two off where the double one is exact but for one value
// in 1e9 next to a step.
GS_HD uint32_t sample_weight(float opacity_raw, float min_opacity) {
    if (!(gsm::sigmoidf_(opacity_raw) > min_opacity)) return 0u;
    const double w = floor(16777216.0 / (1.0 + exp(-(double)opacity_raw)));
    return w < 1.0 ? 1u : (uint32_t)w;
}

GS_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// the row whose interval [prefix[j], prefix[j] + w_j) of the exclusive prefix sums holds t (0 <= t < total): the LAST j with
// prefix[j] <= t.  A row of weight 0 shares its prefix with its successor and is never the last one, and t < total rules out a
// dead tail.  n >= 1, prefix[0] = 0.
GS_HD int64_t search_prefix(const uint64_t* prefix, int64_t n, uint64_t t) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

GS_HD int64_t draw_source(const uint64_t* prefix, int64_t n, uint64_t total, uint64_t seed, int64_t row, uint32_t iteration) {
    uint32_t x[4];
    row_random(seed, row, iteration, STREAM_RELOCATE, x);
    const uint64_t r = ((uint64_t)x[0] << 32) | (uint64_t)x[1];
    return search_prefix(prefix, n, mulhi64(r, total));
}

// ---- relocation ------------------------------------------------------------------------------------------------------------
constexpr int RELOCATE_MAX_N = 51;

// A Gaussian of opacity o that becomes n Gaussians at the same place: each gets o' = 1 - (1 - o)^(1/n), so that the n of them
// composite to o, and its scales are multiplied by c = o / D,
//     D = sum_{i=1..n} sum_{k=0..i-1} C(i-1, k) (-1)^k o'^(k+1) / sqrt(k+1)  =  sum_{k=0..n-1} C(n, k+1) (-1)^k o'^(k+1) / sqrt(k+1)
// (sum_{i=k+1..n} C(i-1, k) = C(n, k+1): one loop of n terms instead of n (n + 1) / 2).  The sum alternates with terms up to
// ~(1 + o')^n / sqrt(n) -- 1e5 at n = 51 --, which float32 cannot hold: double, once per relocated row.  C(51, 25) < 2^48: the
// binomials are exact integers.  Returns o'' = clamp(o', min_opacity, 1 - 2^-24) and ln c.
// o itself is capped at 1 - 2^-24, the largest opacity below 1 that float32 holds: sigmoidf_ returns exactly 1 from a raw value
// of 16.7 on, and with o' = 1 the terms are the bare binomials -- 2.5e14 at n = 51, which double cannot cancel either.
GS_HD void relocation_coefficient(double o, int n, double min_opacity, double& o_new, double& ln_c) {
    if (n < 1) n = 1;
    if (n > RELOCATE_MAX_N) n = RELOCATE_MAX_N;
    if (o > 1.0 - 5.9604644775390625e-08) o = 1.0 - 5.9604644775390625e-08;
    const double op = (n == 1) ? o : -expm1(log1p(-o) / (double)n);
    double D = 0.0, p = 1.0;
    uint64_t binom = 1u;                                         // C(n, k)
    for (int k = 0; k < n; ++k) {
        binom = binom * (uint64_t)(n - k) / (uint64_t)(k + 1);   // C(n, k + 1): the product is C(n, k + 1) (k + 1), exact
        p *= op;
        const double term = (double)binom * p / sqrt((double)(k + 1));
        D += (k & 1) ? -term : term;
    }
    const double c = o / D;
    ln_c = (c > 0.0 && c < 1.0e300) ? log(c) : 0.0;              // (o = 0 or a NaN: leave the scale alone)
    const double hi = 1.0 - 5.9604644775390625e-08;
    o_new = op < min_opacity ? min_opacity : (op > hi ? hi : op);
    if (!(o_new == o_new)) o_new = min_opacity;
}

// what relocation writes: opacity_raw = logit(o''), scale_raw + ln c, each rounded once to float32
GS_HD void relocated_values(float opacity_raw_src, const float scale_raw_src[3], int n, float min_opacity, float& opacity_raw_new,
                            float scale_raw_new[3]) {
    double o_new, ln_c;
    relocation_coefficient((double)gsm::sigmoidf_(opacity_raw_src), n, (double)min_opacity, o_new, ln_c);
    opacity_raw_new = (float)log(o_new / (1.0 - o_new));
    for (int k = 0; k < 3; ++k) scale_raw_new[k] = (float)((double)scale_raw_src[k] + ln_c);
}

// ---- position noise --------------------------------------------------------------------------------------------------------
// g = 1 / (1 + exp(100 sigmoid(opacity_raw) - 0.5)): the logistic of 1 - opacity with k = 100, x0 = 0.995.  From an opacity of 0.893
// on the exponential is +inf in float32 and g exactly 0.
GS_HD float noise_gate(float opacity_raw) { return 1.0f / (1.0f + expf(100.0f * gsm::sigmoidf_(opacity_raw) - 0.5f)); }

// d = Sigma (z a g) with the project's own covariance (its clamp of the scales, its normalisation of q_raw).  Returns false --
// and d = 0 -- where g is 0: the caller leaves the row alone, so an infinite covariance times zero never becomes a NaN.
GS_HD bool noise_displacement(const float scale_raw[3], const float q_raw[4], float opacity_raw, const float z[3], float a, float d[3]) {
    const float g = noise_gate(opacity_raw);
    d[0] = d[1] = d[2] = 0.f;
    if (!(g > 0.f)) return false;
    float S[6];
    gsm::CovMid mid;
    gsm::cov_from_params(scale_raw, q_raw, S, mid);
    const float v0 = z[0] * a * g, v1 = z[1] * a * g, v2 = z[2] * a * g;
    d[0] = S[0] * v0 + S[1] * v1 + S[2] * v2;
    d[1] = S[1] * v0 + S[3] * v1 + S[4] * v2;
    d[2] = S[2] * v0 + S[4] * v1 + S[5] * v2;
    return true;
}

// ---- regularisers ----------------------------------------------------------------------------------------------------------
// sigmoid (1 - sigmoid) without the cancellation of 1 - sigmoid near 1: e / (1 + e)^2, e = exp(-|x|)
GS_HD float sigmoid_slope(float x) { const float e = expf(-fabsf(x)); return e / ((1.0f + e) * (1.0f + e)); }

}  // namespace gsmc
