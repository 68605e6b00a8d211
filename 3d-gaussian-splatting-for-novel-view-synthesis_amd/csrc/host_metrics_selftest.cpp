// host_metrics_selftest.cpp -- a stand-alone program over the host build of gs_metrics.h, for the sanitizer run of `make check-asan`
// (AddressSanitizer + UBSan on the CPU build; an instrumented program needs no preloaded runtime).  It walks every body over arrays
// sized exactly, so that an index out of range stops it, and checks the known properties on the way: a planted affine comes back, a
// constant-colour image has the ridge's answer, S is exactly 1 for equal windows, and the PSNR edge cases.
#include <cmath>
#include <cstdio>
#include <vector>

#include "host_metrics_check.cpp"

static int fail(const char* what) { fprintf(stderr, "host_metrics_selftest: %s\n", what); return 1; }

int main() {
    const int64_t n = 1027;                                          // one workgroup's span and a ragged end
    std::vector<float> x(n * 3), y(n * 3), o(n * 3);
    std::vector<uint8_t> mask(n);
    uint32_t r = 12345u;
    const float E0[12] = {0.9f, 0.05f, -0.02f, 0.03f, 0.01f, 0.8f, 0.04f, 0.05f, 0.03f, 0.02f, 0.85f, 0.02f};
    for (int64_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) { r = r * 1664525u + 1013904223u; x[i * 3 + k] = (float)((r >> 8) % 1001) / 1000.f; }
        for (int k = 0; k < 3; ++k)
            y[i * 3 + k] = E0[k * 4] * x[i * 3] + E0[k * 4 + 1] * x[i * 3 + 1] + E0[k * 4 + 2] * x[i * 3 + 2] + E0[k * 4 + 3];
        r = r * 1664525u + 1013904223u; mask[i] = (uint8_t)((r >> 8) % 4 != 0);
    }
    double sums[21];
    float E[12], v[4];
    for (const uint8_t* m : {(const uint8_t*)nullptr, (const uint8_t*)mask.data()}) {
        const int64_t cnt = hmet_moments_of(n, x.data(), y.data(), m, sums);
        if (cnt < 1 || cnt > n) return fail("the count of valid pixels");
        hmet_solve(sums, cnt, E);
        for (int k = 0; k < 12; ++k)
            if (!(std::fabs(E[k] - E0[k]) < 1e-4)) return fail("a planted affine did not come back");
    }
    hmet_correct(n, x.data(), E, o.data());
    for (int64_t i = 0; i < n * 3; ++i)
        if (!(o[i] >= 0.f && o[i] <= 1.f) || std::fabs(o[i] - y[i]) > 1e-4) return fail("the corrected image");
    // a constant-colour image: A is singular without the ridge; with it M = I and t = y - x up to lambda
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { x[i * 3 + k] = 0.3f * (float)(k + 1); y[i * 3 + k] = 0.5f; }      // (no dyadic colour: its products round)
    hmet_solve(sums, hmet_moments_of(n, x.data(), y.data(), nullptr, sums), E);
    hmet_correct(n, x.data(), E, o.data());
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(E[k])) return fail("a constant-colour image has no finite answer");
    for (int64_t i = 0; i < n * 3; ++i)
        if (std::fabs(o[i] - 0.5f) > 1e-4) return fail("a constant-colour image is not mapped onto its target");
    hmet_solve(sums, 0, E);
    for (int k = 0; k < 12; ++k)
        if (!std::isnan(E[k])) return fail("no valid pixel must give NaN");
    // S: exactly 1 where the windows are equal, the textbook value elsewhere
    std::vector<float> mu(n), e(n), z(n, 0.f), S(n);
    for (int64_t i = 0; i < n; ++i) { r = r * 1664525u + 1013904223u; mu[i] = (float)((r >> 8) % 1001) / 1000.f; e[i] = mu[i] * mu[i] + 0.01f * mu[i]; }
    hmet_ssim_values(n, mu.data(), mu.data(), e.data(), e.data(), z.data(), S.data());
    for (int64_t i = 0; i < n; ++i)
        if (S[i] != 1.0f) return fail("S of equal windows is not exactly 1");
    {
        const float m1 = 0.4f, m2 = 0.6f, e11 = 0.2f, e22 = 0.41f, e12 = 0.25f, edd = e11 + e22 - 2.f * e12;
        hmet_ssim_values(1, &m1, &m2, &e11, &e22, &edd, S.data());
        const double s12 = (double)e12 - (double)m1 * m2, s11 = (double)e11 - (double)m1 * m1, s22 = (double)e22 - (double)m2 * m2;
        const double want = (2.0 * m1 * m2 + 1e-4) * (2.0 * s12 + 9e-4) / (((double)m1 * m1 + (double)m2 * m2 + 1e-4) * (s11 + s22 + 9e-4));
        if (std::fabs(S[0] - want) > 1e-5) return fail("S against the textbook formula");
    }
    // the PSNR edges
    hmet_finish(0.0, 0.0, 3.0 * 49, 49, v);
    if (!(std::isinf(v[0]) && v[0] > 0) || v[1] != 1.0f || v[2] != 0.f || v[3] != 0.f) return fail("an image against itself");
    hmet_finish(3.0, 0.03, 1.5, 10, v);
    if (std::fabs(v[0] - 30.0) > 1e-5 || std::fabs(v[1] - 0.05) > 1e-7 || std::fabs(v[2] - 0.1) > 1e-7 || std::fabs(v[3] - 1e-3) > 1e-9) return fail("known values");
    hmet_finish(1.0, 1.0, 1.0, 0, v);
    for (int k = 0; k < 4; ++k)
        if (!std::isnan(v[k])) return fail("no valid pixel must give NaN");
    if (hmet_moments() != 21 || hmet_row_words() != 22 || hmet_stats_row_words() != 4) return fail("the constants the tests read");
    printf("host_metrics_selftest ok\n");
    return 0;
}
