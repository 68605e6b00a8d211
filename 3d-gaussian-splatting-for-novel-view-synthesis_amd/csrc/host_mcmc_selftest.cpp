// host_mcmc_selftest.cpp -- a stand-alone program over the host build of gs_mcmc.h, for the sanitizer run of `make check-asan`
// (AddressSanitizer + UBSan on the CPU build; an instrumented program needs no preloaded runtime).  It walks every body over small
// arrays sized exactly, so that an index out of range or an undefined shift stops it, and checks the known answers on the way.
#include <cstdio>
#include <vector>

#include "host_mcmc_check.cpp"

static int fail(const char* what) { fprintf(stderr, "host_mcmc_selftest: %s\n", what); return 1; }

int main() {
    const uint32_t ctr[12] = {0, 0, 0, 0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u};
    const uint32_t key[6] = {0, 0, 0xffffffffu, 0xffffffffu, 0xa4093822u, 0x299f31d0u};
    const uint32_t want[12] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u, 0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu,
                               0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u};
    uint32_t out[12];
    hmc_philox(3, ctr, key, out);
    for (int k = 0; k < 12; ++k) if (out[k] != want[k]) return fail("Philox known answer");

    const int64_t n = 1000;
    std::vector<uint32_t> words(n * 4), w(n);
    std::vector<float> u(n * 4), z(n * 3), raw(n), sr(n * 3), q(n * 4), d(n * 3);
    std::vector<int32_t> moved(n), src(n), count(n);
    std::vector<uint64_t> prefix(n);
    hmc_row_random(0xDEADBEEFCAFEF00Dull, (int64_t(1) << 32) - 500, n, 0xffffffffu, 1u, words.data(), u.data(), z.data());
    for (int64_t i = 0; i < n * 4; ++i) if (!(u[i] > 0.f && u[i] < 1.f)) return fail("uniform outside (0, 1)");
    for (int64_t i = 0; i < n; ++i) {
        raw[i] = (i % 10 == 0) ? -20.f : (i % 97 == 0 ? 80.f : -6.f + 0.02f * (float)i);
        for (int k = 0; k < 3; ++k) sr[i * 3 + k] = -5.f + 0.001f * (float)(i + k);
        for (int k = 0; k < 4; ++k) q[i * 4 + k] = z[(i * 3 + k) % (n * 3)];
    }
    raw[1] = -80.f; raw[2] = NAN;
    hmc_weights(n, raw.data(), 0.005f, w.data());
    if (w[0] != 0u || w[1] != 0u || w[2] != 0u || w[97] != 16777216u) return fail("weight");
    const uint64_t total = hmc_draw(n, w.data(), 7u, 3u, prefix.data(), src.data(), count.data());
    int64_t drawn = 0, dead = 0;
    for (int64_t i = 0; i < n; ++i) {
        dead += w[i] == 0u; drawn += count[i];
        if ((w[i] == 0u) != (src[i] >= 0)) return fail("a live row drew, or a dead one did not");
        if (src[i] >= 0 && !(w[src[i]] > 0u && prefix[src[i]] < total)) return fail("a dead source");
    }
    if (drawn != dead) return fail("draw count");
    std::fill(w.begin(), w.end(), 0u);
    if (hmc_draw(n, w.data(), 7u, 3u, prefix.data(), src.data(), count.data()) != 0u) return fail("total of no weights");
    const float sigmas[5] = {0.0051f, 0.05f, 0.5f, 0.99f, 1.0f - 5.9604644775390625e-08f};
    for (float s : sigmas)
        for (int k = -2; k <= 60; ++k) {
            double o_new, ln_c;
            hmc_relocation_coefficient((double)s, k, 0.005, &o_new, &ln_c);
            if (!(o_new >= 0.005 && o_new < 1.0 && ln_c <= 1e-12 && ln_c > -2.0)) return fail("relocation coefficient out of range");
            float o_raw, s_new[3];
            hmc_relocated_values(logf(s / (1.0f - s)), sr.data(), k, 0.005f, &o_raw, s_new);
            if (!(o_raw == o_raw)) return fail("relocated opacity is a NaN");
        }
    double o_new, ln_c;
    hmc_relocation_coefficient(0.5, 2, 0.005, &o_new, &ln_c);
    if (fabs(exp(ln_c) - 0.952152) > 1e-6) return fail("c(0.5, 2)");
    hmc_relocation_coefficient(1.0, 51, 0.005, &o_new, &ln_c);               // a float32 sigmoid of exactly 1: capped, not 2.5e14-term noise
    if (fabs(exp(ln_c) - 0.501431) > 1e-6 || fabs(o_new - 0.278330) > 1e-6) return fail("c(1, 51)");
    hmc_noise(n, raw.data(), sr.data(), q.data(), 80.f, 9u, 77u, d.data(), moved.data());
    for (int64_t i = 0; i < n * 3; ++i) if (!(d[i] == d[i])) return fail("noise is a NaN");
    if (moved[97] || !moved[1]) return fail("noise gate");
    printf("host_mcmc_selftest ok\n");
    return 0;
}
