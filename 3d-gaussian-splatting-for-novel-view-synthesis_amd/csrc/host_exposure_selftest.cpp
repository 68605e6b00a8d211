// host_exposure_selftest.cpp -- a stand-alone program over the host build of gs_exposure.h, for the sanitizer run of `make check-asan`
// (AddressSanitizer + UBSan on the CPU build; an instrumented program needs no preloaded runtime).  It walks every body over arrays
// sized exactly, so that an index out of range stops it, and checks the known properties on the way: the identity bit for bit in
// both directions, the sums of a dyadic frame exactly, and one transform against double.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_exposure_check.cpp"

static int fail(const char* what) { fprintf(stderr, "host_exposure_selftest: %s\n", what); return 1; }

int main() {
    const int64_t n = 1027;                                          // one workgroup's span and a ragged end
    std::vector<float> c(n * 3), go(n * 3), o(n * 3), gc(n * 3);
    uint32_t x = 12345u;
    for (int64_t i = 0; i < n * 3; ++i) {                            // dyadic: c in eighths of [0, 1], g_o in 64ths of [-1, 1]
        x = x * 1664525u + 1013904223u; c[i] = (float)((x >> 8) % 9) / 8.f;
        x = x * 1664525u + 1013904223u; go[i] = ((float)((x >> 8) % 129) - 64.f) / 64.f;
    }
    const float I[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    float gp[12];
    hexp_forward(n, c.data(), I, o.data());
    hexp_backward(n, c.data(), I, go.data(), gc.data(), gp);
    if (memcmp(o.data(), c.data(), (size_t)n * 12)) return fail("the identity changed a colour");
    for (int64_t i = 0; i < n * 3; ++i)
        if (gc[i] != go[i]) return fail("the identity changed a gradient");
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) {
            double want = 0.0;
            for (int64_t i = 0; i < n; ++i) want += (double)go[i * 3 + r] * (k < 3 ? (double)c[i * 3 + k] : 1.0);
            if ((double)gp[r * 4 + k] != want) return fail("a sum over a dyadic frame is not exact");
        }
    const float E[12] = {1.1f, -0.05f, 0.02f, 0.01f, 0.03f, 0.9f, -0.04f, -0.02f, 0.f, 0.07f, 1.2f, 0.05f};
    hexp_forward(n, c.data(), E, o.data());
    hexp_backward(n, c.data(), E, go.data(), gc.data(), gp);
    for (int64_t i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) {
            double want = E[r * 4 + 3], back = 0.0;
            for (int k = 0; k < 3; ++k) { want += (double)E[r * 4 + k] * c[i * 3 + k]; back += (double)E[k * 4 + r] * go[i * 3 + k]; }
            if (std::fabs(o[i * 3 + r] - want) > 1e-6 || std::fabs(gc[i * 3 + r] - back) > 1e-6) return fail("known answer");
        }
    if (hexp_sum_depth() != 12 || hexp_block_pixels() != 1024) return fail("the constants the tests read");
    printf("host_exposure_selftest ok\n");
    return 0;
}
