// host_pose_delta_selftest.cpp -- a stand-alone program over the host build of gs_pose_delta.h, for the sanitizer run of
// `make check-asan` (AddressSanitizer + UBSan on the CPU build; an instrumented program needs no preloaded runtime).  It walks every
// body over arrays sized exactly, so that an index out of range stops it, and checks the known properties on the way: the zero
// correction returns the pose as the same numbers, the composed rotation is orthonormal, either half of the backward alone has the
// bits of both together, the gradient of delta against central differences in double, and an active clamp stays finite.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_pose_delta_check.cpp"

static int fail(const char* what) { fprintf(stderr, "host_pose_delta_selftest: %s\n", what); return 1; }

// the forward in double, for the differences
static void compose(const double* c, const double* t, double* o) {
    double a1[3] = {t[3] + 1, t[4], t[5]}, a2[3] = {t[6], t[7] + 1, t[8]}, b1[3], b2[3], b3[3], u[3];
    const double n1 = std::fmax(std::sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), 1e-12);
    for (int k = 0; k < 3; ++k) b1[k] = a1[k] / n1;
    const double dot = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    for (int k = 0; k < 3; ++k) u[k] = a2[k] - dot * b1[k];
    const double n2 = std::fmax(std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), 1e-12);
    for (int k = 0; k < 3; ++k) b2[k] = u[k] / n2;
    b3[0] = b1[1] * b2[2] - b1[2] * b2[1]; b3[1] = b1[2] * b2[0] - b1[0] * b2[2]; b3[2] = b1[0] * b2[1] - b1[1] * b2[0];
    const double* D[3] = {b1, b2, b3};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = c[i * 4] * D[0][j] + c[i * 4 + 1] * D[1][j] + c[i * 4 + 2] * D[2][j];
        o[i * 4 + 3] = c[i * 4] * t[0] + c[i * 4 + 1] * t[1] + c[i * 4 + 2] * t[2] + c[i * 4 + 3];
    }
    for (int j = 0; j < 4; ++j) o[12 + j] = c[12 + j];
}

int main() {
    const int64_t n = 67;                                            // a wave and a ragged end
    std::vector<float> c(n * 16), d(n * 9), g(n * 16), o(n * 16), gc(n * 16), gd(n * 9), gc1(n * 16), gd1(n * 9), zero(n * 9, 0.f);
    uint32_t x = 4321u;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (float)((x >> 8) % 2001) / 1000.f - 1.f; };
    for (int64_t b = 0; b < n; ++b) {
        // a rotation from a random quaternion, a translation within [-10, 10]^3
        float q[4] = {rnd() + 1.5f, rnd(), rnd(), rnd()};
        const float qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        for (float& v : q) v /= qn;
        const float w = q[0], X = q[1], Y = q[2], Z = q[3];
        const float R[9] = {1 - 2 * (Y * Y + Z * Z), 2 * (X * Y - w * Z), 2 * (X * Z + w * Y), 2 * (X * Y + w * Z), 1 - 2 * (X * X + Z * Z),
                            2 * (Y * Z - w * X), 2 * (X * Z - w * Y), 2 * (Y * Z + w * X), 1 - 2 * (X * X + Y * Y)};
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) c[b * 16 + i * 4 + j] = R[i * 3 + j];
            c[b * 16 + i * 4 + 3] = 10.f * rnd();
        }
        c[b * 16 + 12] = c[b * 16 + 13] = c[b * 16 + 14] = 0.f; c[b * 16 + 15] = 1.f;
        for (int k = 0; k < 9; ++k) d[b * 9 + k] = 0.2f * rnd();
        for (int k = 0; k < 16; ++k) g[b * 16 + k] = rnd();
    }
    hpd_forward(n, c.data(), zero.data(), o.data());
    for (int64_t i = 0; i < n * 16; ++i)
        if (o[i] != c[i]) return fail("the zero correction changed a pose");
    hpd_forward(n, c.data(), d.data(), o.data());
    for (int64_t b = 0; b < n; ++b)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0.0;
                for (int k = 0; k < 3; ++k) s += (double)o[b * 16 + k * 4 + i] * o[b * 16 + k * 4 + j];
                if (std::fabs(s - (i == j)) > 1e-5) return fail("the composed rotation is not orthonormal");
            }
    hpd_backward(n, c.data(), d.data(), g.data(), gc.data(), gd.data());
    hpd_backward(n, c.data(), d.data(), g.data(), gc1.data(), nullptr);
    hpd_backward(n, c.data(), d.data(), g.data(), nullptr, gd1.data());
    if (memcmp(gc.data(), gc1.data(), (size_t)n * 64) || memcmp(gd.data(), gd1.data(), (size_t)n * 36)) return fail("a half alone differs from both together");
    for (int64_t b = 0; b < n; ++b) {
        double cd[16], td[9], gg[16], op[16], om[16];
        for (int k = 0; k < 16; ++k) { cd[k] = c[b * 16 + k]; gg[k] = g[b * 16 + k]; }
        for (int k = 0; k < 9; ++k) td[k] = d[b * 9 + k];
        for (int k = 0; k < 9; ++k) {
            const double h = 1e-6, keep = td[k];
            td[k] = keep + h; compose(cd, td, op);
            td[k] = keep - h; compose(cd, td, om);
            td[k] = keep;
            double want = 0.0;
            for (int e = 0; e < 16; ++e) want += gg[e] * (op[e] - om[e]) / (2 * h);
            if (std::fabs(gd[b * 9 + k] - want) > 2e-4) return fail("the gradient of delta against central differences");
        }
    }
    // p = (-1, 0, 0): a1 = 0, the first clamp is active
    for (int64_t b = 0; b < n; ++b) { d[b * 9 + 3] = -1.f; d[b * 9 + 4] = d[b * 9 + 5] = 0.f; }
    hpd_forward(n, c.data(), d.data(), o.data());
    hpd_backward(n, c.data(), d.data(), g.data(), gc.data(), gd.data());
    for (int64_t i = 0; i < n * 16; ++i)
        if (!std::isfinite(o[i]) || !std::isfinite(gc[i])) return fail("an active clamp gave a non-finite pose");
    for (int64_t i = 0; i < n * 9; ++i)
        if (!std::isfinite(gd[i])) return fail("an active clamp gave a non-finite gradient");
    if (hpd_params() != 9 || hpd_threads() != 64) return fail("the constants the tests read");
    printf("host_pose_delta_selftest ok\n");
    return 0;
}
