// host_bilagrid_selftest.cpp -- a stand-alone program over the host build of gs_bilagrid.h, for the sanitizer run of `make check-asan`
// (AddressSanitizer + UBSan on the CPU build; an instrumented program needs no preloaded runtime).  It walks every body over arrays
// sized exactly, so that an index out of range stops it, and checks the known properties on the way: the identity bit for bit in
// both directions, the total variation of the identity, the sum of the grid gradient against the sum of g_o (x) [c, 1] (the eight
// weights of a pixel add up to one), and the slice of a grid that is affine in (x, y) against double.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_bilagrid_check.cpp"

static int fail(const char* what) { fprintf(stderr, "host_bilagrid_selftest: %s\n", what); return 1; }

static int run(int H, int W, int X, int Y, int L) {
    const int64_t n = (int64_t)H * W, cells = (int64_t)L * Y * X;
    std::vector<float> c(n * 3), go(n * 3), o(n * 3), gc(n * 3), G(12 * cells), gG(12 * cells), gtv(12 * cells);
    uint32_t x = 12345u;
    for (int64_t i = 0; i < n * 3; ++i) {                            // c in [-0.25, 1.25]: black, white and beyond are all met
        x = x * 1664525u + 1013904223u; c[i] = (float)((x >> 8) % 13) / 8.f - 0.25f;
        x = x * 1664525u + 1013904223u; go[i] = ((float)((x >> 8) % 129) - 64.f) / 64.f;
    }
    for (int ch = 0; ch < 12; ++ch)
        for (int64_t k = 0; k < cells; ++k) G[ch * cells + k] = (ch % 5 == 0) ? 1.f : 0.f;
    hbila_forward(H, W, X, Y, L, c.data(), G.data(), o.data());
    hbila_backward(H, W, X, Y, L, c.data(), G.data(), go.data(), gc.data(), gG.data());
    if (memcmp(o.data(), c.data(), (size_t)n * 12)) return fail("the identity changed a colour");
    for (int64_t i = 0; i < n * 3; ++i)
        if (gc[i] != go[i]) return fail("the identity changed a gradient");
    if (hbila_tv(1, X, Y, L, 10.f, G.data(), gtv.data()) != 0.0) return fail("the total variation of the identity is not 0");
    for (int64_t k = 0; k < 12 * cells; ++k)
        if (gtv[k] != 0.f) return fail("the TV gradient of the identity is not 0");
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 4; ++k) {
            double want = 0.0, got = 0.0, mag = 0.0;
            for (int64_t i = 0; i < n; ++i) {
                const double t = (double)go[i * 3 + r] * (k < 3 ? (double)c[i * 3 + k] : 1.0);
                want += t; mag += std::fabs(t);
            }
            for (int64_t q = 0; q < cells; ++q) got += gG[(r * 4 + k) * cells + q];
            if (std::fabs(got - want) > 1e-5 * (mag + 1.0)) return fail("the grid gradient does not add up to the sum of g_o (x) [c, 1]");
        }
    // a grid affine in (x, y), constant in z: trilinear interpolation reproduces it at every pixel
    for (int ch = 0; ch < 12; ++ch)
        for (int l = 0; l < L; ++l)
            for (int y = 0; y < Y; ++y)
                for (int xx = 0; xx < X; ++xx) G[((ch * L + l) * Y + y) * X + xx] = 0.125f * ch + 0.25f * xx - 0.5f * y;
    hbila_forward(H, W, X, Y, L, c.data(), G.data(), o.data());
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j)
            for (int r = 0; r < 3; ++r) {
                const double u = (j + 0.5) / W * (X - 1), v = (i + 0.5) / H * (Y - 1);
                const float* p = c.data() + ((int64_t)i * W + j) * 3;
                double want = 0.125 * (4 * r + 3) + 0.25 * u - 0.5 * v;
                for (int k = 0; k < 3; ++k) want += (0.125 * (4 * r + k) + 0.25 * u - 0.5 * v) * p[k];
                if (std::fabs(o[((int64_t)i * W + j) * 3 + r] - want) > 1e-3) return fail("known answer");
            }
    return 0;
}

int main() {
    if (run(1, 1, 2, 2, 2) || run(5, 7, 16, 16, 8) || run(37, 29, 3, 5, 4) || run(23, 41, 64, 2, 16)) return 1;
    if (hbila_sum_depth_fixed() != 13 || hbila_block_pixels() != 256 || hbila_wave_pixels() != 64 || hbila_level_group() != 8)
        return fail("the constants the tests read");
    printf("host_bilagrid_selftest ok\n");
    return 0;
}
