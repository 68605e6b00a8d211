// host_knn_selftest.cpp -- a stand-alone program over the host build of gs_knn.h, for the sanitizer run of `make check-asan-knn`
// (AddressSanitizer + UBSan on the CPU build; an instrumented program needs no preloaded runtime).  It walks every body over arrays
// sized exactly, so that an index out of range stops it, and checks the known properties on the way: the key's order and its edge
// cases, the box distance never above the point distance, the insert against a sort, and the brute force on small known clouds.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_knn_check.cpp"

static int fail(const char* what) { fprintf(stderr, "host_knn_selftest: %s\n", what); return 1; }

static uint32_t rng_state = 12345u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)(rng_state >> 8) * (1.0f / 16777216.0f); }

int main() {
    // keys: monotone per axis, zero extent -> 0, an extent that overflows -> no NaN and still monotone, the top key reserved
    {
        uint32_t prev = 0u;
        for (int k = 0; k <= 1000; ++k) {
            const uint32_t q = hknn_key_axis(-3.f + 0.007f * (float)k, -3.f, 4.f);
            if (q < prev || q > KEY_MAX_AXIS) return fail("key_axis is not monotone");
            prev = q;
        }
        if (hknn_key_axis(-3.f, -3.f, 4.f) != 0u || hknn_key_axis(4.f, -3.f, 4.f) != KEY_MAX_AXIS) return fail("key_axis ends");
        if (hknn_key_axis(2.f, 2.f, 2.f) != 0u) return fail("zero extent");
        const float big = 3e38f;
        if (hknn_key_axis(-big, -big, big) != 0u || hknn_key_axis(big, -big, big) != KEY_MAX_AXIS) return fail("infinite extent: ends");
        const uint32_t mid = hknn_key_axis(0.f, -big, big);
        if (mid < KEY_MAX_AXIS / 2 - 1 || mid > KEY_MAX_AXIS / 2 + 1) return fail("infinite extent: middle");
        const float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {1.f, 1.f, 1.f}, one[3] = {1.f, 1.f, 1.f}, bad[3] = {0.5f, NAN, 0.5f}, inf[3] = {INFINITY, 0.f, 0.f};
        if (hknn_key(one, lo, hi) != 0x7fffffffffffffffull) return fail("the largest finite key is not 2^63 - 1");
        if (hknn_key(bad, lo, hi) != KEY_NONFINITE || hknn_key(inf, lo, hi) != KEY_NONFINITE) return fail("non-finite rows");
        const float x1[3] = {1.f, 0.f, 0.f}, y1[3] = {0.f, 1.f, 0.f}, z1[3] = {0.f, 0.f, 1.f};
        if (hknn_key(x1, lo, hi) != 0x1249249249249249ull || hknn_key(y1, lo, hi) != 0x2492492492492492ull ||
            hknn_key(z1, lo, hi) != 0x4924924924924924ull) return fail("bit interleave");
    }
    // the box distance: <= the distance to every point inside, for queries outside, on the faces and inside
    for (int t = 0; t < 20000; ++t) {
        float lo[3], hi[3], p[3], q[3];
        for (int a = 0; a < 3; ++a) {
            const float u = 4.f * rnd() - 2.f, v = 4.f * rnd() - 2.f;
            lo[a] = u < v ? u : v; hi[a] = u < v ? v : u;
            p[a] = lo[a] + (hi[a] - lo[a]) * rnd();
            p[a] = p[a] < lo[a] ? lo[a] : (p[a] > hi[a] ? hi[a] : p[a]);
            const int mode = t % 4;
            q[a] = mode == 0 ? 6.f * rnd() - 3.f : mode == 1 ? (rnd() < 0.5f ? lo[a] : hi[a]) : mode == 2 ? p[a] : lo[a] + (hi[a] - lo[a]) * rnd();
        }
        if (!(hknn_dist2_box(q, lo, hi) <= hknn_dist2(q, p))) return fail("the box is farther than a point inside it");
        if (hknn_dist2(q, p) != hknn_dist2(p, q)) return fail("d2 is not symmetric");
    }
    // insert3 against a sort, with ties
    for (int t = 0; t < 200; ++t) {
        const int n = t % 9;
        std::vector<float> d((size_t)n);
        for (float& x : d) x = (float)((int)(rnd() * 6.f));
        float best[3];
        hknn_insert3(n, d.data(), best);
        std::sort(d.begin(), d.end());
        for (int k = 0; k < 3; ++k)
            if (best[k] != (k < n ? d[(size_t)k] : INFINITY)) return fail("insert3");
    }
    // the brute force: the corners of a unit square, a duplicate, non-finite rows, and the small sizes
    {
        const float pts[7 * 3] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 1.f, 1.f, 0.f, NAN, 0.f, 0.f, 0.f, INFINITY, 0.f, 0.f, 0.f, 0.f};
        std::vector<float> out(7);
        hknn_mean_dist2(4, pts, out.data());
        const float want4 = ((1.f + 1.f) + 2.f) * 0.333333343f;
        for (int k = 0; k < 4; ++k) if (memcmp(&out[(size_t)k], &want4, 4)) return fail("unit square");
        hknn_mean_dist2(7, pts, out.data());
        if (out[4] != 0.f || out[5] != 0.f) return fail("a non-finite row is not 0");
        const float dup = ((0.f + 1.f) + 1.f) * 0.333333343f;
        if (memcmp(&out[0], &dup, 4) || memcmp(&out[6], &dup, 4)) return fail("a duplicate is not a neighbour at distance 0");
        hknn_mean_dist2(1, pts, out.data());
        if (out[0] != 0.f) return fail("one point");
        hknn_mean_dist2(2, pts, out.data());
        if (out[0] != 1.f || out[1] != 1.f) return fail("two points");
        hknn_mean_dist2(3, pts, out.data());
        if (out[0] != 1.f || out[1] != 1.5f || out[2] != 1.5f) return fail("three points");
        hknn_mean_dist2(2, pts + 4 * 3, out.data());
        if (out[0] != 0.f || out[1] != 0.f) return fail("no finite row");
        hknn_mean_dist2(0, pts, out.data());
    }
    // a random cloud against a plain sort of all distances
    {
        const int n = 300;
        std::vector<float> p((size_t)n * 3), out((size_t)n);
        for (float& x : p) x = rnd();
        hknn_mean_dist2(n, p.data(), out.data());
        for (int i = 0; i < n; ++i) {
            std::vector<float> d;
            for (int j = 0; j < n; ++j) if (j != i) d.push_back(hknn_dist2(&p[(size_t)i * 3], &p[(size_t)j * 3]));
            std::sort(d.begin(), d.end());
            const float want = hknn_mean_smallest(d[0], d[1], d[2], n - 1);
            if (memcmp(&out[(size_t)i], &want, 4)) return fail("random cloud");
        }
    }
    printf("host_knn_selftest ok\n");
    return 0;
}
