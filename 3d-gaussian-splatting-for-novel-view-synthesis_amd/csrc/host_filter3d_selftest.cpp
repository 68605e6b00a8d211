// host_filter3d_selftest.cpp -- a stand-alone program over the host build of gs_filter3d.h, for the sanitizer run of `make check-asan`
// (AddressSanitizer + UBSan on the CPU build; an instrumented program needs no preloaded runtime).  It walks every body over arrays
// sized exactly, so that an index out of range stops it, and checks the known properties on the way: the f == 0 identity bit for
// bit, finite results on the extreme inputs, and a few values against double.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_filter3d_check.cpp"

static int fail(const char* what) { fprintf(stderr, "host_filter3d_selftest: %s\n", what); return 1; }

int main() {
    const float scales[] = {-20.f, -14.f, -13.f, -5.f, 0.f, 3.f, 20.f, 80.f}, opacities[] = {-100.f, -12.f, -1.f, 0.f, 1.f, 12.f, 30.f, 100.f};
    const float filts[] = {0.f, 1e-30f, 1e-6f, 1e-3f, 0.1f, 1.f, 10.f, 1e30f};
    std::vector<float> sr, o, f;
    for (float a : scales) for (float b : scales) for (float x : opacities) for (float y : filts) {
        sr.push_back(a); sr.push_back(b); sr.push_back(0.5f * (a + b)); o.push_back(x); f.push_back(y);
    }
    const int64_t n = (int64_t)o.size();
    std::vector<float> so(n * 3), oo(n), gs(n * 3), go(n), ds(n * 3), dq(n);
    for (int64_t i = 0; i < n; ++i) { go[i] = (i % 3 == 0) ? -1.5f : 0.75f; for (int k = 0; k < 3; ++k) gs[i * 3 + k] = 0.25f * (float)(k + 1) - 0.4f; }
    hf3_apply(n, sr.data(), o.data(), f.data(), so.data(), oo.data());
    hf3_apply_backward(n, sr.data(), o.data(), f.data(), gs.data(), go.data(), ds.data(), dq.data());
    for (int64_t i = 0; i < n; ++i) {
        if (f[i] == 0.f) {
            if (memcmp(&so[i * 3], &sr[i * 3], 12) || memcmp(&oo[i], &o[i], 4)) return fail("f == 0 is not the identity");
            if (memcmp(&ds[i * 3], &gs[i * 3], 12) || memcmp(&dq[i], &go[i], 4)) return fail("f == 0: the backward is not the identity");
        }
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(so[i * 3 + k]) || !std::isfinite(ds[i * 3 + k])) return fail("a scale or its gradient is not finite");
        if (!std::isfinite(oo[i]) || !std::isfinite(dq[i])) return fail("an opacity or its gradient is not finite");
        if (!(oo[i] <= o[i] + 1e-5f * (1.f + fabsf(o[i])))) return fail("the filter raised an opacity");
    }
    {   // s = (1, 1, 1), f = 1, o = 0: scale' = log sqrt 2, c = 2^-1.5, opacity' = logit(c / 2)
        const float s1[3] = {0.f, 0.f, 0.f};
        float s2[3], o2;
        apply_row(s1, 0.f, 1.f, s2, o2);
        const double c = pow(2.0, -1.5), want = log(0.5 * c / (1.0 - 0.5 * c));
        if (fabs(s2[0] - 0.5 * log(2.0)) > 1e-6 || fabs(o2 - want) > 1e-6) return fail("known answer");
    }
    // the sampling interval: one camera at the origin looking down +z, 100 x 80 pixels, focal 50 / 40
    float cam[2 * CAMERA_FLOATS] = {0};
    for (int c = 0; c < 2; ++c) {
        float* r = cam + c * CAMERA_FLOATS;
        r[0] = r[5] = r[10] = 1.f; r[12] = 50.f; r[13] = 40.f; r[14] = 50.f; r[15] = 40.f; r[16] = 100.f; r[17] = 80.f;
    }
    cam[CAMERA_FLOATS + 11] = -2.f;                                   // the second camera two units behind the first
    cam[CAMERA_FLOATS + 12] = 25.f; cam[CAMERA_FLOATS + 13] = 20.f;
    const float pos[6 * 3] = {0.f, 0.f, 5.f, 0.f, 0.f, 0.1f, 100.f, 0.f, 5.f, NAN, 0.f, 5.f, 0.f, 0.f, INFINITY, 0.f, 0.f, -3.f};
    float filt[6];
    hf3_compute(6, pos, 2, cam, 0.2f, 0.15f, 0.25f, filt);
    if (fabsf(filt[0] - 0.5f * 5.f / 50.f) > 1e-7f) return fail("interval of a point both cameras see");
    if (fabsf(filt[1] - 0.5f * 2.1f / 25.f) > 1e-7f) return fail("interval of a point only the far camera sees");
    const float top = filt[0] > filt[1] ? filt[0] : filt[1];
    for (int k = 2; k < 6; ++k) if (memcmp(&filt[k], &top, 4)) return fail("an unseen row is not the maximum");
    hf3_compute(6, pos, 0, cam, 0.2f, 0.15f, 0.25f, filt);
    for (int k = 0; k < 6; ++k) if (filt[k] != 0.f) return fail("no camera: not zero");
    hf3_compute(4, pos + 6, 2, cam, 0.2f, 0.15f, 0.25f, filt);
    for (int k = 0; k < 4; ++k) if (filt[k] != 0.f) return fail("nobody seen: not zero");
    printf("host_filter3d_selftest ok\n");
    return 0;
}
