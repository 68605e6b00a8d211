// host_bilagrid_check.cpp -- host build of the per-pixel bodies in gs_bilagrid.h, for CPU unit tests only (tests/test_bilagrid_cpu.py).
//
// NOT part of the product path: the product library contains only HIP kernels and fails loudly without a GPU.  This file lets
// `pytest -m "not gpu"` check the slice, its two gradients, the total variation and the identity's bit-exactness against the oracle
// (tests/bilagrid_oracle.py) on a machine with no GPU.
#include "gs_bilagrid.h"

using namespace gsbila;

extern "C" {

int32_t hbila_sum_depth_fixed() { return BILAGRID_SUM_DEPTH_FIXED; }
int32_t hbila_wave_pixels() { return BILAGRID_WAVE_PIX; }
int32_t hbila_block_pixels() { return BILAGRID_BLOCK_PIX; }
int32_t hbila_level_group() { return BILAGRID_LEVEL_GROUP; }
int32_t hbila_stage_floats() { return BILAGRID_STAGE_FLOATS; }
int64_t hbila_gather_thread_pixels(int32_t H, int32_t W, int32_t X, int32_t Y) { return gather_thread_pixels(H, W, X, Y); }

// image, out: [H, W, 3]; G: [12, L, Y, X]
void hbila_forward(int32_t H, int32_t W, int32_t X, int32_t Y, int32_t L, const float* image, const float* G, float* out) {
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            const float* c = image + ((int64_t)i * W + j) * 3;
            float A[BILAGRID_CHANNELS];
            slice(G, X, Y, L, locate(i, j, H, W, X, Y, L, c), A, nullptr);
            apply_affine(A, c, out + ((int64_t)i * W + j) * 3);
        }
}

// g_image [H, W, 3] and g_G [12, L, Y, X]: every vertex walks the pixels of its support in row-major order and adds in fp32 (the
// kernel's walk by one thread instead of 512: the order differs; on dyadic inputs both are exact)
void hbila_backward(int32_t H, int32_t W, int32_t X, int32_t Y, int32_t L, const float* image, const float* G, const float* g_out,
                    float* g_image, float* g_G) {
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            const int64_t at = ((int64_t)i * W + j) * 3;
            const Cell q = locate(i, j, H, W, X, Y, L, image + at);
            float A[BILAGRID_CHANNELS], D[BILAGRID_CHANNELS];
            slice(G, X, Y, L, q, A, D);
            backward_pixel(A, D, q, L, image + at, g_out + at, g_image + at);
        }
    for (int gy = 0; gy < Y; ++gy)
        for (int gx = 0; gx < X; ++gx) {
            int ilo, ihi, jlo, jhi;
            support(gy, H, Y, ilo, ihi);
            support(gx, W, X, jlo, jhi);
            for (int l = 0; l < L; ++l) {
                float s[BILAGRID_CHANNELS] = {0.f};
                for (int i = ilo; i <= ihi; ++i)
                    for (int j = jlo; j <= jhi; ++j) {
                        const int64_t at = ((int64_t)i * W + j) * 3;
                        const Cell q = locate(i, j, H, W, X, Y, L, image + at);
                        const float w = axis_weight(gx, q.x0, q.fx) * axis_weight(gy, q.y0, q.fy) * axis_weight(l, q.z0, q.fz);
                        if (w == 0.f) continue;
                        float T[BILAGRID_CHANNELS];
                        outer(image + at, g_out + at, T);
                        for (int k = 0; k < BILAGRID_CHANNELS; ++k) s[k] = __builtin_fmaf(w, T[k], s[k]);
                    }
                for (int k = 0; k < BILAGRID_CHANNELS; ++k) g_G[(((int64_t)k * L + l) * Y + gy) * X + gx] = s[k];
            }
        }
}

// grids, grad: [V, 12, L, Y, X]; returns scale tv (the loss in element order, in double)
double hbila_tv(int64_t V, int32_t X, int32_t Y, int32_t L, float scale, const float* grids, float* grad) {
    const double per = 1.0 / ((double)V * BILAGRID_CHANNELS);
    const double c[3] = {per / ((double)(L - 1) * Y * X), per / ((double)L * (Y - 1) * X), per / ((double)L * Y * (X - 1))};
    const float k[3] = {(float)(2.0 * scale * c[0]), (float)(2.0 * scale * c[1]), (float)(2.0 * scale * c[2])};
    double loss = 0.0;
    const int64_t n = V * BILAGRID_CHANNELS * L * Y * X;
    for (int64_t e = 0; e < n; ++e)
        grad[e] = tv_element(grids + e, (int)(e % X), (int)(e / X % Y), (int)(e / ((int64_t)X * Y) % L), X, Y, L, k, c, &loss);
    return (double)scale * loss;
}

}  // extern "C"
