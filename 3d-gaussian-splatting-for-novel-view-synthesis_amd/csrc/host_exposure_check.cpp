// host_exposure_check.cpp -- host build of the per-pixel bodies in gs_exposure.h, for CPU unit tests only (tests/test_exposure_cpu.py).
//
// NOT part of the product path: the product library contains only HIP kernels and fails loudly without a GPU.  This file lets
// `pytest -m "not gpu"` check the exposure transform, its two gradients and the identity's bit-exactness against the oracle
// (tests/exposure_oracle.py) on a machine with no GPU.
#include "gs_exposure.h"

using namespace gsexp;

extern "C" {

int32_t hexp_sum_depth() { return EXPOSURE_SUM_DEPTH; }
int32_t hexp_block_pixels() { return EXPOSURE_BLOCK_PIX; }

// image, out: [n, 3]; E: 12 floats
void hexp_forward(int64_t n, const float* image, const float* E, float* out) {
    for (int64_t i = 0; i < n; ++i) apply_pixel(E, image + i * 3, out + i * 3);
}

// g_image [n, 3] and g_params [12]: the sums in pixel order, in fp32 (the kernels' order differs; on dyadic inputs both are exact)
void hexp_backward(int64_t n, const float* image, const float* E, const float* g_out, float* g_image, float* g_params) {
    float s[EXPOSURE_PARAMS] = {0.f};
    for (int64_t i = 0; i < n; ++i) {
        backward_pixel(E, g_out + i * 3, g_image + i * 3);
        accumulate_pixel(image + i * 3, g_out + i * 3, s);
    }
    for (int k = 0; k < EXPOSURE_PARAMS; ++k) g_params[k] = s[k];
}

}  // extern "C"
