// host_pose_delta_check.cpp -- host build of the per-view bodies in gs_pose_delta.h, for CPU unit tests only
// (tests/test_pose_delta_cpu.py).
//
// NOT part of the product path: the product library contains only HIP kernels and fails loudly without a GPU.  This file lets
// `pytest -m "not gpu"` check the composition, its two gradients, the identity's exactness and the clamps against the oracle
// (tests/pose_delta_oracle.py) on a machine with no GPU.
#include "gs_pose_delta.h"

using namespace gspd;

extern "C" {

int32_t hpd_params() { return POSE_DELTA_PARAMS; }
int32_t hpd_threads() { return POSE_DELTA_THREADS; }

// c2w, out: [n, 16]; delta: [n, 9]
void hpd_forward(int64_t n, const float* c2w, const float* delta, float* out) {
    for (int64_t b = 0; b < n; ++b) pose_delta_forward_view(c2w + b * 16, delta + b * POSE_DELTA_PARAMS, out + b * 16);
}

// g_c2w [n, 16] and g_delta [n, 9], either NULL: not formed
void hpd_backward(int64_t n, const float* c2w, const float* delta, const float* g_out, float* g_c2w, float* g_delta) {
    for (int64_t b = 0; b < n; ++b)
        pose_delta_backward_view(c2w + b * 16, delta + b * POSE_DELTA_PARAMS, g_out + b * 16, g_c2w ? g_c2w + b * 16 : nullptr,
                                 g_delta ? g_delta + b * POSE_DELTA_PARAMS : nullptr);
}

}  // extern "C"
