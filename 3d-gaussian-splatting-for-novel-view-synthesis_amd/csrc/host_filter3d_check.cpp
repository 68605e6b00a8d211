// host_filter3d_check.cpp -- host build of the per-row bodies in gs_filter3d.h, for CPU unit tests only (tests/test_filter3d_cpu.py).
//
// NOT part of the product path: the product library contains only HIP kernels and fails loudly without a GPU.  This file lets
// `pytest -m "not gpu"` check the filter's forward, its vector-Jacobian product and the sampling interval against the oracle
// (tests/filter3d_oracle.py) on a machine with no GPU.
#include "gs_filter3d.h"

using namespace gsf3;

extern "C" {

void hf3_apply(int64_t n, const float* scale_raw, const float* opacity_raw, const float* filt, float* scale_out, float* opacity_out) {
    for (int64_t i = 0; i < n; ++i) apply_row(scale_raw + i * 3, opacity_raw[i], filt[i], scale_out + i * 3, opacity_out[i]);
}

void hf3_apply_backward(int64_t n, const float* scale_raw, const float* opacity_raw, const float* filt, const float* g_scale_out,
                        const float* g_opacity_out, float* g_scale_raw, float* g_opacity_raw) {
    for (int64_t i = 0; i < n; ++i)
        apply_row_backward(scale_raw + i * 3, opacity_raw[i], filt[i], g_scale_out + i * 3, g_opacity_out[i], g_scale_raw + i * 3, g_opacity_raw[i]);
}

// what the two kernels compute, in their order: the minimum per row over the cameras, the maximum of those, the fill, sqrt(s)
void hf3_compute(int64_t n, const float* pos, int32_t n_cams, const float* cams, float near, float margin, float s, float* filt) {
    uint32_t top = 0u;
    for (int64_t i = 0; i < n; ++i) {
        const float* p = pos + i * 3;
        uint32_t best = UNSEEN;
        for (int32_t c = 0; c < n_cams; ++c) {
            float rec[STAGED_FLOATS];
            stage_camera(cams + (int64_t)c * CAMERA_FLOATS, near, margin, rec);
            const uint32_t b = camera_interval(rec, p[0], p[1], p[2]);
            best = b < best ? b : best;
        }
        if (!(finite_bits(p[0]) && finite_bits(p[1]) && finite_bits(p[2]))) best = UNSEEN;
        filt[i] = bits_float(best);
        if (best != UNSEEN && best > top) top = best;
    }
    const float sqrt_s = sqrtf(s);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t b = float_bits(filt[i]);
        filt[i] = sqrt_s * bits_float(b == UNSEEN ? top : b);
    }
}

}  // extern "C"
