// host_metrics_check.cpp -- host build of the per-pixel and per-image bodies in gs_metrics.h, for CPU unit tests only
// (tests/test_metrics_cpu.py).
//
// NOT part of the product path: the product library contains only HIP kernels and fails loudly without a GPU.  This file lets
// `pytest -m "not gpu"` check the solve of the colour correction, the SSIM value and the PSNR edge cases against the oracle
// (tests/metrics_oracle.py) on a machine with no GPU.
#include "gs_metrics.h"

using namespace gsmet;

extern "C" {

int32_t hmet_moments() { return METRICS_MOMENTS; }
int32_t hmet_row_words() { return METRICS_ROW; }
int32_t hmet_stats_row_words() { return METRICS_STATS_ROW; }
double hmet_ridge() { return METRICS_RIDGE; }

// pred, target: [n, 3]; mask: n bytes or NULL.  sums[21], in pixel order (the kernels' order differs); returns the count.
int64_t hmet_moments_of(int64_t n, const float* pred, const float* target, const uint8_t* mask, double* sums) {
    for (int k = 0; k < METRICS_MOMENTS; ++k) sums[k] = 0.0;
    int64_t cnt = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (mask && !mask[i]) continue;
        accumulate_moments(pred + i * 3, target + i * 3, sums);
        ++cnt;
    }
    return cnt;
}

void hmet_solve(const double* sums, int64_t n, float* affine) { solve_affine(sums, n, affine); }

// image, out: [n, 3]; E: 12 floats
void hmet_correct(int64_t n, const float* image, const float* E, float* out) {
    for (int64_t i = 0; i < n; ++i) correct_pixel(E, image + i * 3, out + i * 3);
}

// five arrays of n windowed sums -> n SSIM values
void hmet_ssim_values(int64_t n, const float* mu1, const float* mu2, const float* e11, const float* e22, const float* edd, float* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = ssim_value(mu1[i], mu2[i], e11[i], e22[i], edd[i]);
}

void hmet_finish(double sum_abs, double sum_sq, double sum_s, int64_t n, float* out) { finish_values(sum_abs, sum_sq, sum_s, n, out); }

}  // extern "C"
