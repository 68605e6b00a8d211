// host_knn_check.cpp -- host build of the bodies in gs_knn.h, for CPU unit tests only (tests/test_knn_oracle_cpu.py) and as the
// bit-for-bit reference of the device result (tests/test_gpu_knn.py).  Built with -ffp-contract=off.
//
// NOT part of the product path: the product library contains only HIP kernels and fails loudly without a GPU.  hknn_mean_dist2 is the
// definition in gs_knn.h evaluated by brute force, O(N^2), with the same d2, the same insert and the same mean as the kernels.
#include "gs_knn.h"

using namespace gsknn;

extern "C" {

float hknn_dist2(const float* a, const float* b) { return dist2_points(a[0], a[1], a[2], b[0], b[1], b[2]); }

float hknn_dist2_box(const float* q, const float* lo, const float* hi) { return dist2_box(q[0], q[1], q[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]); }

uint32_t hknn_key_axis(float x, float lo, float hi) { return key_axis(x, lo, hi); }

uint64_t hknn_key(const float* p, const float* lo, const float* hi) { return morton_key(p[0], p[1], p[2], lo, hi); }

uint64_t hknn_key_nonfinite(void) { return KEY_NONFINITE; }

// best[3] (ascending, +inf where empty) after the n values of d have gone through insert3
void hknn_insert3(int64_t n, const float* d, float* best) {
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    for (int64_t i = 0; i < n; ++i) insert3(b0, b1, b2, d[i]);
    best[0] = b0; best[1] = b1; best[2] = b2;
}

float hknn_mean_smallest(float b0, float b1, float b2, int64_t others) { return mean_smallest(b0, b1, b2, others); }

void hknn_mean_dist2(int64_t n, const float* points, float* dist2) {
    int64_t finite = 0;
    for (int64_t i = 0; i < n; ++i) finite += finite_row(points[i * 3], points[i * 3 + 1], points[i * 3 + 2]) ? 1 : 0;
    for (int64_t i = 0; i < n; ++i) {
        const float* p = points + i * 3;
        dist2[i] = 0.f;
        if (!finite_row(p[0], p[1], p[2])) continue;
        float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
        for (int64_t j = 0; j < n; ++j) {
            const float* c = points + j * 3;
            if (j == i || !finite_row(c[0], c[1], c[2])) continue;
            insert3(b0, b1, b2, dist2_points(p[0], p[1], p[2], c[0], c[1], c[2]));
        }
        dist2[i] = mean_smallest(b0, b1, b2, finite - 1);
    }
}

}  // extern "C"
