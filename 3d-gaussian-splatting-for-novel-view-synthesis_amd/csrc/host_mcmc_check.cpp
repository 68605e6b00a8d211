// host_mcmc_check.cpp -- host build of the per-row bodies in gs_mcmc.h, for CPU unit tests only (tests/test_mcmc_cpu.py).
//
// NOT part of the product path: the product library contains only HIP kernels and fails loudly without a GPU.  This file lets
// `pytest -m "not gpu"` check the random numbers, the weights, the draw and the relocation coefficient against the oracle
// (tests/mcmc_oracle.py) on a machine with no GPU.
#include "gs_mcmc.h"

using namespace gsmc;

extern "C" {

void hmc_philox(int64_t count, const uint32_t* ctr4, const uint32_t* key2, uint32_t* out4) {
    for (int64_t i = 0; i < count; ++i) philox4x32_10(ctr4 + i * 4, key2 + i * 2, out4 + i * 4);
}

// rows first .. first + count - 1 of one (seed, iteration, stream): the four words, the four u of them, the three normals
void hmc_row_random(uint64_t seed, int64_t first, int64_t count, uint32_t iteration, uint32_t stream, uint32_t* words4, float* u4, float* z3) {
    for (int64_t i = 0; i < count; ++i) {
        uint32_t x[4];
        row_random(seed, first + i, iteration, stream, x);
        for (int k = 0; k < 4; ++k) { words4[i * 4 + k] = x[k]; u4[i * 4 + k] = unit_open(x[k]); }
        normals3(x, z3 + i * 3);
    }
}

void hmc_weights(int64_t n, const float* opacity_raw, float min_opacity, uint32_t* w) {
    for (int64_t i = 0; i < n; ++i) w[i] = sample_weight(opacity_raw[i], min_opacity);
}

uint64_t hmc_mulhi64(uint64_t a, uint64_t b) { return mulhi64(a, b); }

void hmc_search(const uint64_t* prefix, int64_t n, int64_t count, const uint64_t* t, int64_t* out) {
    for (int64_t i = 0; i < count; ++i) out[i] = search_prefix(prefix, n, t[i]);
}

// the whole draw on given weights: exclusive prefix sums, then every row of weight 0 draws; src = -1 elsewhere.  Returns the total.
uint64_t hmc_draw(int64_t n, const uint32_t* w, uint64_t seed, uint32_t iteration, uint64_t* prefix, int32_t* src, int32_t* count) {
    uint64_t total = 0u;
    for (int64_t i = 0; i < n; ++i) { prefix[i] = total; total += w[i]; src[i] = -1; count[i] = 0; }
    if (total == 0u) return 0u;
    for (int64_t i = 0; i < n; ++i) {
        if (w[i] != 0u) continue;
        const int64_t s = draw_source(prefix, n, total, seed, i, iteration);
        src[i] = (int32_t)s; count[s] += 1;
    }
    return total;
}

void hmc_relocation_coefficient(double o, int32_t n, double min_opacity, double* o_new, double* ln_c) {
    relocation_coefficient(o, n, min_opacity, *o_new, *ln_c);
}

void hmc_relocated_values(float opacity_raw_src, const float* scale_raw_src, int32_t n, float min_opacity, float* opacity_raw_new,
                          float* scale_raw_new) {
    relocated_values(opacity_raw_src, scale_raw_src, n, min_opacity, *opacity_raw_new, scale_raw_new);
}

// returns 1 where the row moves
void hmc_noise(int64_t n, const float* opacity_raw, const float* scale_raw, const float* q_raw, float a, uint64_t seed, uint32_t iteration,
               float* d3, int32_t* moved) {
    for (int64_t i = 0; i < n; ++i) {
        uint32_t x[4];
        float z[3];
        row_random(seed, i, iteration, STREAM_NOISE, x);
        normals3(x, z);
        moved[i] = noise_displacement(scale_raw + i * 3, q_raw + i * 4, opacity_raw[i], z, a, d3 + i * 3) ? 1 : 0;
    }
}

float hmc_sigmoid_slope(float x) { return sigmoid_slope(x); }

float hmc_sigmoid(float x) { return gsm::sigmoidf_(x); }

}  // extern "C"
