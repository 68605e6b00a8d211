// gsplat_mcmc.hip -- density control at a fixed budget (not in the reference): the position noise and the two
// regularisers of every iteration, and the refinement that moves dead Gaussians onto live ones in place.
//
// The per-row arithmetic is gs_mcmc.h (shared with the host test build).  Nothing here waits on another workgroup: the prefix sum
// is three launches (block sums, one workgroup over the block sums, rescan with offsets), the relocation two (destinations read
// the sources' old values in the first, the sources change in the second).  The draw counts are int32 atomics and the weights
// integers, so every result is the same bits whatever order the waves run in -- and on every data-parallel rank.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_blocksum.h"
#include "gs_entry.h"
#include "gs_mcmc.h"

namespace {

constexpr int THREADS = 256;
constexpr int SCAN_BLOCK = 256;     // rows per workgroup of the scan (one per lane)
constexpr int SCAN_CHUNK = 256;     // block sums one pass of the middle kernel holds (one per lane)
constexpr int REG_PARTS = 512;      // workgroups of the regulariser = partial sums

struct Layout { int64_t bytes, reg, w, prefix, src, count, total, block_sums; };

inline int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

Layout layout_of(int64_t n) {
    Layout L;
    const int64_t blocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    int64_t off = 0;
    L.reg = off;        off += up256(256 + (int64_t)REG_PARTS * 2 * sizeof(double));    // arrival counter | partial sums
    L.total = off;      off += 256;
    L.w = off;          off += up256(n * 4);
    L.prefix = off;     off += up256(n * 8);
    L.src = off;        off += up256(n * 4);
    L.count = off;      off += up256(n * 4);
    L.block_sums = off; off += up256(blocks * 8);
    L.bytes = off;
    return L;
}

// ---- every iteration ---------------------------------------------------------------------------------------------------------
// Streaming, one row per lane: 32 B of covariance parameters + 4 B opacity in, 12 B position in and out (56 B per row).
__global__ __launch_bounds__(THREADS) void noise_kernel(int64_t n, float* __restrict__ pos, const float* __restrict__ opacity_raw,
                                                        const float* __restrict__ scale_raw, const float* __restrict__ q_raw, float a,
                                                        uint64_t seed, uint32_t iteration) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float sr[3] = {scale_raw[i * 3], scale_raw[i * 3 + 1], scale_raw[i * 3 + 2]};
    const float4 q4 = *reinterpret_cast<const float4*>(q_raw + i * 4);
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    uint32_t x[4];
    gsmc::row_random(seed, i, iteration, gsmc::STREAM_NOISE, x);
    float z[3], d[3];
    gsmc::normals3(x, z);
    if (!gsmc::noise_displacement(sr, q, opacity_raw[i], z, a, d)) return;          // gate exactly 0: the row keeps its bits
    pos[i * 3] += d[0]; pos[i * 3 + 1] += d[1]; pos[i * 3 + 2] += d[2];
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    gsblk::sum(v, red);
    const double t = gsblk::column<THREADS / 64>(red);                     // (every thread: the caller's branches are uniform)
    __syncthreads();                                                       // (red is free for the next sum)
    return t;
}

// L_o = lambda_o mean sigmoid(opacity_raw), L_s = lambda_s mean exp(scale_raw); their gradients are ADDED to the two gradient arrays.
// One launch: every workgroup leaves its two partial sums (double), the LAST one to arrive adds them in index order and writes
// values[3] = (L_o, L_s, *base + L_o + L_s).  The arrival counter only elects who adds; nobody waits, and the sums do not depend
// on who was elected.  (The partials are agent-scope stores, performed at the memory side, and are complete before the arrival is
// counted -- as the projection kernel's counters are, gs_project.h.)
__global__ __launch_bounds__(THREADS) void regularise_kernel(int64_t n, const float* __restrict__ opacity_raw, const float* __restrict__ scale_raw,
                                                             float* __restrict__ g_opacity, float* __restrict__ g_scale, float lambda_o,
                                                             float lambda_s, float go, float gsc, const float* __restrict__ base,
                                                             float* __restrict__ values, uint32_t* arrived, double* part) {
    __shared__ double red[4];
    __shared__ uint32_t last;
    double so = 0.0, ss = 0.0;
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
        const float x = opacity_raw[i];
        so += (double)gsm::sigmoidf_(x);
        if (g_opacity) g_opacity[i] += go * gsmc::sigmoid_slope(x);
    }
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n * 3; i += stride) {
        const float e = expf(scale_raw[i]);
        ss += (double)e;
        if (g_scale) g_scale[i] += gsc * e;
    }
    so = block_sum(so, red);
    ss = block_sum(ss, red);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&part[blockIdx.x * 2], so, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&part[blockIdx.x * 2 + 1], ss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        last = (__hip_atomic_fetch_add(arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    double to = 0.0, ts = 0.0;
    for (uint32_t k = threadIdx.x; k < gridDim.x; k += THREADS) {           // lane t: parts t, t + 256, ... in that order
        to += __hip_atomic_load(&part[k * 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ts += __hip_atomic_load(&part[k * 2 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    to = block_sum(to, red);
    ts = block_sum(ts, red);
    if (threadIdx.x == 0) {
        const float lo = (float)((double)lambda_o * to / (double)n), ls = (float)((double)lambda_s * ts / (3.0 * (double)n));
        values[0] = lo; values[1] = ls; values[2] = (base ? *base : 0.f) + lo + ls;
        __hip_atomic_store(arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // zero again for the next call
    }
}

// ---- refinement: weights and their exclusive prefix sum ----------------------------------------------------------------------
// exclusive scan of one value per lane over the workgroup; returns the workgroup's total through `total`
__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t* wave_tot, uint64_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
    for (int s = 1; s < 64; s <<= 1) {
        const uint64_t up = (uint64_t)__shfl_up((long long)inc, s);
        if (lane >= s) inc += up;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint64_t before = 0u, all = 0u;
    for (int k = 0; k < THREADS / 64; ++k) { const uint64_t t = wave_tot[k]; if (k < wave) before += t; all += t; }
    __syncthreads();
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(THREADS) void weight_kernel(int64_t n, const float* __restrict__ opacity_raw, float min_opacity,
                                                         uint32_t* __restrict__ w, int32_t* __restrict__ src, int32_t* __restrict__ count,
                                                         uint64_t* __restrict__ block_sums) {
    __shared__ uint64_t wave_tot[THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    uint32_t wi = 0u;
    if (i < n) {
        wi = gsmc::sample_weight(opacity_raw[i], min_opacity);
        w[i] = wi; src[i] = -1; count[i] = 0;
    }
    uint64_t total;
    block_exclusive_scan((uint64_t)wi, wave_tot, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block sums -> exclusive offsets in place, SCAN_CHUNK at a time; the grand total
__global__ __launch_bounds__(THREADS) void block_offsets_kernel(int64_t blocks, uint64_t* __restrict__ block_sums, uint64_t* __restrict__ total_out) {
    __shared__ uint64_t wave_tot[THREADS / 64];
    uint64_t running = 0u;
    for (int64_t c = 0; c < blocks; c += SCAN_CHUNK) {
        const int64_t k = c + threadIdx.x;
        const uint64_t v = k < blocks ? block_sums[k] : 0u;
        uint64_t total;
        const uint64_t ex = block_exclusive_scan(v, wave_tot, total);
        if (k < blocks) block_sums[k] = running + ex;
        running += total;
    }
    if (threadIdx.x == 0) *total_out = running;
}

__global__ __launch_bounds__(THREADS) void prefix_kernel(int64_t n, const uint32_t* __restrict__ w, const uint64_t* __restrict__ block_off,
                                                         uint64_t* __restrict__ prefix) {
    __shared__ uint64_t wave_tot[THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * SCAN_BLOCK + threadIdx.x;
    const uint64_t wi = i < n ? (uint64_t)w[i] : 0u;
    uint64_t total;
    const uint64_t ex = block_exclusive_scan(wi, wave_tot, total);
    if (i < n) prefix[i] = block_off[blockIdx.x] + ex;
}

// every dead row draws one source in proportion to the weights
__global__ __launch_bounds__(THREADS) void draw_kernel(int64_t n, const uint32_t* __restrict__ w, const uint64_t* __restrict__ prefix,
                                                       const uint64_t* __restrict__ total_p, uint64_t seed, uint32_t iteration,
                                                       int32_t* __restrict__ src, int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n || w[i] != 0u) return;
    const uint64_t total = *total_p;
    if (total == 0u) return;
    const int64_t s = gsmc::draw_source(prefix, n, total, seed, i, iteration);
    src[i] = (int32_t)s;
    atomicAdd(&count[s], 1);
}

struct Params { float* pos; float* f_dc; float* f_rest; float* opacity_raw; float* scale_raw; float* q_raw; };
struct Moments { float* m[12]; };       // exp_avg, exp_avg_sq of pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw (NULL: no optimiser state)

__device__ __forceinline__ void zero_moments(const Moments& mo, int64_t i) {
    const int width[6] = {3, 3, 45, 1, 3, 4};
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float* p = mo.m[t * 2 + h];
            if (p) for (int k = 0; k < width[t]; ++k) p[i * width[t] + k] = 0.f;
        }
}

// first launch: a destination (a dead row that drew) becomes its source, from the source's OLD values
__global__ __launch_bounds__(THREADS) void relocate_destinations_kernel(int64_t n, Params p, Moments mo, const int32_t* __restrict__ src,
                                                                        const int32_t* __restrict__ count, float min_opacity) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t s = src[i];
    if (s < 0) return;
    for (int k = 0; k < 3; ++k) { p.pos[i * 3 + k] = p.pos[s * 3 + k]; p.f_dc[i * 3 + k] = p.f_dc[s * 3 + k]; }
    for (int k = 0; k < 45; ++k) p.f_rest[i * 45 + k] = p.f_rest[s * 45 + k];
    for (int k = 0; k < 4; ++k) p.q_raw[i * 4 + k] = p.q_raw[s * 4 + k];
    const float sr[3] = {p.scale_raw[s * 3], p.scale_raw[s * 3 + 1], p.scale_raw[s * 3 + 2]};
    const int c = count[s];
    float o_new, s_new[3];
    gsmc::relocated_values(p.opacity_raw[s], sr, (c < gsmc::RELOCATE_MAX_N ? c : gsmc::RELOCATE_MAX_N - 1) + 1, min_opacity, o_new, s_new);
    p.opacity_raw[i] = o_new;
    for (int k = 0; k < 3; ++k) p.scale_raw[i * 3 + k] = s_new[k];
    zero_moments(mo, i);
}

// second launch: the sources take the same new opacity and scale
__global__ __launch_bounds__(THREADS) void relocate_sources_kernel(int64_t n, Params p, Moments mo, const int32_t* __restrict__ count, float min_opacity) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int c = count[i];
    if (c <= 0) return;
    const float sr[3] = {p.scale_raw[i * 3], p.scale_raw[i * 3 + 1], p.scale_raw[i * 3 + 2]};
    float o_new, s_new[3];
    gsmc::relocated_values(p.opacity_raw[i], sr, (c < gsmc::RELOCATE_MAX_N ? c : gsmc::RELOCATE_MAX_N - 1) + 1, min_opacity, o_new, s_new);
    p.opacity_raw[i] = o_new;
    for (int k = 0; k < 3; ++k) p.scale_raw[i * 3 + k] = s_new[k];
    zero_moments(mo, i);
}

constexpr int64_t MAX_ROWS = 0x7fffffff;      // src is int32

}  // namespace

extern "C" {

int64_t gsplat_mcmc_scratch_bytes(int64_t n) {
    if (n < 0 || n > MAX_ROWS) return -1;
    return layout_of(n).bytes;
}

int gsplat_mcmc_scratch_layout(int64_t n, gsplat_mcmc_layout* out) {
    if (n < 0 || n > MAX_ROWS) return bad_arg("gsplat_mcmc_scratch_layout", "n must be in [0, 2^31)");
    if (!out) return bad_arg("gsplat_mcmc_scratch_layout", "out is NULL");
    const Layout L = layout_of(n);
    out->bytes = L.bytes; out->reg = L.reg; out->w = L.w; out->prefix = L.prefix; out->src = L.src; out->count = L.count;
    out->total = L.total; out->block_sums = L.block_sums; out->scan_block = SCAN_BLOCK; out->scan_chunk = SCAN_CHUNK;
    return GSPLAT_OK;
}

int gsplat_mcmc_noise(int64_t n, float* pos, const float* opacity_raw, const float* scale_raw, const float* q_raw, float scale,
                      uint64_t seed, uint32_t iteration, void* stream) {
    const char* E = "gsplat_mcmc_noise";
    if (n < 0 || n > MAX_ROWS) return bad_arg(E, "n must be in [0, 2^31)");
    if (!std::isfinite(scale)) return bad_arg(E, "scale must be finite");
    if (n == 0) return GSPLAT_OK;
    if (!pos || !opacity_raw || !scale_raw || !q_raw) return bad_arg(E, "NULL array");
    if (!aligned(pos, 4) || !aligned(opacity_raw, 4) || !aligned(scale_raw, 4) || !aligned(q_raw, 16)) return bad_arg(E, "q_raw must be 16-byte aligned, the others 4");
    hipLaunchKernelGGL(noise_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, n, pos, opacity_raw,
                       scale_raw, q_raw, scale, seed, iteration);
    return launch_err(E);
}

int gsplat_mcmc_regularise(int64_t n, const float* opacity_raw, const float* scale_raw, float* grad_opacity_raw, float* grad_scale_raw,
                           float lambda_opacity, float lambda_scale, const float* base, float* values, void* scratch, void* stream) {
    const char* E = "gsplat_mcmc_regularise";
    if (n < 0 || n > MAX_ROWS) return bad_arg(E, "n must be in [0, 2^31)");
    if (!std::isfinite(lambda_opacity) || !std::isfinite(lambda_scale) || lambda_opacity < 0.f || lambda_scale < 0.f)
        return bad_arg(E, "the weights must be finite and >= 0");
    if (n == 0) return GSPLAT_OK;
    if (!opacity_raw || !scale_raw || !values || !scratch) return bad_arg(E, "NULL array");
    if (!aligned(scratch, 256)) return bad_arg(E, "scratch must be 256-byte aligned");
    const Layout L = layout_of(n);
    uint32_t* arrived = (uint32_t*)((char*)scratch + L.reg);
    double* part = (double*)((char*)scratch + L.reg + 256);
    int64_t blocks = (n * 3 + THREADS * 4 - 1) / (THREADS * 4);           // four values per lane and pass at least
    if (blocks > REG_PARTS) blocks = REG_PARTS;
    hipLaunchKernelGGL(regularise_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, n, opacity_raw, scale_raw,
                       grad_opacity_raw, grad_scale_raw, lambda_opacity, lambda_scale, (float)((double)lambda_opacity / (double)n),
                       (float)((double)lambda_scale / (3.0 * (double)n)), base, values, arrived, part);
    return launch_err(E);
}

int gsplat_mcmc_refine(float* pos, float* f_dc, float* f_rest, float* opacity_raw, float* scale_raw, float* q_raw,
                       const gsplat_mcmc_moments* moments, int64_t n, float min_opacity, uint64_t seed, uint32_t iteration, void* scratch,
                       void* stream) {
    const char* E = "gsplat_mcmc_refine";
    if (n < 0 || n > MAX_ROWS) return bad_arg(E, "n must be in [0, 2^31)");
    if (!(min_opacity >= 0.f && min_opacity < 1.f)) return bad_arg(E, "min_opacity must be in [0, 1)");
    if (n == 0) return GSPLAT_OK;
    if (!pos || !f_dc || !f_rest || !opacity_raw || !scale_raw || !q_raw) return bad_arg(E, "NULL parameter array");
    if (!scratch || !aligned(scratch, 256)) return bad_arg(E, "scratch must be a 256-byte aligned device buffer");
    Moments mo;
    for (int k = 0; k < 12; ++k) mo.m[k] = nullptr;
    if (moments) {
        float* const all[12] = {moments->pos[0], moments->pos[1], moments->f_dc[0], moments->f_dc[1], moments->f_rest[0], moments->f_rest[1],
                                moments->opacity_raw[0], moments->opacity_raw[1], moments->scale_raw[0], moments->scale_raw[1],
                                moments->q_raw[0], moments->q_raw[1]};
        for (int k = 0; k < 12; k += 2) {
            if ((all[k] == nullptr) != (all[k + 1] == nullptr)) return bad_arg(E, "a parameter has one moment without the other");
            mo.m[k] = all[k]; mo.m[k + 1] = all[k + 1];
        }
    }
    const Layout L = layout_of(n);
    char* sb = (char*)scratch;
    uint32_t* w = (uint32_t*)(sb + L.w);
    uint64_t* prefix = (uint64_t*)(sb + L.prefix);
    int32_t* src = (int32_t*)(sb + L.src);
    int32_t* count = (int32_t*)(sb + L.count);
    uint64_t* total = (uint64_t*)(sb + L.total);
    uint64_t* block_sums = (uint64_t*)(sb + L.block_sums);
    const int64_t blocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    const dim3 grid((unsigned)blocks), rows((unsigned)((n + THREADS - 1) / THREADS)), tb(THREADS);
    hipStream_t st = (hipStream_t)stream;
    const Params p{pos, f_dc, f_rest, opacity_raw, scale_raw, q_raw};
    hipLaunchKernelGGL(weight_kernel, grid, tb, 0, st, n, (const float*)opacity_raw, min_opacity, w, src, count, block_sums);
    hipLaunchKernelGGL(block_offsets_kernel, dim3(1), tb, 0, st, blocks, block_sums, total);
    hipLaunchKernelGGL(prefix_kernel, grid, tb, 0, st, n, (const uint32_t*)w, (const uint64_t*)block_sums, prefix);
    hipLaunchKernelGGL(draw_kernel, rows, tb, 0, st, n, (const uint32_t*)w, (const uint64_t*)prefix, (const uint64_t*)total, seed, iteration, src, count);
    hipLaunchKernelGGL(relocate_destinations_kernel, rows, tb, 0, st, n, p, mo, (const int32_t*)src, (const int32_t*)count, min_opacity);
    hipLaunchKernelGGL(relocate_sources_kernel, rows, tb, 0, st, n, p, mo, (const int32_t*)count, min_opacity);
    return launch_err(E);
}

}  // extern "C"
