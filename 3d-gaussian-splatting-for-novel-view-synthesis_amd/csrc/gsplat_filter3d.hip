// gsplat_filter3d.hip -- the Mip-Splatting 3D smoothing filter (not in the reference): the per-Gaussian sampling limit
// from the training cameras, and the filter applied to the raw scale and opacity, forward and backward.
//
// The per-row arithmetic is gs_filter3d.h (shared with the host test build).  Minimum and maximum are taken on the integer bits of
// positive floats (they order as unsigned integers), the one cross-workgroup value is an integer atomic max: every result is the same
// bits whatever order the waves run in, on any stream and on any data-parallel rank that holds the same positions.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_entry.h"
#include "gs_filter3d.h"

namespace {

constexpr int THREADS = 256;
constexpr int CAM_CHUNK = GSPLAT_FILTER3D_CAMERA_CHUNK;     // cameras staged in LDS at a time: 64 x 96 B = 6 KiB
constexpr int MAX_BLOCKS = 4096;                            // the streaming kernels stride over the rest
constexpr int64_t MAX_ROWS = 0x7fffffff;

static_assert(gsf3::CAMERA_FLOATS == GSPLAT_FILTER3D_CAMERA_FLOATS, "the header documents the camera record");
static_assert(CAM_CHUNK <= THREADS, "one thread stages one camera");

// ---- the sampling interval -------------------------------------------------------------------------------------------------
// POINTS Gaussians per lane (rows base + j THREADS of the workgroup's THREADS x POINTS rows: coalesced), all cameras.  A chunk of cameras
// is staged by the workgroup's first CAM_CHUNK lanes (the derived record of gs_filter3d.h), then every lane reads each record at a
// wave-uniform LDS address -- five 16-byte broadcasts -- and tests its POINTS positions against it, ~30 VALU instructions each: with one
// point per lane the LDS reads cost as much as the arithmetic (0.28 ms at 1 M x 200), with four they are a quarter of that.
// tbits[k] = the bits of min z / f over the cameras that see k, or UNSEEN; *t_max = the largest of them (an integer atomic max of at
// most one value per workgroup; zeroed by the caller's memset node).
constexpr int POINTS = 4;

__global__ __launch_bounds__(THREADS) void interval_kernel(int64_t n, const float* __restrict__ pos, int32_t n_cams, const float* __restrict__ cams,
                                                           float near, float margin, uint32_t* __restrict__ tbits, uint32_t* t_max) {
    __shared__ float4 staged[CAM_CHUNK * gsf3::STAGED_FLOATS / 4];
    __shared__ uint32_t wave_max[THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * (THREADS * POINTS) + threadIdx.x;
    float px[POINTS], py[POINTS], pz[POINTS];
    uint32_t best[POINTS];
#pragma unroll
    for (int j = 0; j < POINTS; ++j) {
        const int64_t i = base + (int64_t)j * THREADS;
        px[j] = py[j] = pz[j] = NAN;
        if (i < n) { px[j] = pos[i * 3]; py[j] = pos[i * 3 + 1]; pz[j] = pos[i * 3 + 2]; }
        best[j] = gsf3::UNSEEN;
    }
    for (int32_t c0 = 0; c0 < n_cams; c0 += CAM_CHUNK) {
        const int32_t cnt = n_cams - c0 < CAM_CHUNK ? n_cams - c0 : CAM_CHUNK;
        __syncthreads();                                                      // the previous chunk has been read
        if ((int32_t)threadIdx.x < cnt)
            gsf3::stage_camera(cams + (int64_t)(c0 + threadIdx.x) * gsf3::CAMERA_FLOATS, near, margin,
                               reinterpret_cast<float*>(staged) + threadIdx.x * gsf3::STAGED_FLOATS);
        __syncthreads();
        for (int32_t c = 0; c < cnt; ++c) {
            float rec[gsf3::STAGED_FLOATS];
#pragma unroll
            for (int k = 0; k < 5; ++k) {                                     // floats 0..19; the padding is not read
                const float4 v = staged[c * (gsf3::STAGED_FLOATS / 4) + k];
                rec[k * 4] = v.x; rec[k * 4 + 1] = v.y; rec[k * 4 + 2] = v.z; rec[k * 4 + 3] = v.w;
            }
#pragma unroll
            for (int j = 0; j < POINTS; ++j) {
                const uint32_t b = gsf3::camera_interval(rec, px[j], py[j], pz[j]);
                best[j] = b < best[j] ? b : best[j];
            }
        }
    }
    uint32_t m = 0u;
#pragma unroll
    for (int j = 0; j < POINTS; ++j) {
        const int64_t i = base + (int64_t)j * THREADS;
        if (!(gsf3::finite_bits(px[j]) && gsf3::finite_bits(py[j]) && gsf3::finite_bits(pz[j]))) best[j] = gsf3::UNSEEN;    // (a NaN or an infinity: seen by nobody)
        if (i < n) tbits[i] = best[j];
        if (best[j] != gsf3::UNSEEN && best[j] > m) m = best[j];
    }
    // the workgroup's maximum, then ONE atomic -- and only if it would raise the value: *t_max never falls, so a stale read can only
    // cost an atomic, never lose one (one atomic per wave, 15 625 on one address at 1 M rows, took 0.16 ms)
    for (int s = 32; s > 0; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)m, s); m = o > m ? o : m; }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < THREADS / 64; ++k) m = wave_max[k] > m ? wave_max[k] : m;
        if (m > __hip_atomic_load(t_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(t_max, m);
    }
}

// The second pass: a row nobody saw gets the largest interval of the seen ones (0 if there is none); filt = sqrt(s) t, in place.
__global__ __launch_bounds__(THREADS) void fill_kernel(int64_t n, float* __restrict__ filt, const uint32_t* __restrict__ t_max, float sqrt_s) {
    const uint32_t top = *t_max;
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t b = gsf3::float_bits(filt[i]);
        filt[i] = sqrt_s * gsf3::bits_float(b == gsf3::UNSEEN ? top : b);
    }
}

// ---- applying it -----------------------------------------------------------------------------------------------------------
// One row per lane and pass: 20 B in and 16 B out per row forward, 36 B in and 16 B out (16 B in more when adding) backward.  At 1 M rows
// the backward runs at 4.9 TB/s and the forward, bound by its four logarithms, at 3.2; a variant with four rows per lane
// and 16-byte accesses was measured 10 % SLOWER and is not kept.
__global__ __launch_bounds__(THREADS) void apply_kernel(int64_t n, const float* __restrict__ scale_raw, const float* __restrict__ opacity_raw,
                                                        const float* __restrict__ filt, float* __restrict__ scale_out, float* __restrict__ opacity_out) {
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
        const float s[3] = {scale_raw[i * 3], scale_raw[i * 3 + 1], scale_raw[i * 3 + 2]};
        float so[3], oo;
        gsf3::apply_row(s, opacity_raw[i], filt[i], so, oo);
        scale_out[i * 3] = so[0]; scale_out[i * 3 + 1] = so[1]; scale_out[i * 3 + 2] = so[2]; opacity_out[i] = oo;
    }
}

__global__ __launch_bounds__(THREADS) void apply_backward_kernel(int64_t n, const float* __restrict__ scale_raw, const float* __restrict__ opacity_raw,
                                                                 const float* __restrict__ filt, const float* __restrict__ g_scale_out,
                                                                 const float* __restrict__ g_opacity_out, float* __restrict__ g_scale_raw,
                                                                 float* __restrict__ g_opacity_raw, int accumulate) {
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
        const float s[3] = {scale_raw[i * 3], scale_raw[i * 3 + 1], scale_raw[i * 3 + 2]};
        const float gs[3] = {g_scale_out[i * 3], g_scale_out[i * 3 + 1], g_scale_out[i * 3 + 2]};
        float ds[3], dv;
        gsf3::apply_row_backward(s, opacity_raw[i], filt[i], gs, g_opacity_out[i], ds, dv);
        if (accumulate) { ds[0] += g_scale_raw[i * 3]; ds[1] += g_scale_raw[i * 3 + 1]; ds[2] += g_scale_raw[i * 3 + 2]; dv += g_opacity_raw[i]; }
        g_scale_raw[i * 3] = ds[0]; g_scale_raw[i * 3 + 1] = ds[1]; g_scale_raw[i * 3 + 2] = ds[2]; g_opacity_raw[i] = dv;
    }
}

inline bool real_nonneg(float x) { return std::isfinite(x) && x >= 0.f; }

unsigned stream_blocks(int64_t items) {
    const int64_t b = (items + THREADS - 1) / THREADS;
    return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

}  // namespace

extern "C" {

int64_t gsplat_filter3d_scratch_bytes(int64_t n) {
    if (n < 0 || n > MAX_ROWS) return -1;
    return 256;                                                // the maximum's word
}

int gsplat_filter3d_compute(int64_t n, const float* pos, int32_t n_cams, const float* cams, float near, float margin, float s, float* filt,
                            void* scratch, void* stream) {
    const char* E = "gsplat_filter3d_compute";
    if (n < 0 || n > MAX_ROWS) return bad_arg(E, "n must be in [0, 2^31)");
    if (n_cams < 0) return bad_arg(E, "n_cams must be >= 0");
    if (!real_nonneg(near)) return bad_arg(E, "near must be finite and >= 0");
    if (!real_nonneg(margin)) return bad_arg(E, "margin must be finite and >= 0");
    if (!real_nonneg(s)) return bad_arg(E, "s must be finite and >= 0");
    if (n == 0) return GSPLAT_OK;
    if (!filt) return bad_arg(E, "filt is NULL");
    if (!aligned(filt, 4)) return bad_arg(E, "filt must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (n_cams == 0) {                                         // no camera: every interval is 0
        (void)hipMemsetAsync(filt, 0, (size_t)n * sizeof(float), st);
        return launch_err(E);
    }
    if (!pos) return bad_arg(E, "pos is NULL");
    if (!cams) return bad_arg(E, "cams is NULL");
    if (!scratch) return bad_arg(E, "scratch is NULL");
    if (!aligned(pos, 4)) return bad_arg(E, "pos must be 4-byte aligned");
    if (!aligned(cams, 4)) return bad_arg(E, "cams must be 4-byte aligned");
    if (!aligned(scratch, 256)) return bad_arg(E, "scratch must be 256-byte aligned");
    uint32_t* t_max = (uint32_t*)scratch;
    (void)hipMemsetAsync(t_max, 0, sizeof(uint32_t), st);
    hipLaunchKernelGGL(interval_kernel, dim3((unsigned)((n + THREADS * POINTS - 1) / (THREADS * POINTS))), dim3(THREADS), 0, st, n, pos, n_cams, cams, near, margin,
                       (uint32_t*)filt, t_max);
    hipLaunchKernelGGL(fill_kernel, dim3(stream_blocks(n)), dim3(THREADS), 0, st, n, filt, (const uint32_t*)t_max, sqrtf(s));
    return launch_err(E);
}

int gsplat_filter3d_apply(int64_t n, const float* scale_raw, const float* opacity_raw, const float* filt, float* scale_out, float* opacity_out,
                          void* stream) {
    const char* E = "gsplat_filter3d_apply";
    if (n < 0 || n > MAX_ROWS) return bad_arg(E, "n must be in [0, 2^31)");
    if (n == 0) return GSPLAT_OK;
    if (!scale_raw) return bad_arg(E, "scale_raw is NULL");
    if (!opacity_raw) return bad_arg(E, "opacity_raw is NULL");
    if (!filt) return bad_arg(E, "filt is NULL");
    if (!scale_out) return bad_arg(E, "scale_out is NULL");
    if (!opacity_out) return bad_arg(E, "opacity_out is NULL");
    const void* all[5] = {scale_raw, opacity_raw, filt, scale_out, opacity_out};
    for (const void* p : all)
        if (!aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    hipLaunchKernelGGL(apply_kernel, dim3(stream_blocks(n)), dim3(THREADS), 0, (hipStream_t)stream, n, scale_raw, opacity_raw, filt, scale_out, opacity_out);
    return launch_err(E);
}

int gsplat_filter3d_apply_backward(int64_t n, const float* scale_raw, const float* opacity_raw, const float* filt, const float* g_scale_out,
                                   const float* g_opacity_out, float* g_scale_raw, float* g_opacity_raw, int32_t accumulate, void* stream) {
    const char* E = "gsplat_filter3d_apply_backward";
    if (n < 0 || n > MAX_ROWS) return bad_arg(E, "n must be in [0, 2^31)");
    if (n == 0) return GSPLAT_OK;
    if (!scale_raw) return bad_arg(E, "scale_raw is NULL");
    if (!opacity_raw) return bad_arg(E, "opacity_raw is NULL");
    if (!filt) return bad_arg(E, "filt is NULL");
    if (!g_scale_out) return bad_arg(E, "g_scale_out is NULL");
    if (!g_opacity_out) return bad_arg(E, "g_opacity_out is NULL");
    if (!g_scale_raw) return bad_arg(E, "g_scale_raw is NULL");
    if (!g_opacity_raw) return bad_arg(E, "g_opacity_raw is NULL");
    const void* all[7] = {scale_raw, opacity_raw, filt, g_scale_out, g_opacity_out, g_scale_raw, g_opacity_raw};
    for (const void* p : all)
        if (!aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    hipLaunchKernelGGL(apply_backward_kernel, dim3(stream_blocks(n)), dim3(THREADS), 0, (hipStream_t)stream, n, scale_raw, opacity_raw, filt,
                       g_scale_out, g_opacity_out, g_scale_raw, g_opacity_raw, (int)accumulate);
    return launch_err(E);
}

}  // extern "C"
