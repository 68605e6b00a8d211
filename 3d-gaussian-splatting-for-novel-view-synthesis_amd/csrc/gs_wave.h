// gs_wave.h -- wave64 primitives shared by the stages: row staging through LDS, DPP scans and reductions.
#pragma once
#include <hip/hip_runtime.h>
#include "gs_body.h"
#include "gs_adam.h"

using namespace gsm;
namespace {

// ---- rows of 64 Gaussians through LDS (K1, K1b, K8, the stand-alone ops) -----------------------------
// One wave64 per 64 Gaussians.  The reference layout is array-of-structures (pos[N,3], f_rest[N,45] ...): a lane
// reading its own row directly issues 45 loads that each touch 64 different cache lines.  Instead the wave copies its
// 64 contiguous rows into LDS with fully coalesced 16-byte accesses and every lane then reads its row from LDS
// (row strides 3, 4, 9, 45 words are conflict-free or 2-way at worst).  The SH block (f_dc + f_rest, 192 of the 236
// input bytes) is only fetched when at least one Gaussian of the wave survived the culls.
// Full 64-row blocks go global -> LDS directly (global_load_lds_dwordx4, gfx950): no VGPR round trip, and a wave can put
// all of its ~15 KB of inputs in flight at once and wait for them once (the kernels run at 8-10 waves per CU, so bytes
// in flight per wave are what buys bandwidth).  One such instruction writes 64 lanes x 16 B contiguously at a
// wave-uniform LDS base: exactly the row-block image.  The caller's __syncthreads() (vmcnt(0) + barrier) retires them.
// The last, partial block of an array takes the register path.
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* glb_ptr_t;

template <int R>
__device__ __forceinline__ void stage_rows(float* __restrict__ lds, const float* __restrict__ g, int64_t row0, int64_t n, int lane) {
    const int64_t left = n - row0;
    const float* __restrict__ src = g + row0 * R;             // 16-B aligned: row0 % 64 == 0, base 16-B aligned (host checks)
    constexpr int PIECES = 64 * R / 4;
    if (left >= 64) {
#pragma unroll
        for (int it = 0; it < (PIECES + 63) / 64; ++it) {
            const int piece = it * 64 + lane;
            if (piece < PIECES)
                __builtin_amdgcn_global_load_lds((glb_ptr_t)(src + piece * 4), (lds_ptr_t)(lds + it * 256), 16, 0, 0);
        }
        return;
    }
    const int total = (int)left * R;       // floats to copy
#pragma unroll
    for (int it = 0; it < (PIECES + 63) / 64; ++it) {
        const int piece = it * 64 + lane;
        if (piece * 4 + 3 < total) {
            *reinterpret_cast<f4*>(lds + piece * 4) = *reinterpret_cast<const f4*>(src + piece * 4);
        } else if (piece * 4 < total) {
            for (int k = piece * 4; k < total; ++k) lds[k] = src[k];
        }
    }
}

// ACC: the rows are ADDED to what g holds (the gradient of several views summed in place, GSPLAT_BACKWARD_ACCUMULATE)
template <int R, bool ACC = false>
__device__ __forceinline__ void unstage_rows(float* __restrict__ g, const float* __restrict__ lds, int64_t row0, int64_t n, int lane) {
    const int64_t left = n - row0;
    const int total = (int)(left < 64 ? left : 64) * R;
    float* __restrict__ dst = g + row0 * R;
    constexpr int PIECES = 64 * R / 4;
#pragma unroll
    for (int it = 0; it < (PIECES + 63) / 64; ++it) {
        const int piece = it * 64 + lane;
        if (piece * 4 + 3 < total) {
            f4 v = *reinterpret_cast<const f4*>(lds + piece * 4);
            if (ACC) { const f4 o = *reinterpret_cast<const f4*>(dst + piece * 4); v = f4{o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w}; }
            *reinterpret_cast<f4*>(dst + piece * 4) = v;
        } else if (piece * 4 < total) {
            for (int k = piece * 4; k < total; ++k) dst[k] = ACC ? dst[k] + lds[k] : lds[k];
        }
    }
}

// Rows [row0, row0 + 64) of g written as zeros, with the pieces of unstage_rows (SH degree 0: the f_rest gradient is not formed).
template <int R>
__device__ __forceinline__ void zero_rows(float* __restrict__ g, int64_t row0, int64_t n, int lane) {
    const int64_t left = n - row0;
    const int total = (int)(left < 64 ? left : 64) * R;
    float* __restrict__ dst = g + row0 * R;
    constexpr int PIECES = 64 * R / 4;
#pragma unroll
    for (int it = 0; it < (PIECES + 63) / 64; ++it) {
        const int piece = it * 64 + lane;
        if (piece * 4 + 3 < total) {
            *reinterpret_cast<f4*>(dst + piece * 4) = f4{0.f, 0.f, 0.f, 0.f};
        } else if (piece * 4 < total) {
            for (int k = piece * 4; k < total; ++k) dst[k] = 0.f;
        }
    }
}

// The rows of a wave's R-float gradients (in LDS, as unstage_rows would write them) applied to the parameter instead: one Adam step
// of rows [row0, row0 + 64) of p with the moments m, v -- 16-byte pieces, the same lanes reading and writing them.
// counts / capacity: the frame's device counters and the pair capacity it was queued with -- a frame that outgrew its buffers (its
// gradients are garbage and the host will render it again) or that has nothing on screen (the host will raise the reference's
// exception) must not step anything: the guard is on the device because the host has not looked at the counters yet.
// ZERO (SH degree 0): the gradient of every value is 0 and `lds` is not read -- the same adam_one, so moments left from a higher
// degree decay as they do in the optimiser's own kernel.
struct AdamRest { float* p; float* m; float* v; AdamStep k; const void* counts; long long capacity; };
typedef float fv4 __attribute__((ext_vector_type(4)));
template <int R, bool ZERO = false>
__device__ __forceinline__ void adam_rows(const AdamRest& a, const float* __restrict__ lds, int64_t row0, int64_t n, int lane) {
    const int64_t left = n - row0;
    const int total = (int)(left < 64 ? left : 64) * R;
    float* __restrict__ P = a.p + row0 * R; float* __restrict__ M = a.m + row0 * R; float* __restrict__ V = a.v + row0 * R;
    constexpr int PIECES = 64 * R / 4;
#pragma unroll
    for (int it = 0; it < (PIECES + 63) / 64; ++it) {
        const int piece = it * 64 + lane;
        if (piece * 4 + 3 < total) {
            fv4 p = *reinterpret_cast<const fv4*>(P + piece * 4), g = {0.f, 0.f, 0.f, 0.f};
            if (!ZERO) g = *reinterpret_cast<const fv4*>(lds + piece * 4);
            fv4 m = __builtin_nontemporal_load(reinterpret_cast<const fv4*>(M + piece * 4)), v = __builtin_nontemporal_load(reinterpret_cast<const fv4*>(V + piece * 4));
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float pc = p[c], gc = g[c], mc = m[c], vc = v[c];
                adam_one(pc, gc, mc, vc, 1.0f, false, a.k.step_size, a.k.b1, a.k.b2, a.k.inv_sqrt_bc2, a.k.eps);
                p[c] = pc; m[c] = mc; v[c] = vc;
            }
            __builtin_nontemporal_store(m, reinterpret_cast<fv4*>(M + piece * 4));
            __builtin_nontemporal_store(v, reinterpret_cast<fv4*>(V + piece * 4));
            *reinterpret_cast<fv4*>(P + piece * 4) = p;
        } else if (piece * 4 < total) {
            for (int k = piece * 4; k < total; ++k) {
                float gk = ZERO ? 0.f : lds[k];
                adam_one(P[k], gk, M[k], V[k], 1.0f, false, a.k.step_size, a.k.b1, a.k.b2, a.k.inv_sqrt_bc2, a.k.eps);
            }
        }
    }
}

struct ShCoefLds {          // same access as ShCoefGlobal, on the staged copy
    const float* dc;
    const float* rest;
    __device__ __forceinline__ float operator()(int k, int ch) const { return k == 0 ? dc[ch] : rest[ch * 15 + (k - 1)]; }
};

struct ShEmitLds {
    float* dc;
    float* rest;
    __device__ __forceinline__ void operator()(int k, int ch, float v) const {
        if (k == 0) dc[ch] = v; else rest[ch * 15 + (k - 1)] = v;
    }
};

// SH degree 0: only f_dc has a gradient (the f_rest rows are zeros, written without passing through LDS)
struct ShEmitDc {
    float* dc;
    float* rest;            // (not used: the same two fields as ShEmitLds, so that one expression builds either)
    __device__ __forceinline__ void operator()(int k, int ch, float v) const {
        if (k == 0) dc[ch] = v;
    }
};
// the emitter of a render with NB active bases
template <int NB> using ShEmitFor = std::conditional_t<(NB > 1), ShEmitLds, ShEmitDc>;

__device__ __forceinline__ bool rect_is_big(u2 rect) {
    const int w = (int)(rect.y & 0xFFFF) - (int)(rect.x & 0xFFFF) + 1, h = (int)(rect.y >> 16) - (int)(rect.x >> 16) + 1;
    return w * h > 32;
}

// ---- DPP: a lane reads another lane's register inside a VALU instruction -----------------------------
// v as lane-pattern CTRL delivers it; `idn` where the pattern (or the row mask RMASK) delivers nothing: the operation's identity.
template <int CTRL, int RMASK = 0xF>
__device__ __forceinline__ uint32_t dpp(uint32_t v, uint32_t idn = 0u) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)idn, (int)v, CTRL, RMASK, 0xF, false);
}
template <int CTRL, int RMASK = 0xF>
__device__ __forceinline__ float dpp(float v, float idn = 0.f) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(idn), __float_as_int(v), CTRL, RMASK, 0xF, false));
}
// Inclusive prefix sum over the 64 lanes in the VALU (DPP row shifts inside the rows of 16, row broadcasts across them): six adds,
// where six __shfl_up are six round trips through the LDS crossbar.
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
    x += dpp<0x111, 0xF>(x);            // row_shr:1
    x += dpp<0x112, 0xF>(x);            // row_shr:2
    x += dpp<0x114, 0xF>(x);            // row_shr:4
    x += dpp<0x118, 0xF>(x);            // row_shr:8
    x += dpp<0x142, 0xA>(x);            // row_bcast:15 -> rows 1, 3
    x += dpp<0x143, 0xC>(x);            // row_bcast:31 -> rows 2, 3
    return x;
}
// Sum / maximum / minimum over the 64 lanes the same way (the result in every lane, through lane 63 and an SGPR): six DPP steps
// instead of six ds_bpermute butterflies.
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(x), 63);
}
// The same sum of a float: the partial sums meet in a fixed order (the DPP pattern), so the result does not change from run to run.
__device__ __forceinline__ float wave_sum_f(float x) {
    x += dpp<0x111, 0xF>(x); x += dpp<0x112, 0xF>(x); x += dpp<0x114, 0xF>(x);
    x += dpp<0x118, 0xF>(x); x += dpp<0x142, 0xA>(x); x += dpp<0x143, 0xC>(x);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
    x = max(x, dpp<0x111, 0xF>(x)); x = max(x, dpp<0x112, 0xF>(x)); x = max(x, dpp<0x114, 0xF>(x));
    x = max(x, dpp<0x118, 0xF>(x)); x = max(x, dpp<0x142, 0xA>(x)); x = max(x, dpp<0x143, 0xC>(x));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
    constexpr uint32_t I = 0xFFFFFFFFu;
    x = min(x, dpp<0x111, 0xF>(x, I)); x = min(x, dpp<0x112, 0xF>(x, I)); x = min(x, dpp<0x114, 0xF>(x, I));
    x = min(x, dpp<0x118, 0xF>(x, I)); x = min(x, dpp<0x142, 0xA>(x, I)); x = min(x, dpp<0x143, 0xC>(x, I));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
// A barrier for a group of threads: the workgroup, or (WAVE) one wave by itself -- then nothing but the order of the wave's own LDS
// instructions, which the fences keep the compiler from changing (K4 has the details).
template <bool WAVE>
__device__ __forceinline__ void group_sync() {
    if (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
    } else {
        __syncthreads();
    }
}

// lane src's value of x in every lane (through an SGPR)
__device__ __forceinline__ float readlane_f(float x, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src)); }

}  // namespace
