// gs_project.h -- K1 project_kernel and K1b colour_kernel.
#pragma once
#include "gs_layout.h"
#include "gs_wave.h"

using namespace gsm;
namespace {

// (LDS is handed out in pieces of 1280 B: with fused inputs the projection kernels use 15 104 B -> 10 waves per CU; the 9-float
// rows of the un-fused layout would cost the fused kernels a piece, and a wave per CU, for nothing)
template <bool FUSED>
struct ProjectLds {
    float pos[64 * 3];
    float opa[64];
    float a[64 * (FUSED ? 4 : 9)];   // fused: q_raw [64][4]       un-fused: sigma [64][9]
    float b[64 * 3];                 // fused: scale_raw [64][3]   un-fused: colour [64][3]
};

template <bool FUSED>
__device__ __forceinline__ GaussIn gauss_from_lds(const ProjectLds<FUSED>& s, int lane) {
    GaussIn in;
#pragma unroll
    for (int k = 0; k < 3; ++k) in.p[k] = s.pos[lane * 3 + k];
    in.o_raw = s.opa[lane];
    if (FUSED) {
#pragma unroll
        for (int k = 0; k < 4; ++k) in.qr[k] = s.a[lane * 4 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) in.sr[k] = s.b[lane * 3 + k];
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) in.S9[k] = s.a[lane * 9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) in.col[k] = s.b[lane * 3 + k];
    }
    return in;
}

// the 12 values of GSPLAT_PROJECT_SAVE_SH_JACOBIAN: 48 contiguous bytes per lane
__device__ __forceinline__ void store_kj(float* __restrict__ kj_out, int64_t i, const float (&kj)[12]) {
    f4* dst = reinterpret_cast<f4*>(kj_out + i * 12);
    dst[0] = f4{kj[0], kj[1], kj[2], kj[3]};
    dst[1] = f4{kj[4], kj[5], kj[6], kj[7]};
    dst[2] = f4{kj[8], kj[9], kj[10], kj[11]};
}

template <bool FUSED>
__device__ __forceinline__ void stage_geometry(ProjectLds<FUSED>& s, const gsplat_gaussians& g, int64_t row0, int lane) {
    stage_rows<3>(s.pos, g.pos, row0, g.n, lane);
    stage_rows<1>(s.opa, g.opacity_raw, row0, g.n, lane);
    if (FUSED) {
        stage_rows<4>(s.a, g.q_raw, row0, g.n, lane);
        stage_rows<3>(s.b, g.scale_raw, row0, g.n, lane);
    } else {
        stage_rows<9>(s.a, g.sigma, row0, g.n, lane);
        stage_rows<3>(s.b, g.color, row0, g.n, lane);
    }
}

// COLOUR = false (fused inputs): geometry only, 44 of the 236 input bytes; colour_kernel evaluates the SH colour later,
// queued behind the copy of the counters so that it runs while the host reads them and sizes the binning buffers.
// The camera block (w2c, eye) is derived from c2w by every wave itself (16 uniform loads + 30 flops: cheaper than the launch of
// a 1-thread kernel in front); wave 0 stores it for the later kernels.  The first waves clear the coarse-bin totals
// bin_count_kernel accumulates into.  Epilogue: per-wave counts -> sharded counters -> the LAST wave to arrive (agent-scope
// acq_rel counter) adds the shards up, writes the totals (device, and the caller's mapped host block if given) and leaves
// the counter block zeroed for the next call.
// JAC (FUSED && COLOUR only): also store, per visible Gaussian, the 12 values that spare the backward the SH coefficients.
// TOTALS = false (GSPLAT_PROJECT_COUNTS_LATE): the waves only add to the sharded counters and leave; bin_count_kernel, queued
// right behind, totals and clears them.  (With the totals in here every wave waits for ALL its stores and atomics and then for
// a returning arrival atomic before it can retire: a quarter of a wave's life.)
// NB (FUSED && COLOUR): the active SH bases of the render's degree, 1 / 4 / 9 / 16 (gs_math.h).  NB = 1 (degree 0) needs no f_rest:
// nothing of it is staged and its 11 520 B of LDS are not reserved (with them goes the barrier that waited for the coefficients).
// NB = 4, 9 stage whole rows like NB = 16: the global_load_lds image of a block of rows is contiguous, three runs of 3 or 8 floats
// per row are not.
// (Workgroups of 2 / 4 waves instead of one: 89 / 91 us against 90 -- the kernel is not held by the rate at which one-wave
// workgroups can be dispatched.  As a STREAM -- 6 persistent waves per CU, two sets of LDS rows, block k + 1 requested before
// block k is computed -- 158 us against 96: with 1.5 waves per SIMD the long dependent chains of the geometry math issue at a
// fraction of the VALU rate; this kernel lives on wave-level parallelism.)
// FILTER: the screen-space low-pass (and, with vk.antialias, the opacity compensation) of gs_math.h project_gaussian<true>; the
// instantiations without it are the kernels they were.
template <bool FUSED, bool COLOUR, bool JAC = false, bool TOTALS = true, int NB = 16, bool FILTER = false>
__global__ __launch_bounds__(64) void project_kernel(gsplat_gaussians g, const float* __restrict__ c2w, Camera* __restrict__ cam_out, ViewK vk,
                                                     Records out, CounterBlock* cb, DevCounts* counts, DevCounts* counts_mapped,
                                                     uint32_t* __restrict__ bin_total, int nb, float* __restrict__ kj_out,
                                                     uint32_t* __restrict__ big_flag) {
    // DIRECT (fused inputs with the colour inside): the 44 bytes of geometry per Gaussian are loaded by the lanes themselves (rows
    // of 3 / 4 floats coalesce well enough) and only the 180 bytes of f_rest go through LDS: 11 520 B per wave instead of
    // 15 104 -> 12 waves per CU instead of 10, and the geometry math starts while the coefficients are still arriving.
    constexpr bool DIRECT = FUSED && COLOUR;
    constexpr bool REST = FUSED && COLOUR && NB > 1;         // does the colour read f_rest at all?
    static_assert(NB == 16 || DIRECT, "the SH degree belongs to the kernels that evaluate the colour");
    __shared__ float s_geo[DIRECT ? 4 : sizeof(ProjectLds<FUSED>) / 4];
    ProjectLds<FUSED>& s = *reinterpret_cast<ProjectLds<FUSED>*>(s_geo);
    __shared__ float s_rest[REST ? 64 * 45 : 4];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + lane;
    GaussIn in;
    float dc[3] = {0.f, 0.f, 0.f};                           // (DIRECT: the 3 f_dc values with the geometry; 11 520 B of LDS would allow 14
                                                             //  waves per CU, but the Jacobian variant needs 132 VGPRs: forced to 128 it spills, 94 us against 90)
    if (DIRECT) {                                            // (issued BEFORE the LDS-DMA: vmcnt counts in order)
        if (i < g.n) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dc[k] = g.f_dc[i * 3 + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) in.p[k] = g.pos[i * 3 + k];
            in.o_raw = g.opacity_raw[i];
            const f4 q = *reinterpret_cast<const f4*>(g.q_raw + i * 4);
            in.qr[0] = q.x; in.qr[1] = q.y; in.qr[2] = q.z; in.qr[3] = q.w;
#pragma unroll
            for (int k = 0; k < 3; ++k) in.sr[k] = g.scale_raw[i * 3 + k];
        }
    } else {
        stage_geometry<FUSED>(s, g, row0, lane);
    }
    if (REST) stage_rows<45>(s_rest, g.f_rest, row0, g.n, lane);                     // all inputs of the wave in flight at once
    Camera cam;                                              // (derived while the inputs are in flight)
    {
        float m[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = c2w[k];
        build_camera(m, cam);
        if (blockIdx.x == 0 && lane == 0) *cam_out = cam;
    }
    for (int b = blockIdx.x * 64 + lane; b < BIN_TOTAL_ROWS * nb; b += gridDim.x * 64) bin_total[b] = 0u;     // (every shard + the large Gaussians' totals and cursor)
    if (!DIRECT) __syncthreads();
    Proj o;
    o.vis = VIS_CULLED;
    if (i < g.n) {
        if (!DIRECT) in = gauss_from_lds<FUSED>(s, lane);
        o = project_geometry<FILTER>(in, FUSED, cam, vk);
    }
    if (REST) __syncthreads();                               // the SH coefficients have arrived
    RecOut r;
    r.vis = o.vis; r.tiles = 0; r.mask = 0u; r.ref_tiles = 0; r.rect = u2{0u, 0u}; r.ref_rect = u2{0u, 0u};
    float kj[12];
    if (FUSED) {
        if (o.vis == VIS_OK) r = project_finish<NB>(in, o, true, ShCoefLds{dc, s_rest + lane * 45}, cam, COLOUR, JAC ? kj : nullptr);
    } else if (o.vis == VIS_OK) {
        r = project_finish(in, o, false, ShCoefLds{nullptr, nullptr}, cam);
    }
    if (i < g.n) {
        if (r.vis == VIS_OK) {
            Rec64 line;
            line.r0 = r.r0; line.r1 = r.r1; line.r2 = r.r2; line.pad = r.r3;
            out.rec[i] = line;                   // 64 contiguous bytes per lane, 4 KB per wave
            out.rect[i] = r.rect;
            out.depth[i] = r.r2.w;
            out.mask[i] = r.mask;
            if (JAC) store_kj(kj_out, i, kj);
        }
        out.tiles[i] = r.tiles;
#ifdef GSPLAT_DIAGNOSTICS
        if (out.ref_rect) out.ref_rect[i] = r.ref_rect;
        if (out.ref_tiles) out.ref_tiles[i] = r.vis == VIS_OK ? r.ref_tiles : 0u;
#endif
    }
    {
        const bool any_large = __any(r.tiles != 0u && rect_is_big(r.rect));
        if (lane == 0) big_flag[blockIdx.x] = any_large ? 1u : 0u;
    }
    const unsigned long long surv = __ballot(o.vis != VIS_CULLED);
    const unsigned long long seen = __ballot(o.vis == VIS_OK);
    const uint32_t mx = wave_max(r.tiles), refp = wave_sum(r.ref_tiles), binp = wave_sum(r.tiles);
    uint32_t arrived = 0u;
    if (lane == 0) {
        CountShard* sh = cb->shards + (blockIdx.x % COUNT_SHARDS);
        if (surv) atomicAdd(&sh->survivors, (int)__popcll(surv));
        if (seen) atomicAdd(&sh->visible, (int)__popcll(seen));
        if (mx) atomicMax(&sh->max_tiles, (int)mx);
        if (refp) atomicAdd(&sh->ref_pairs, refp);
        if (binp) atomicAdd(&sh->bin_pairs, binp);
        // The adds above are agent-scope atomics (performed at the memory side, coherent without any cache maintenance); they
        // only have to be COMPLETE before this wave reports in: s_waitcnt vmcnt(0) (atomics stay counted until performed).  (An
        // agent-scope release fence here costs an L2 write-back per wave: 15 625 of them took 0.8 ms.)
        if (TOTALS) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // arrival, two levels: last wave of its shard -> last shard of the grid
            const uint32_t shard = blockIdx.x % COUNT_SHARDS, shards_used = min(gridDim.x, (uint32_t)COUNT_SHARDS);
            const uint32_t waves_of_shard = (gridDim.x - shard + COUNT_SHARDS - 1u) / COUNT_SHARDS;
            if (__hip_atomic_fetch_add(&sh->arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == waves_of_shard - 1u)
                arrived = (__hip_atomic_fetch_add(&cb->done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards_used - 1u) ? 1u : 0u;
        }
    }
    if (!TOTALS) return;
    arrived = (uint32_t)__builtin_amdgcn_readfirstlane((int)arrived);
    if (!arrived) return;
    // ---- last wave: totals of the 256 shards (4 per lane; agent-scope atomic loads: the adds were made at that scope)
    unsigned long long t4[4] = {0ull, 0ull, 0ull, 0ull};
    uint32_t mxt = 0u;
#pragma unroll
    for (int k = 0; k < COUNT_SHARDS / 64; ++k) {
        CountShard* sh = cb->shards + k * 64 + lane;
        t4[0] += (unsigned long long)(uint32_t)__hip_atomic_load(&sh->survivors, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t4[1] += (unsigned long long)(uint32_t)__hip_atomic_load(&sh->visible, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t4[2] += (unsigned long long)__hip_atomic_load(&sh->ref_pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t4[3] += (unsigned long long)__hip_atomic_load(&sh->bin_pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mxt = max(mxt, (uint32_t)__hip_atomic_load(&sh->max_tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        // leave the block zeroed for the next call (agent-scope stores: not parked in this XCD's L2 behind the atomics)
        __hip_atomic_store(&sh->survivors, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->visible, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->ref_pairs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->bin_pairs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->max_tiles, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int sft = 32; sft > 0; sft >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) t4[k] += (unsigned long long)__shfl_xor((long long)t4[k], sft);
        mxt = max(mxt, (uint32_t)__shfl_xor((int)mxt, sft));
    }
    if (lane == 0) {
        DevCounts c;
        c.n_survivors = (int32_t)t4[0]; c.n_visible = (int32_t)t4[1]; c.n_pairs = (int64_t)t4[2]; c.max_tiles = (int32_t)mxt;
        c.reserved = 0; c.n_binned = (int64_t)t4[3];
        *counts = c;
        if (counts_mapped) *counts_mapped = c;               // pinned host memory: visible to the host once the event behind us fires
        __hip_atomic_store(&cb->done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- K1b: SH colour (fused inputs) -------------------------------------------------------------------
// F3 for the Gaussians that were binned: 192 of the 236 input bytes per Gaussian are SH coefficients.  Writes r, g, b into
// the record line the geometry pass left (z stays).
// NB: as in project_kernel (NB = 1: f_rest is neither staged nor given LDS).
template <bool JAC, int NB = 16>
__global__ __launch_bounds__(64) void colour_kernel(gsplat_gaussians g, const Camera* __restrict__ camp, const uint32_t* __restrict__ tiles,
                                                    Rec64* __restrict__ rec, float* __restrict__ kj_out) {
    __shared__ float s_pos[64 * 3], s_dc[64 * 3], s_rest[NB > 1 ? 64 * 45 : 4];
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + lane;
    const bool need = i < g.n && tiles[i] != 0u;
    if (!__any(need)) return;                                // wave-uniform: skip 204 B / Gaussian when none is binned
    stage_rows<3>(s_pos, g.pos, row0, g.n, lane);
    stage_rows<3>(s_dc, g.f_dc, row0, g.n, lane);
    if (NB > 1) stage_rows<45>(s_rest, g.f_rest, row0, g.n, lane);
    const Camera cam = *camp;
    __syncthreads();
    if (need) {
        const float p[3] = {s_pos[lane * 3], s_pos[lane * 3 + 1], s_pos[lane * 3 + 2]};
        ShMid sm;
        sh_basis(p, cam.eye, sm);
        float rgb[3];
        if (JAC) {
            float kj[12];
            sh_colour_jac<NB>(sm, ShCoefLds{s_dc + lane * 3, s_rest + lane * 45}, rgb, kj);
            store_kj(kj_out, i, kj);
        } else {
            sh_colour<NB>(sm, ShCoefLds{s_dc + lane * 3, s_rest + lane * 45}, rgb);
        }
        float* r2 = reinterpret_cast<float*>(&rec[i].r2);
        r2[0] = rgb[0]; r2[1] = rgb[1]; r2[2] = rgb[2];
    }
}

}  // namespace
