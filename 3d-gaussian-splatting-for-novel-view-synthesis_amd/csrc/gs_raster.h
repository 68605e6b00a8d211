// gs_raster.h -- K6 / K7 raster kernels and the deterministic-mode kernels.
#pragma once
#include "gs_layout.h"
#include "gs_wave.h"

using namespace gsm;
namespace {

// ---- K6 / K7: rasterizer -----------------------------------------------------------------------------
// One wave64 per list (16 x 8 pixels).  The wave is EIGHT groups of 8 lanes: group g owns the 4 x 4-pixel sub-tile
// (g & 3, g >> 2) of the list; lane j of a group owns pixels (j & 3, j >> 2) and (j & 3, (j >> 2) + 2) of the sub-tile, so a
// lane's two pixels form a float2 and the arithmetic runs on packed fp32 (v_pk_fma_f32 ...).
//
// Why groups: a projected Gaussian covers ~57 pixels on the benchmark scene, a list 128: with the whole wave evaluating
// every list entry only 13 % of the lane evaluations were inside the ellipse, and both raster kernels are VALU-bound.
// So the wave walks its depth-sorted list 64 entries at a time; lane l fetches entry l's 64-byte record, stages it in LDS
// (conic pre-scaled for exp2) and tests the entry's bounding box {|du| <= ex, |dv| <= ey} against the 8 sub-tiles; one
// ballot per sub-tile compacts the touching entries, in depth order, into that sub-tile's queue (LDS, 2-byte record
// offsets).  In the inner loop every group pops ITS OWN queue: one iteration composites eight different (sub-tile,
// Gaussian) pairs, 2.7x fewer pixel evaluations than list-wide evaluation (tools/subtile_stats.py); the loop runs to the
// longest of the 8 queues (queues padded with a null record: opacity 0 -> alpha 0).  A Gaussian missing from a sub-tile's
// queue has q > chi, i.e. alpha = 0, on all of its pixels: the composite is unchanged term by term.
// The next chunk's records are fetched while the current chunk is composited.
//
// Launch order: block b takes list order[b] (longest first, from plan_kernel), and the first blocks raise their wave
// priority so that a dense list is not slowed down by light co-resident waves.
typedef float v2f __attribute__((ext_vector_type(2)));
// Exact ellipse / sub-tile test at staging time (subtile_mask_exact), measured on one box: the backward, whose iterations cost
// 2.5x the forward's, gains (217 -> 207 us); the forward loses (85.6 -> 91.5 us) and keeps the box test.
// (per-chunk partial sums of the colour and the suffix sums: tried and dropped)
constexpr int CHUNK = 64;                            // list entries staged per round (one per lane)
constexpr int QCAP = CHUNK + 8;                      // queue capacity: the inner loops read entries in pairs
constexpr uint32_t NULL_OFF = CHUNK * 16;            // byte offset of the null record
constexpr int N_SUB = 8;                             // 4 x 2 sub-tiles of 4 x 4 pixels

// Per-wave statistics for tools/raster_stats.py: only a diagnostics build (-DGSPLAT_DIAGNOSTICS, libgsplat_mi355x_diag.so)
// can register a buffer; the product library always passes NULL.
struct WaveStats { uint32_t list_len, chunks, visited, cycles, begin_lo, launch_index; };   // chunks | duration in 100 MHz ticks << 12; begin: 100 MHz ticks; launch_index | XCD << 24
__device__ __forceinline__ uint32_t xcc_id() {                // (every XCD has its own s_memtime counter)
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 0xFu;
}
#ifdef GSPLAT_DIAGNOSTICS
WaveStats* g_stats_fwd = nullptr;
WaveStats* g_stats_bwd = nullptr;
u2* g_ref_rect = nullptr;            // tools/ref_pairs_diff.py: the reference's own tile rectangle (F10) and tile count per Gaussian
uint32_t* g_ref_tiles = nullptr;
#define STATS_FWD g_stats_fwd
#define STATS_BWD g_stats_bwd
#define REF_RECT g_ref_rect
#define REF_TILES g_ref_tiles
#else
#define STATS_FWD ((WaveStats*)nullptr)
#define STATS_BWD ((WaveStats*)nullptr)
#define REF_RECT ((u2*)nullptr)
#define REF_TILES ((uint32_t*)nullptr)
#endif

constexpr float QK = -0.72134752044448170368f;      // -0.5 * log2(e)

template <int Q>               // Q = slots per queue (the forward kernel: QCAP; the backward kernel, whose queues are capped: fewer)
struct RasterLdsT {
    static constexpr int QSLOTS = Q;
    f4 r0[CHUNK + 1];          // u, v, k A11, 2 k A12                    [CHUNK] = the null record
    f4 r1[CHUNK + 1];          // k A22, opacity, r, g
    f4 r2[CHUNK + 1];          // b, Gaussian id (bits), camera depth z (the depth / opacity variants; else 0), 0
    uint16_t q[N_SUB][Q];      // per sub-tile: record offsets (16 * entry) of the entries that touch it, depth order
};
using RasterLds = RasterLdsT<QCAP>;
static_assert(sizeof(uint16_t) * N_SUB * QCAP == 16 * QCAP, "queue block = QCAP 16-byte pieces");

struct Candidate {         // one list entry held by one lane between fetch and staging
    f4 q0, q1, q2;
    uint32_t id;
    uint32_t saved_mask;   // (backward) the sub-tile mask the forward left for this pair
};

__device__ __forceinline__ Candidate fetch_candidate(int lane, uint32_t base, uint32_t end, const uint32_t* __restrict__ ids,
                                                     const Rec64* __restrict__ rec, uint32_t id_max,
                                                     const uint8_t* __restrict__ pair_mask = nullptr) {
    Candidate c;
    const uint32_t idx = base + lane;
    c.id = 0;
    c.saved_mask = 0u;
    c.q0 = c.q1 = c.q2 = f4{0.f, 0.f, 0.f, 0.f};
    if (idx < end) {
        if (pair_mask) c.saved_mask = pair_mask[idx];
        c.id = min(ids[idx], id_max);                     // never gather outside the record array
        const Rec64* __restrict__ r = rec + c.id;        // one 64-byte line
        c.q0 = r->r0;
        c.q1 = r->r1;
        c.q2 = r->r2;
    }
    return c;
}

// Which of the list's 8 sub-tiles can the Gaussian touch?  Bit s = its box [u - ex, u + ex] x [v - ey, v + ey] (the padded
// half-extents of {q <= chi} from the projection, gs_math.h) meets the pixel centres of sub-tile s.  (ox, oy) = list origin.
__device__ __forceinline__ uint32_t subtile_mask(const Candidate& c, float ox, float oy) {
    const float x0 = c.q0.x - c.q1.z - ox, x1 = c.q0.x + c.q1.z - ox;
    const float y0 = c.q0.y - c.q1.w - oy, y1 = c.q0.y + c.q1.w - oy;
    uint32_t cm = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) cm |= (x1 >= (float)(4 * k) && x0 <= (float)(4 * k + 3)) ? (1u << k) : 0u;
    uint32_t m = 0u;
    if (y1 >= 0.f && y0 <= 3.f) m |= cm;
    if (y1 >= 4.f && y0 <= 7.f) m |= cm << 4;
    return m;
}

// Stage one chunk: records into LDS, sub-tile queues built.  n = entries offered (uniform, <= CHUNK).  A queue holds at most
// MAXQ entries: when a sub-tile would get more, the chunk is cut to the longest prefix of the list that fits (the rest
// comes back in the next chunk).  Returns {entries taken, length of the longest queue} (uniform); m8 = the lane's sub-tile
// mask (0 beyond the entries taken), ranks = the lane's position in each of its queues (8 bits per sub-tile).
struct Staged { int n, maxc; };
// The same question answered exactly: does {q <= chi} (padded by 1e-3 like the list test of the projection, gs_math.h) reach the
// pixel centres of sub-tile s?  q is convex: its minimum over the sub-tile's rectangle is 0 if the centre is inside, else it lies
// on an edge that FACES the centre.  With X = the centre's x clamped to the rectangle (0 in centre-relative coordinates if it
// is inside the x-range, else the nearer vertical edge) the line x = X is that vertical edge -- or, when there is none, a line
// through the rectangle, whose points are harmless extra candidates -- and the minimum of q along it is a clamped 1-D quadratic
// (v_med3); the same with Y.  min(qx, qy) is then the exact minimum in every case, the centre-inside case (X = Y = 0 -> 0)
// included.  ~135 instructions per entry for the 8 sub-tiles; removes ~14 % of the (sub-tile, Gaussian) pairs the box test lets
// through.  Non-PD conics: every sub-tile.
__device__ __forceinline__ uint32_t subtile_mask_exact(const Candidate& c, float ox, float oy, float chi_pad) {
    const float u = c.q0.x - ox, v = c.q0.y - oy, A = c.q0.z, B = c.q0.w, C = c.q1.x;
    const float tB_C = -B * __builtin_amdgcn_rcpf(C), tB_A = -B * __builtin_amdgcn_rcpf(A), B2 = 2.0f * B;
    float dx0[4], dx1[4], ax[4], bx[4], tx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        dx0[k] = (float)(4 * k) - u; dx1[k] = (float)(4 * k + 3) - u;
        const float X = __builtin_amdgcn_fmed3f(0.0f, dx0[k], dx1[k]);
        ax[k] = A * X * X; bx[k] = B2 * X; tx[k] = tB_C * X;
    }
    uint32_t m = 0u;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float dy0 = (float)(4 * r) - v, dy1 = (float)(4 * r + 3) - v;
        const float Y = __builtin_amdgcn_fmed3f(0.0f, dy0, dy1);
        const float cy = C * Y * Y, by = B2 * Y, sy = tB_A * Y;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = __builtin_amdgcn_fmed3f(tx[k], dy0, dy1);          // minimiser of q on the line x = X, clamped to the rectangle
            const float qx = ax[k] + (bx[k] + C * t) * t;
            const float sc = __builtin_amdgcn_fmed3f(sy, dx0[k], dx1[k]);
            const float qy = cy + (by + A * sc) * sc;
            if (!(fminf(qx, qy) > chi_pad)) m |= 1u << (4 * r + k);             // NaN -> touched
        }
    }
    return (A > 0.f && C > 0.f && A * C - B * B > 0.f) ? m : 0xFFu;
}

// max of two wave-uniform counts as ONE s_max_i32
__device__ __forceinline__ int smax(int a, int b) {
    int r;
    asm("s_max_i32 %0, %1, %2" : "=s"(r) : "s"(a), "s"(b) : "scc");
    return r;
}

// MASK: 0 = box test, 1 = box and exact test, 2 = the mask the forward pass saved for this pair (c.saved_mask)
// Z: the record's camera depth is staged too (r2.z: the depth / opacity variants composite it as a fourth channel)
template <int MAXQ, int MASK = 0, class Lds = RasterLds, bool Z = false>
__device__ __forceinline__ Staged stage_chunk(Lds& s, const Candidate& c, int n, int lane, float ox, float oy, uint32_t& m8,
                                              uint64_t& ranks, float chi_pad = 0.f) {
    constexpr int QS = Lds::QSLOTS;                         // 16-byte pieces of the queue block
    static_assert(MAXQ >= CHUNK || MAXQ + 4 <= QS, "a capped queue is read up to MAXQ + 3");
    __syncthreads();       // previous chunk's LDS reads are done (single-wave block: orders LDS traffic only)
    m8 = 0u;
    if (lane == 63) { s.r0[CHUNK] = f4{0.f, 0.f, 0.f, 0.f}; s.r1[CHUNK] = f4{0.f, 0.f, 0.f, 0.f}; s.r2[CHUNK] = f4{0.f, 0.f, 0.f, 0.f}; }
    if (lane < n) {
        // conic pre-scaled by k = -0.5 log2(e): the loop evaluates q' = k q and alpha = o * exp2(q') (v_exp_f32 directly)
        s.r0[lane] = f4{c.q0.x, c.q0.y, QK * c.q0.z, (2.0f * QK) * c.q0.w};
        s.r1[lane] = f4{QK * c.q1.x, c.q1.y, c.q2.x, c.q2.y};
        s.r2[lane] = f4{c.q2.z, __uint_as_float(c.id), Z ? c.q2.w : 0.f, 0.f};
        if (MASK == 2) m8 = c.saved_mask;
        else if (MASK == 1) m8 = subtile_mask_exact(c, ox, oy, chi_pad);      // (conservative by itself: the box test adds nothing)
        else m8 = subtile_mask(c, ox, oy);
    }
    {   // every queue slot -> the null record (QCAP 16-byte pieces)
        const uint32_t nn = NULL_OFF | (NULL_OFF << 16);
        uint4* qv = reinterpret_cast<uint4*>(&s.q[0][0]);
        if (QS >= 64 || lane < QS) qv[lane] = uint4{nn, nn, nn, nn};
        if (QS > 64 && lane < QS - 64) qv[64 + lane] = uint4{nn, nn, nn, nn};
    }
    ranks = 0ull;
    if (MAXQ >= CHUNK) {                      // no cap (forward): queue entries written as the ballots come
        int maxc = 0;
#pragma unroll
        for (int t = 0; t < N_SUB; ++t) {
            const bool hit = (m8 >> t) & 1u;
            const unsigned long long b = __ballot(hit);
            if (hit) s.q[t][__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u))] = (uint16_t)(lane * 16);
            maxc = max(maxc, (int)__popcll(b));
        }
        __syncthreads();
        return Staged{n, maxc};
    }
    // (the bit tests are made ONCE: a queue is written under its ballot, cut to the entries taken -- scalar work where a second test of
    //  the bit cost two vector instructions per sub-tile; the longest queue is a scalar maximum, smax: left to itself the compiler moves
    //  the counts to VGPRs for a v_max3_u32)
    unsigned long long bal[N_SUB];
    int maxc = 0;
#pragma unroll
    for (int t = 0; t < N_SUB; ++t) {
        bal[t] = __ballot((m8 >> t) & 1u);
        maxc = smax(maxc, (int)__popcll(bal[t]));
    }
    while (maxc > MAXQ) {                 // rare (dense lists of large Gaussians): scalar work only
        n = max(n - 4, MAXQ);             // n = MAXQ always fits
        const unsigned long long keep = (1ull << n) - 1ull;
        maxc = 0;
#pragma unroll
        for (int t = 0; t < N_SUB; ++t) maxc = smax(maxc, (int)__popcll(bal[t] & keep));
    }
    const unsigned long long taken = n >= 64 ? ~0ull : (1ull << n) - 1ull;      // lanes [0, n)
    if (lane >= n) m8 = 0u;
#pragma unroll
    for (int t = 0; t < N_SUB; ++t) {
        if (__builtin_amdgcn_inverse_ballot_w64(bal[t] & taken)) {
            const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[t] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[t], 0u));
            s.q[t][r] = (uint16_t)(lane * 16);
            ranks |= (uint64_t)r << (8 * t);
        }
    }
    __syncthreads();
    return Staged{n, maxc};
}

template <class T>
__device__ __forceinline__ T lds_at(const T* base, uint32_t byte_off) {
    return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byte_off);
}

// ---- the pieces K6, K7 and K10 (gs_contrib.h) share: ONE copy each, so that "the same traversal" is the same code ---------------
// (with stage_chunk above.  Three pieces stay spelled out, because a shared copy changed the compiled kernels beyond register numbers
//  and the order of a few prologue instructions (DESIGN.md sections 21, 31): the two clock reads of the statistics and the slot
//  combine of K7 / K10 / K12, marked "(copy: ...)" where they stand, and the alpha of an entry, which has two spellings: K6's own,
//  and GS_WALK_WEIGHT for K10, K11 and K12.)

// Which pixels does `lane` own in `list`?  Group grp = lane >> 3 owns sub-tile (grp & 3, grp >> 2), lane j of it the pixels (px, pya)
// and (px, pyb = pya + 2); va / vb: inside the image; (ox, oy) = list origin; T = the initial transmittance (0 outside the image).
struct LanePixels { int tx, hy, grp, j, px, pya, pyb; bool va, vb; float fpx; v2f fpy; float ox, oy; v2f T; };
__device__ __forceinline__ LanePixels lane_pixels(uint32_t list, int lists_x, int lane, int H, int W) {
    LanePixels p;
    p.tx = list % lists_x; p.hy = list / lists_x;
    p.grp = lane >> 3; p.j = lane & 7;
    p.px = p.tx * LIST_W + (p.grp & 3) * 4 + (p.j & 3);
    p.pya = p.hy * LIST_H + (p.grp >> 2) * 4 + (p.j >> 2); p.pyb = p.pya + 2;
    p.va = (p.px < W) && (p.pya < H); p.vb = (p.px < W) && (p.pyb < H);
    p.fpx = (float)p.px;
    p.fpy = v2f{(float)p.pya, (float)p.pyb};
    p.ox = (float)(p.tx * LIST_W); p.oy = (float)(p.hy * LIST_H);
    p.T = v2f{p.va ? 1.0f : 0.0f, p.vb ? 1.0f : 0.0f};
    return p;
}

// Per-wave statistics (K6, K7): the record lane 0 stores at the wave's end, from the two clocks the kernel read at its start.
__device__ __forceinline__ WaveStats wave_stats_end(unsigned long long t_begin, unsigned long long t_real, uint2 rg, uint32_t chunks, uint32_t visited) {
    return WaveStats{rg.y - rg.x, (chunks & 0xFFFu) | ((uint32_t)(__builtin_amdgcn_s_memrealtime() - t_real) << 12), visited, (uint32_t)(__builtin_amdgcn_s_memtime() - t_begin), (uint32_t)t_real, blockIdx.x | (xcc_id() << 24)};
}

// min as ONE v_min_f32 (fminf() first canonicalises a scalar operand with a v_max_f32 every time it is used; no NaNs here)
// b is wave-uniform (a kernel argument): taken from its SGPR as src0, not copied to a VGPR first
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(b));
    return r;
}

// One queue entry against the lane's two pixels, "the forward's way" (K10, K11, K12; a = r0, b = r1 of the staged record): the
// weight w = alpha T, and T advances.  Reads fpx, fpy, chik, alpha_max, alpha_cutoff and T of the kernel around it.  K6 spells the
// same arithmetic for two entries interleaved and keeps that one spelling of its own (DESIGN.md sections 21, 31); this is the other.
#define GS_WALK_WEIGHT(a, b)                                                                                                 \
    const float du = fpx - (a).x;                                                                                            \
    const v2f dv = fpy - (a).y;                                                                                              \
    const v2f q = ((a).z * du * du) + dv * (((a).w * du) + (b).x * dv);                  /* k q  (k < 0) */                 \
    const bool i0 = q.x >= chik, i1 = q.y >= chik;                                        /* q <= chi */                     \
    v2f g;                                                                                                                   \
    g.x = __builtin_amdgcn_exp2f(q.x); g.y = __builtin_amdgcn_exp2f(q.y);                                                    \
    v2f al = (b).y * g;                                                                                                      \
    al.x = vmin(al.x, alpha_max); al.y = vmin(al.y, alpha_max);                                                              \
    al.x = (i0 && al.x >= alpha_cutoff && T.x > 5e-5f) ? al.x : 0.0f;      /* K6's one select: see there */                  \
    al.y = (i1 && al.y >= alpha_cutoff && T.y > 5e-5f) ? al.y : 0.0f;                                                        \
    const v2f w = al * T;                                                                                                    \
    T = T - al * T

// the first blocks of a launch (the longest lists) raise their wave priority (s_setprio takes a constant)
__device__ __forceinline__ void raise_launch_priority(uint32_t b, uint32_t grid) {
    const int prio = b * 64u < grid ? 3 : (b * 16u < grid ? 2 : (b * 4u < grid ? 1 : 0));
    if (prio == 3) __builtin_amdgcn_s_setprio(3);
    else if (prio == 2) __builtin_amdgcn_s_setprio(2);
    else if (prio == 1) __builtin_amdgcn_s_setprio(1);
}

// one layer's contribution w = alpha T (two pixels) to the running colour
__device__ __forceinline__ void add_colour(v2f& Cr, v2f& Cg, v2f& Cb, v2f w, float r, float g, float b) {
    Cr += w * r; Cg += w * g; Cb += w * b;
}

// (6 waves per SIMD as the compiler leaves it: 76 VGPRs.  Forced to 7 -- 69 VGPRs, no spill -- 90 us against 87.5; to 8: spills, 99 us)
// SAVE (a backward pass will follow: accum is given): the queues come from the exact ellipse / sub-tile test, which costs this
// kernel 6 us more than it saves it, and the resulting mask is left per pair (pair_mask, one byte) for the backward, which then
// needs no test of its own.
//
// AUX (gsplat_rasterize_forward_aux): depth and opacity beside the colour.  With w_i = alpha_i T_i [T_i > 5e-5] the wave also
// accumulates A = sum w_i and D = sum w_i z_i (z_i = the record's camera depth, staged in r2.z: no LDS more), two packed
// accumulators more; the pixel gets image = clamp(C + (1 - A) bg), depth = D, alpha = A (neither clamped nor normalised), and,
// for a backward pass, accum = C as always and accum_aux = (D, A).
struct AuxFwd {
    float* depth; float* alpha;      // [H,W] each, nullable (a background alone)
    float* accum_aux;                // [H,W,2]: (D, A) for the backward pass, given with accum
    float bg[3]; int has_bg;
};
// the composited, un-clamped colour: ONE fma, the same in the forward kernel and where the backward kernel rebuilds the clamp mask
__device__ __forceinline__ float over_background(float c, float a, float bg) { return __builtin_fmaf(1.0f - a, bg, c); }

template <bool SAVE, bool AUX = false>
__global__ __launch_bounds__(64) void raster_forward_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ ids,
                                                            const Rec64* __restrict__ rec, const uint32_t* __restrict__ order,
                                                            int lists_x, int H, int W, float chi, float alpha_max,
                                                            float alpha_cutoff, float* __restrict__ image,
                                                            float* __restrict__ accum, WaveStats* __restrict__ stats, uint32_t id_max,
                                                            float* __restrict__ zero_rows, int64_t n_zero_rows, uint8_t* __restrict__ pair_mask,
                                                            AuxFwd aux = AuxFwd{}) {
    __shared__ RasterLds s;
    const int lane = threadIdx.x;
    if (zero_rows) {        // the coming backward accumulates into grad2d: clear this wave's share now (the kernel is VALU-bound,
                            // the stores ride along; a separate 64 MB fill cost 10 us + a dependent launch)
        const int64_t per = (n_zero_rows + gridDim.x - 1) / gridDim.x, r0 = (int64_t)blockIdx.x * per;
        const int64_t r1 = r0 + per < n_zero_rows ? r0 + per : n_zero_rows;
        const f4 z = f4{0.f, 0.f, 0.f, 0.f};
        for (int64_t r = r0 + lane; r < r1; r += 64) {
            f4* row = reinterpret_cast<f4*>(zero_rows + r * 16);
            row[0] = z; row[1] = z; row[2] = z; row[3] = z;
        }
    }
    const uint32_t list = order[blockIdx.x];
    const LanePixels lp = lane_pixels(list, lists_x, lane, H, W);
    raise_launch_priority(blockIdx.x, gridDim.x);
    const unsigned long long t_begin = stats ? __builtin_amdgcn_s_memtime() : 0ull;              // (copy: K6, K7)
    const unsigned long long t_real = stats ? __builtin_amdgcn_s_memrealtime() : 0ull;      // 100 MHz, one clock for the whole chip
    uint32_t st_chunks = 0, st_visited = 0;
    const int px = lp.px;
    const float fpx = lp.fpx;
    const v2f fpy = lp.fpy;
    v2f T = lp.T;
    v2f Cr = {0.f, 0.f}, Cg = {0.f, 0.f}, Cb = {0.f, 0.f};
    v2f Dz = {0.f, 0.f}, Aw = {0.f, 0.f};                    // (AUX) sum w z, sum w
    const uint2 rg = ranges[list];
    const float chik = chi * QK;
    bool alive_any = __any(lp.va || lp.vb);
    uint32_t base = rg.x;
    Candidate cand;
    if (alive_any && base < rg.y) cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max);
    const uint16_t* myq = &s.q[lp.grp][0];
    while (alive_any && base < rg.y) {
        uint32_t m8;
        uint64_t ranks;
        const int maxc = stage_chunk<CHUNK, SAVE ? 1 : 0, RasterLds, AUX>(s, cand, (int)min(rg.y - base, (uint32_t)CHUNK), lane, lp.ox, lp.oy, m8, ranks, chi * 1.001f + 1e-4f).maxc;
        if (SAVE && base + (uint32_t)lane < rg.y) pair_mask[base + lane] = (uint8_t)m8;     // 64 contiguous bytes per chunk
        base += CHUNK;
        if (base < rg.y) cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max);   // in flight during the loop below
        ++st_chunks;
        st_visited += (uint32_t)maxc;
        // The queue's entries two at a time, every group its own queue; the terms join the running colour directly.  Every 16
        // entries the wave asks whether any pixel is still alive.
        for (int k0 = 0; k0 < maxc; k0 += 16) {
          const int k1 = min(k0 + 16, maxc);
          for (int k = k0; k < k1; k += 2) {
            const uint32_t offs = *reinterpret_cast<const uint32_t*>(myq + k);       // two queue entries
            const uint32_t o0 = offs & 0xFFFFu, o1 = offs >> 16;
            const f4 a0 = lds_at(s.r0, o0), b0 = lds_at(s.r1, o0), a1 = lds_at(s.r0, o1), b1 = lds_at(s.r1, o1);
            const float cb0 = lds_at(reinterpret_cast<const float*>(s.r2), o0), cb1 = lds_at(reinterpret_cast<const float*>(s.r2), o1);
            const float du0 = fpx - a0.x, du1 = fpx - a1.x;
            const v2f dv0 = fpy - a0.y, dv1 = fpy - a1.y;
            const v2f q0 = (a0.z * du0 * du0) + dv0 * ((a0.w * du0) + b0.x * dv0);        // k q  (k < 0)
            const v2f q1 = (a1.z * du1 * du1) + dv1 * ((a1.w * du1) + b1.x * dv1);
            const bool i00 = q0.x >= chik, i01 = q0.y >= chik, i10 = q1.x >= chik, i11 = q1.y >= chik;   // q <= chi
            v2f g0, g1;
            g0.x = __builtin_amdgcn_exp2f(q0.x); g0.y = __builtin_amdgcn_exp2f(q0.y);
            g1.x = __builtin_amdgcn_exp2f(q1.x); g1.y = __builtin_amdgcn_exp2f(q1.y);
            v2f al0 = b0.y * g0, al1 = b1.y * g1;
            al0.x = vmin(al0.x, alpha_max); al0.y = vmin(al0.y, alpha_max);
            al1.x = vmin(al1.x, alpha_max); al1.y = vmin(al1.y, alpha_max);
            // alpha = 0 outside the chi-square clip, below the cutoff, and on a dead pixel (T <= 5e-5: the term is masked, and a dead
            // pixel stays dead whether or not its T keeps shrinking) -- ONE select for the three, and w = alpha T needs none
            // (K6's own spelling, two entries interleaved; GS_WALK_WEIGHT above is the other, of K10 - K12 -- from a shared helper
            //  the compiler swaps the operands of this loop's s_and_b64)
            al0.x = (i00 && al0.x >= alpha_cutoff && T.x > 5e-5f) ? al0.x : 0.0f;
            al0.y = (i01 && al0.y >= alpha_cutoff && T.y > 5e-5f) ? al0.y : 0.0f;
            const v2f w0 = al0 * T;
            T = T - al0 * T;
            al1.x = (i10 && al1.x >= alpha_cutoff && T.x > 5e-5f) ? al1.x : 0.0f;
            al1.y = (i11 && al1.y >= alpha_cutoff && T.y > 5e-5f) ? al1.y : 0.0f;
            const v2f w1 = al1 * T;
            T = T - al1 * T;
            add_colour(Cr, Cg, Cb, w0, b0.z, b0.w, cb0);
            add_colour(Cr, Cg, Cb, w1, b1.z, b1.w, cb1);
            if (AUX) {
                const float z0 = lds_at(reinterpret_cast<const float*>(s.r2) + 2, o0), z1 = lds_at(reinterpret_cast<const float*>(s.r2) + 2, o1);
                Dz += w0 * z0; Aw += w0;
                Dz += w1 * z1; Aw += w1;
            }
          }
          if (!__any(T.x > 5e-5f || T.y > 5e-5f)) break;       // every 16 entries: all pixels dead
        }
        alive_any = __any(T.x > 5e-5f || T.y > 5e-5f);        // dead pixels stay dead
    }
    if (stats && lane == 0) stats[list] = wave_stats_end(t_begin, t_real, rg, st_chunks, st_visited);
    // One pixel: the clamped colour, and (a backward pass will follow) the colour before the clamp.  AUX: the colour lies over the
    // background before the clamp; depth and opacity as they are; for a backward pass C, D, A unclamped.
    const auto put = [&](int py, float r, float g, float b, float d, float a) {
        const int64_t p = (int64_t)py * W + px, o = p * 3;
        if constexpr (AUX) {
            if (accum) { accum[o + 0] = r; accum[o + 1] = g; accum[o + 2] = b; aux.accum_aux[p * 2] = d; aux.accum_aux[p * 2 + 1] = a; }
            if (aux.has_bg) { r = over_background(r, a, aux.bg[0]); g = over_background(g, a, aux.bg[1]); b = over_background(b, a, aux.bg[2]); }
        }
        image[o + 0] = fminf(fmaxf(r, 0.0f), 1.0f); image[o + 1] = fminf(fmaxf(g, 0.0f), 1.0f); image[o + 2] = fminf(fmaxf(b, 0.0f), 1.0f);
        if constexpr (AUX) {
            if (aux.depth) aux.depth[p] = d;
            if (aux.alpha) aux.alpha[p] = a;
        } else if (accum) { accum[o + 0] = r; accum[o + 1] = g; accum[o + 2] = b; }     // (plain: accum AFTER image on purpose -- the parent's instruction order)
    };
    if (lp.va) put(lp.pya, Cr.x, Cg.x, Cb.x, Dz.x, Aw.x);
    if (lp.vb) put(lp.pyb, Cr.y, Cg.y, Cb.y, Dz.y, Aw.y);
}

// x + y of a two-pixel value as ONE v_add_f32 the SLP vectoriser cannot see: left to itself it pairs these horizontal adds
// into v_pk_add_f32 and pays three v_mov shuffles per pair (-2.5 % on the backward kernel).
__device__ __forceinline__ float hadd(v2f a) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a.x), "v"(a.y));
    return r;
}

// Eight per-lane partial sums v[0..7] -> their totals over the lane's GROUP of 8 lanes, total i delivered in lane i of the
// group: a reduce-scatter inside every group at once (the 8 groups of the wave reduce 8 different Gaussians' sums in the
// same instructions).  Every level halves the number of live values while it sums over one more lane pairing:
//   row_half_mirror (l <-> 7 - l), quad_perm [2,3,0,1] (l <-> l ^ 2), quad_perm [1,0,3,2] (l <-> l ^ 1):
// levels 2 and 3: two selects and a DPP add per pair of values; level 1: two bank-masked DPP adds (17 instructions for 8 sums).
__device__ __forceinline__ float reduce_scatter8(float (&v)[8], int lane) {
    const bool b1 = lane & 2, b0 = lane & 1;
    // level 1 without selects: lane bit 2 is the parity of the lane's DPP bank (4 lanes), so two bank-masked DPP adds write the
    // two halves of the result: banks 0, 2 (lanes 0-3 of every group) get v[i] + mirror(v[i]), banks 1, 3 get v[i+4] + mirror(v[i+4])
    {
        float t0, t1, t2, t3;
        asm("s_nop 1\n"
            "v_add_f32_dpp %0, %4, %4 row_half_mirror row_mask:0xf bank_mask:0x5\n"
            "v_add_f32_dpp %1, %5, %5 row_half_mirror row_mask:0xf bank_mask:0x5\n"
            "v_add_f32_dpp %2, %6, %6 row_half_mirror row_mask:0xf bank_mask:0x5\n"
            "v_add_f32_dpp %3, %7, %7 row_half_mirror row_mask:0xf bank_mask:0x5\n"
            "v_add_f32_dpp %0, %8, %8 row_half_mirror row_mask:0xf bank_mask:0xa\n"
            "v_add_f32_dpp %1, %9, %9 row_half_mirror row_mask:0xf bank_mask:0xa\n"
            "v_add_f32_dpp %2, %10, %10 row_half_mirror row_mask:0xf bank_mask:0xa\n"
            "v_add_f32_dpp %3, %11, %11 row_half_mirror row_mask:0xf bank_mask:0xa"
            : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3)
            : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(v[4]), "v"(v[5]), "v"(v[6]), "v"(v[7]));
        v[0] = t0; v[1] = t1; v[2] = t2; v[3] = t3;
    }
    // levels 2, 3: per pair of values (a, b) and partner lane p, this lane keeps one of the two sums and gives the other to its
    // partner: keep = mine(kept) + partner's(given) -- two selects (1.3 ns each) and ONE DPP add (1.8 ns)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float keep = b1 ? v[i + 2] : v[i], give = b1 ? v[i] : v[i + 2];
        v[i] = keep + dpp<0x4E>(give);                                                    // quad_perm [2,3,0,1]
    }
    const float keep = b0 ? v[1] : v[0], give = b0 ? v[0] : v[1];
    return keep + dpp<0xB1>(give);                                                        // quad_perm [1,0,3,2]
}
// total of x over the lane's group of 8, in every lane of the group
__device__ __forceinline__ float all_reduce8(float x) {
    x += dpp<0x141>(x);                                                                     // row_half_mirror
    x += dpp<0x4E>(x);
    return x + dpp<0xB1>(x);
}

// backward: longest queue per chunk (sizes the slot block below; see the occupancy note at RasterLdsBwd).
constexpr int MAXQ_BWD = 24;                             // (even: the loop evaluates entries in pairs)
constexpr int QSLOTS_BWD = (MAXQ_BWD + 4 + 7) / 8 * 8;   // the loop reads entries k + 2, k + 3 ahead; rows of 16 bytes

// LDS of the backward kernel.  LDS float atomics are slow on this hardware (a ds_add_f32 wave-instruction with 64 lanes cost
// ~100 LDS cycles here: 230 us of a 450 us kernel), so nothing is accumulated with them: every group writes the nine sums of
// iteration k to its own slot (plain stores), and after the chunk each entry's lane adds up the slots of the sub-tiles it
// was queued in (it knows its rank in every queue) and leaves the row in `acc` for the flush.
// LDS per wave decides the occupancy here (12.8 KB -> 12 waves per CU): the chunk's rows `acc` [entry][9] reuse the record
// arrays, which are dead once the chunk's loop is over (the null record is rewritten by every stage_chunk).
using RasterLdsB = RasterLdsT<QSLOTS_BWD>;
template <bool DET, int NS = 9>              // NS = sums per (sub-tile, Gaussian): 9, or 10 with the depth / opacity channels (S_z)
struct RasterLdsBwd {
    float slots[N_SUB * MAXQ_BWD * NS];  // [sub-tile][queue position][NS sums]  (first: at LDS address 0 a slot's byte offset IS its address, and
                                         //  the ds_read2 of the gather, whose two offsets reach 255 words, need no base added per pair of sums)
    RasterLdsB f;
    uint32_t eoff[CHUNK];                // every entry's row of grad2d as an element offset: 16 x its Gaussian id (< 2^26, gs_layout.h)
    uint32_t eslot[DET ? CHUNK : 1];     // (deterministic mode) the row's slot
};
// LDS is handed out in coarse pieces (1280 B by the look of it): at 12 848 B per wave 11 waves were resident per CU (measured with
// tools/raster_stats.py: 2816 waves), at 12 608 B twelve (231 -> 221 us), at 11 456 B and 128 VGPRs fourteen (214 us); sixteen
// (queue cap 18: 10 KB) lose more to chunks cut short than they gain (228 us).
static_assert(sizeof(RasterLdsBwd<false>) <= 11520, "the backward kernel's LDS per wave decides its occupancy");
static_assert(sizeof(f4) * 3 * (CHUNK + 1) >= sizeof(float) * CHUNK * 12, "acc must fit into the record arrays");
// The depth / opacity variant (NS = 10) keeps the queue cap and runs at 3 waves per SIMD = 12 per CU, which 12 800 B each allow
static_assert(sizeof(RasterLdsBwd<true, 10>) <= 12800, "the depth / opacity backward kernel's LDS per wave: 12 waves per CU");
// The absolute-gradient variants (ABS: NS = 11, 12 with the depth / opacity channels) keep the queue cap, too.  Slots of 11 no longer fit
// the 14 waves of the plain kernel but do fit 12 800 B: 3 waves per SIMD = 12 per CU, like the depth / opacity variant.  Slots of 12 need
// 13 360 B = 11 of the 1280-byte pieces: 11 waves per CU by the granularity measured above (not measured on this variant).  A cap of 22 would buy the twelfth wave back; it is not taken: the frames
// that are both aux and absolute are rare, and one cap keeps the chunk cuts of all eight variants the same.
static_assert(sizeof(RasterLdsBwd<true, 11>) <= 12800, "the absolute-gradient backward kernel's LDS per wave: 12 waves per CU");
static_assert(sizeof(RasterLdsBwd<true, 12>) > 12800 && sizeof(RasterLdsBwd<true, 12>) <= 14080, "absolute-gradient + depth / opacity: 11 pieces of 1280 B, 11 waves per CU");

// K7: same traversal as K6 (identical T_i and alive decisions: lane_pixels, fetch_candidate and stage_chunk are K6's).  For pixel p
// and Gaussian i:
//   d alpha_i = alive_i T_i (c_i . Gc) - (sum_{k>i} w_k (c_k . Gc)) / (1 - alpha_i),
// the suffix sum being (total - running prefix), total = Gc . C_unclamped, Gc = dL/dO masked by the output clamp.
// Every group reduces its Gaussian's nine sums over its 8 lanes (reduce-scatter: 8 Gaussians at once in the same
// instructions); the rows of a chunk leave with ONE 36-byte global atomic request per (list, Gaussian) pair, 7 rows per
// instruction (the memory-side atomic units take ~20 G requests/s: per sub-tile requests would cost 3x the time).
//
// DET (deterministic gradients): float atomics add in arrival order, so gradients differ from run to run at the 1e-6 level.
// With DET the rows are STORED instead, one row per (list, Gaussian) pair at slot pair_base[Gaussian] + (ordinal of the list
// in the Gaussian's own rectangle), and pair_reduce_kernel adds each Gaussian's rows in that fixed order: bitwise
// reproducible (the sums inside a wave are already in a fixed order).
struct DetArgs {
    const u2* rect; const uint32_t* mask; const uint32_t* tiles; const uint32_t* pair_base;      // (tiles: read by nothing in K7; kept, so the arguments behind it stay where they are -- to go with a change that re-runs the ISA comparison anyway)
    float* part;             // [pair capacity][9] ([10] for the depth / opacity variant)
    uint32_t capacity;
};

//
// AUX (gsplat_rasterize_backward_aux): the loss also reads depth D = sum w z and opacity A = sum w, and the image may lie over a
// background: image = clamp(C + (1 - A) bg).  (z, 1) are two more colour channels: with c+ = (r, g, b, z, 1) and
// G+ = (Gr, Gg, Gb, G_D, G_A - sum_c G_c bg_c) -- G_c masked by the clamp of the COMPOSITED value -- the formula above holds with
// c+ . G+ for c . Gc and total = G+ . (C, D, A).  One sum more per pair: S_z = sum_px w G_D = dL/dz (column 9 of grad2d; slots and
// rows of 10, 6 rows per atomic instruction).  A missing upstream gradient (NULL) is zeros.
struct AuxBwd {
    const float* accum_aux;          // [H,W,2]: (D, A) unclamped, from the forward pass
    const float* gdepth; const float* galpha;      // [H,W] each, nullable
    float bg[3]; int has_bg;
};

//
// ABS (gsplat_rasterize_backward[_aux]_abs): the absolute-gradient densification statistic (AbsGS).  Two sums more
// per pair, over its pixels: Sx = sum |a (A11 du + A12 dv)|, Sy = sum |a (A12 du + A22 dv)| -- what |dL/du|, |dL/dv| of the projected
// centre are per pixel, up to the opacity, a factor the statistics kernel multiplies in once per Gaussian.  They land in columns 10
// and 11 of grad2d with and without AUX (column 9 stays S_z's).  The linear terms come from the staged conic, which is pre-scaled by k:
// |k x| = |k| |x|, so the pre-scaling is undone once per (list, Gaussian) row, where the chunk's slots are combined.
constexpr float INV_ABS_QK = 1.38629436111989061883f;      // 1 / |QK| = 2 ln 2
// the column of grad2d that sum v of a row of NS goes to: sums 9, 10 of a row without S_z skip column 9
template <bool AUX>
__device__ __forceinline__ constexpr int grad2d_column(int v) { return (!AUX && v >= 9) ? v + 1 : v; }
// |x.x| + |x.y| as ONE v_add_f32 (source modifiers; see hadd)
__device__ __forceinline__ float hadd_abs(v2f a) {
    float r;
    asm("v_add_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a.x), "v"(a.y));
    return r;
}

// (4 waves per SIMD: 93 VGPRs -- 128 while the gather kept a base address per pair of sums and sub-tile; with 10.8 KB of LDS 14 waves fit a CU.
//  AUX: 3 waves per SIMD -- up to 168 VGPRs, and the 12 waves of a CU may have 12.8 KB each: the slots of 10 with the same queue cap.
//  ABS: 3 waves per SIMD as well, see the static_asserts at RasterLdsBwd)
template <bool DET, bool AUX = false, bool ABS = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((AUX || ABS) ? 3 : 4, (AUX || ABS) ? 3 : 4))) void raster_backward_kernel(const uint2* __restrict__ ranges, const uint32_t* __restrict__ ids,
                                                             const Rec64* __restrict__ rec, const uint32_t* __restrict__ order,
                                                             int lists_x, int H, int W, float chi, float alpha_max,
                                                             float alpha_cutoff, const float* __restrict__ accum,
                                                             const float* __restrict__ gimg, float* __restrict__ grad2d,
                                                             WaveStats* __restrict__ stats, uint32_t id_max, DetArgs det,
                                                             const uint8_t* __restrict__ pair_mask, AuxBwd aux = AuxBwd{}) {
    constexpr int NS = (AUX ? 10 : 9) + (ABS ? 2 : 0);      // sums per (list, Gaussian) pair
    constexpr int RPI = 64 / NS;                   // rows per flush instruction
    __shared__ RasterLdsBwd<DET, NS> sb;
    RasterLdsB& s = sb.f;
    const int lane = threadIdx.x;
    const uint32_t list = order[blockIdx.x];
    const uint2 rg = ranges[list];
    if (rg.x >= rg.y) return;
    raise_launch_priority(blockIdx.x, gridDim.x);
    const unsigned long long t_begin = stats ? __builtin_amdgcn_s_memtime() : 0ull;              // (copy: K6, K7)
    const unsigned long long t_real = stats ? __builtin_amdgcn_s_memrealtime() : 0ull;      // 100 MHz, one clock for the whole chip
    uint32_t st_chunks = 0, st_visited = 0;
    const LanePixels lp = lane_pixels(list, lists_x, lane, H, W);
    const int tx = lp.tx, hy = lp.hy, grp = lp.grp, j = lp.j;
    const float fpx = lp.fpx;
    const v2f fpy = lp.fpy;
    v2f T = lp.T;
    // Upstream gradients of the lane's two pixels: g = (Gr, Gg, Gb, G_D, G_A - sum_c G_c bg_c), the last two AUX only, and the suffix
    // sum's start sfx = G+ . (C, D, A).  clamp(x, 0, 1) passes the gradient where 0 <= x <= 1 (render.py:410): x = C, or (AUX) what the
    // forward clamped, C over the background; gimg may be NULL in AUX only.
    // Every load a wave starts with is issued before the first is waited for: the first chunk's ids (fetch_candidate, the oldest, so that
    // its records can follow while the pixels' values arrive) and, per pixel, accum and gimg TOGETHER.  (gimg read only where the clamp
    // passes put each of the six gimg loads behind its accum value: eight dependent round trips in front of every wave's first chunk.)
    const bool alive_start = __any(lp.va || lp.vb);
    Candidate cand;
    if (alive_start) cand = fetch_candidate(lane, rg.x, rg.y, ids, rec, id_max, pair_mask);
    float g[2][5] = {}, sfx[2] = {0.f, 0.f};
    const bool vv[2] = {lp.va, lp.vb};
    const int py[2] = {lp.pya, lp.pyb};
    float cu[2][3] = {}, gi[2][3] = {};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (vv[k]) {
            const int64_t o = ((int64_t)py[k] * W + lp.px) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) cu[k][c] = accum[o + c];
            if (!AUX || gimg) {
#pragma unroll
                for (int c = 0; c < 3; ++c) gi[k][c] = gimg[o + c];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (vv[k]) {
            const int64_t p = (int64_t)py[k] * W + lp.px;
            float D = 0.f, A = 0.f;                               // (AUX) the pixel's depth and opacity sums from the forward pass
            if constexpr (AUX) {
                D = aux.accum_aux[p * 2]; A = aux.accum_aux[p * 2 + 1];
                g[k][3] = aux.gdepth ? aux.gdepth[p] : 0.0f;
                g[k][4] = aux.galpha ? aux.galpha[p] : 0.0f;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float shown = cu[k][c];                           // what the forward clamped
                if constexpr (AUX) { if (aux.has_bg) shown = over_background(cu[k][c], A, aux.bg[c]); }
                const float gv = (shown >= 0.0f && shown <= 1.0f) ? gi[k][c] : 0.0f;
                g[k][c] = gv;
                sfx[k] = __builtin_fmaf(gv, cu[k][c], sfx[k]);          // (spelled out: the three products of a pixel as ONE chain of fmas, whatever the vectoriser would pair)
                if constexpr (AUX) { if (aux.has_bg) g[k][4] -= gv * aux.bg[c]; }
            }
            if constexpr (AUX) sfx[k] += g[k][3] * D + g[k][4] * A;
        }
    }
    const v2f Gr = {g[0][0], g[1][0]}, Gg = {g[0][1], g[1][1]}, Gb = {g[0][2], g[1][2]};
    const v2f Gd = {g[0][3], g[1][3]}, Ga = {g[0][4], g[1][4]};          // (AUX; else 0) dL/dD, dL/dA - sum_c G_c bg_c
    v2f suffix = {sfx[0], sfx[1]};
    const float chik = chi * QK, amax = alpha_max;
    bool alive_any = alive_start;
    uint32_t base = rg.x;
    const int my_g = lane / NS, my_k = lane - NS * my_g;           // flush: lane i carries sum my_k of the round's row my_g
    const uint16_t* myq = &s.q[grp][0];
    float* const myslot = &sb.slots[grp * MAXQ_BWD * NS + j];      // + NS k: where lane j of the group puts sum j of iteration k
    float* const acc = reinterpret_cast<float*>(&sb.f);            // [entry][NS]: over the record arrays, between a chunk's loop and the next stage
    using Lds = RasterLdsBwd<DET, NS>;
    static_assert(offsetof(Lds, f) == sizeof(sb.slots), "acc = the record arrays begin where the slots end");
    float* const gcol = grad2d + (ABS ? grad2d_column<AUX>(my_k) : my_k);       // flush: the lane's column of row 0 of grad2d
    uint32_t arow_off = (uint32_t)(sizeof(sb.slots) + lane * NS * 4);       // entry `lane`'s row of acc (acc lies behind the slots), its
    asm("" : "+v"(arow_off));                                               // address kept whole like a slot's (see the gather)
    float* const arow = reinterpret_cast<float*>(reinterpret_cast<char*>(&sb) + arow_off);
    while (alive_any && base < rg.y) {
        uint32_t m8;
        uint64_t ranks;
        const Staged sg = stage_chunk<MAXQ_BWD, 2, RasterLdsB, AUX>(s, cand, (int)min(rg.y - base, (uint32_t)CHUNK), lane, lp.ox, lp.oy, m8, ranks);
        const int n = sg.n, maxc = sg.maxc;
        sb.eoff[lane] = cand.id * 16u;       // staged once per chunk: a flush round reads this one word per row and adds its column
        base += (uint32_t)n;
        if (base < rg.y) cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max, pair_mask);   // in flight during the loop below
        ++st_chunks;
        st_visited += (uint32_t)maxc;
        int kdone = 0;                       // iterations executed (uniform): slots [0, kdone) of every queue are valid
        // One queue entry: the group's 16 pixels against one Gaussian; the nine sums go to slot k of the group's queue.
        auto entry = [&](const f4& a, const f4& b, const float cbl, const float zl, const int k) {
            const float go = b.y;
            const float du = fpx - a.x;
            const v2f dv = fpy - a.y;
            const float c0 = a.z * du * du, c1 = a.w * du;
            const v2f q = c0 + dv * (c1 + b.x * dv);                                   // k q  (k < 0)
            const bool i0 = q.x >= chik, i1 = q.y >= chik;                              // q <= chi
            v2f g;
            g.x = __builtin_amdgcn_exp2f(q.x);
            g.y = __builtin_amdgcn_exp2f(q.y);
            const v2f og = go * g;
            // alpha = min(o g, alpha_max) where q <= chi and that is >= alpha_cutoff (<=> o g >= alpha_cutoff: cutoff <= alpha_max), else 0
            // (NOT folded with the alive test as in the forward kernel: alpha would then wait for the previous entry's T, and the
            //  chain alpha -> 1 / (1 - alpha) -> d alpha of two consecutive entries could no longer overlap: +7 us, measured)
            const bool p0 = i0 && og.x >= alpha_cutoff, p1 = i1 && og.y >= alpha_cutoff;
            const float cl0 = vmin(og.x, amax), cl1 = vmin(og.y, amax);                 // (unconditional: a select, not a branch)
            v2f al;
            al.x = p0 ? cl0 : 0.0f; al.y = p1 ? cl1 : 0.0f;
            const bool alive0 = T.x > 5e-5f, alive1 = T.y > 5e-5f;
            v2f w = al * T;
            w.x = alive0 ? w.x : 0.0f; w.y = alive1 ? w.y : 0.0f;
            v2f sdot = b.z * Gr + b.w * Gg + cbl * Gb;
            if (AUX) sdot += zl * Gd + Ga;                                 // c+ . G+
            const v2f ar = w * Gr, ag = w * Gg, ab = w * Gb;
            suffix -= w * sdot;                                            // now the sum over k > i
            const v2f sfx = suffix;
            v2f om = 1.0f - al;
            om.x = __builtin_amdgcn_rcpf(om.x); om.y = __builtin_amdgcn_rcpf(om.y);   // 1 - alpha >= 0.01
            v2f dal = T * sdot - sfx * om;
            // the pixel is alive, alpha passed its two tests, and clamp_max passes the gradient where o g <= alpha_max (render.py:372)
            dal.x = (alive0 && p0 && og.x <= alpha_max) ? dal.x : 0.0f;
            dal.y = (alive1 && p1 && og.y <= alpha_max) ? dal.y : 0.0f;
            // a = dL/d alpha * g.  dL/d opacity = sum a, and dL/dq = -0.5 o a: the factor -0.5 o is the same for all pixels of a
            // Gaussian, so the moments are taken of `a` and project_backward_kernel multiplies once per Gaussian:
            //   d u = o (A11 Mx + A12 My), d v = o (A12 Mx + A22 My), d A11 = -0.5 o Mxx, d A12 = -o Mxy, d A22 = -0.5 o Myy
            const v2f ao = dal * g;
            const v2f dva = dv * ao;
            const float m0 = hadd(ao), my = hadd(dva);
            float r[8];
            r[0] = du * m0;                                                // Mx  = sum du a
            r[1] = my;                                                     // My  = sum dv a
            r[2] = du * r[0];                                              // Mxx = sum du^2 a
            r[3] = du * my;                                                // Mxy = sum du dv a
            r[4] = hadd(dv * dva);                                         // Myy = sum dv^2 a
            r[5] = m0;                                                     // M0  = sum a = dL/d opacity
            r[6] = hadd(ar); r[7] = hadd(ag);                              // d r, d g
            const float tot_b = all_reduce8(hadd(ab));                     // d b
            myslot[k * NS] = reduce_scatter8(r, lane);
            if (j == 0) myslot[k * NS + 8] = tot_b;        // (two unconditional stores instead -- 3 instructions fewer -- measured no gain)
            if (AUX) {
                const float tot_z = all_reduce8(hadd(w * Gd));             // S_z = dL/dz
                if (j == 1) myslot[k * NS + 8] = tot_z;                    // (lane 1 of the group: slot index 9)
            }
            if constexpr (ABS) {
                // k (A11 du + A12 dv) = (k A11 du) + (k A12) dv and k (A12 du + A22 dv) = (k A12) du + (k A22) dv from the staged conic
                const float h = 0.5f * a.w;                                // k A12 (exact)
                const v2f lu = a.z * du + h * dv, lv = h * du + b.x * dv;
                const float tot_x = all_reduce8(hadd_abs(ao * lu));        // |k| Sx
                const float tot_y = all_reduce8(hadd_abs(ao * lv));        // |k| Sy
                if (j == NS - 10) myslot[k * NS + 8] = tot_x;              // (slot indices NS - 2, NS - 1)
                if (j == NS - 9) myslot[k * NS + 8] = tot_y;
            }
            T = T - al * T;
        };
        // Software pipeline over the queue (LDS latency is not covered by occupancy here: 3 waves per SIMD), two entries per step
        // in two register sets: entry k + 2 is requested into set 0 as soon as entry k has been evaluated from it, while entry
        // k + 1 is evaluated from set 1, and so on -- no register copies.  An odd queue ends on a null record (its slot gets zeros).
        const float* r2f = reinterpret_cast<const float*>(s.r2);
        uint32_t oo = *reinterpret_cast<const uint32_t*>(myq);
        f4 a0 = lds_at(s.r0, oo & 0xFFFFu), b0 = lds_at(s.r1, oo & 0xFFFFu), a1 = lds_at(s.r0, oo >> 16), b1 = lds_at(s.r1, oo >> 16);
        float cb0 = lds_at(r2f, oo & 0xFFFFu), cb1 = lds_at(r2f, oo >> 16);
        float z0 = 0.f, z1 = 0.f;
        if (AUX) { z0 = lds_at(r2f + 2, oo & 0xFFFFu); z1 = lds_at(r2f + 2, oo >> 16); }
        for (int k0 = 0; k0 < maxc; k0 += 8) {
          const int k1 = min(k0 + 8, maxc);
          for (int k = k0; k < k1; k += 2) {
            oo = *reinterpret_cast<const uint32_t*>(myq + k + 2);                       // entries k + 2, k + 3 (null past the end; k + 3 < QCAP)
            entry(a0, b0, cb0, z0, k);
            a0 = lds_at(s.r0, oo & 0xFFFFu); b0 = lds_at(s.r1, oo & 0xFFFFu); cb0 = lds_at(r2f, oo & 0xFFFFu);
            if (AUX) z0 = lds_at(r2f + 2, oo & 0xFFFFu);
            entry(a1, b1, cb1, z1, k + 1);
            a1 = lds_at(s.r0, oo >> 16); b1 = lds_at(s.r1, oo >> 16); cb1 = lds_at(r2f, oo >> 16);
            if (AUX) z1 = lds_at(r2f + 2, oo >> 16);
          }
          kdone = k1;
          if (!__any(T.x > 5e-5f || T.y > 5e-5f)) break;          // every 8 entries: all pixels dead
        }
        alive_any = __any(T.x > 5e-5f || T.y > 5e-5f);        // dead pixels stay dead
        __syncthreads();
        {   // entry `lane`: add up the slots of the sub-tiles it was queued in  (copy: K7, K10, K12 -- the loop over t, ranks and kdone)
            float tot[NS];
#pragma unroll
            for (int v = 0; v < NS; ++v) tot[v] = 0.f;
#pragma unroll
            for (int t = 0; t < N_SUB; ++t) {
                const int r = (int)((ranks >> (8 * t)) & 0xFFu);
                if (((m8 >> t) & 1u) && r < kdone) {
                    // The slot's byte offset as ONE v_mad_u32_u24, kept whole (the empty asm): the two offsets of a ds_read2 reach 255
                    // words, so the compiler, left to fold the constant part, forms a base per pair of sums -- 5 instructions per round.
                    // (The slots lie at LDS address 0 for the same reason: the offset is the address.)
                    uint32_t off = __umul24((uint32_t)r, NS * 4) + (uint32_t)(t * MAXQ_BWD * NS * 4);
                    asm("" : "+v"(off));
                    const float* p = reinterpret_cast<const float*>(reinterpret_cast<const char*>(sb.slots) + off);
#pragma unroll
                    for (int v = 0; v < NS; ++v) tot[v] += p[v];
                }
            }
            if constexpr (ABS) { tot[NS - 2] *= INV_ABS_QK; tot[NS - 1] *= INV_ABS_QK; }      // the conic's pre-scaling, undone once per row
#pragma unroll
            for (int v = 0; v < NS; ++v) arow[v] = tot[v];
        }
        if (DET && lane < n) {       // entry `lane`: its row's slot = first slot of its Gaussian + ordinal of this list in its rectangle
            const uint32_t id = sb.eoff[lane] >> 4;
            const u2 rc = det.rect[id];
            const uint32_t mk = det.mask[id];
            const int x0 = (int)(rc.x & 0xFFFFu), y0 = (int)(rc.x >> 16), x1 = (int)(rc.y & 0xFFFFu);
            const uint32_t bit = (uint32_t)((hy - y0) * (x1 - x0 + 1) + (tx - x0));          // row-major, like for_each_list
            uint32_t ord;
            if (rect_is_big(rc)) {               // a large Gaussian: its lists are row spans (for_each_big_row): lists in the rows above + offset in this row
                const Rec64* r = rec + id;
                const f4 q0 = r->r0, q1 = r->r1, q3 = r->pad;
                const float kk[4] = {q3.x, q3.y, q3.z, q3.w};
                const BigSpanK bk = big_span_setup(q0.x, q0.y, q1.z, q1.w, kk, x0, x1);
                ord = 0u;
                for (int y = y0; y < hy; ++y) {
                    const RowSpan sp = big_row_span(bk, y);
                    if (sp.xb >= sp.xa) ord += (uint32_t)(sp.xb - sp.xa + 1);
                }
                ord += (uint32_t)(tx - big_row_span(bk, hy).xa);
            } else {
                ord = (uint32_t)__popc(mk & ((1u << (bit & 31u)) - 1u));
            }
            sb.eslot[lane] = det.pair_base[id] + ord;
        }
        __syncthreads();
        // the chunk's rows -> grad2d: 7 rows x 9 sums per atomic instruction, one 36-byte request per row (AUX: 6 x 10, 40 bytes)
        for (int t0 = 0; t0 < n; t0 += RPI) {
            const int c = t0 + my_g;
            if (lane < RPI * NS && c < n) {
                const float val = acc[c * NS + my_k];
                if (DET) {
                    const uint32_t slot = sb.eslot[c];
                    if (slot < det.capacity) det.part[(int64_t)slot * NS + my_k] = val;
                } else if (val != 0.0f) {
                    atomicAdd(gcol + sb.eoff[c], val);
                }
            }
        }
    }
    if (stats && lane == 0) stats[list] = wave_stats_end(t_begin, t_real, rg, st_chunks, st_visited);
}

// ---- deterministic mode: slots of the (list, Gaussian) rows and their fixed-order sum ------------------------------------

__global__ __launch_bounds__(256) void tile_block_sum_kernel(int64_t n, const uint32_t* __restrict__ tiles, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t ws[4];
    uint32_t t = 0u;
    for (int k = 0; k < PB_BLOCK / 256; ++k) {
        const int64_t i = (int64_t)blockIdx.x * PB_BLOCK + k * 256 + threadIdx.x;
        t += i < n ? tiles[i] : 0u;
    }
    for (int sft = 32; sft > 0; sft >>= 1) t += (uint32_t)__shfl_xor((int)t, sft);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) block_sum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// pair_base[i] = number of rows of the Gaussians before i (exclusive scan of tiles[]): thread t of a block owns 8 CONSECUTIVE
// Gaussians, so the scan order is the index order.
__global__ __launch_bounds__(256) void pair_base_kernel(int64_t n, const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ block_sum,
                                                        uint32_t* __restrict__ pair_base) {
    __shared__ uint32_t ws[4], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t before = 0u;
    for (int b = tid; b < (int)blockIdx.x; b += 256) before += block_sum[b];
    for (int sft = 32; sft > 0; sft >>= 1) before += (uint32_t)__shfl_xor((int)before, sft);
    if (lane == 0) ws[wave] = before;
    __syncthreads();
    if (tid == 0) s_base = ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    constexpr int K = PB_BLOCK / 256;
    uint32_t v[K], run = 0u;
    const int64_t i0 = (int64_t)blockIdx.x * PB_BLOCK + (int64_t)tid * K;
#pragma unroll
    for (int k = 0; k < K; ++k) { v[k] = i0 + k < n ? tiles[i0 + k] : 0u; run += v[k]; }
    const uint32_t incl = wave_inclusive_scan(run);
    __syncthreads();
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    uint32_t st = s_base + incl - run;
    for (int k = 0; k < wave; ++k) st += ws[k];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (i0 + k < n) pair_base[i0 + k] = st;
        st += v[k];
    }
}

// grad2d[i][0..NS-1] = sum of Gaussian i's rows, in the order of its lists (row-major in its rectangle): the same order every run;
// columns NS .. 15 = 0.
// NS = floats per row: 9, or 10 behind the depth / opacity backward; 11 and 12 behind the absolute-gradient variants, whose rows of 11
// (GAP) have no S_z: their sums 9, 10 go to columns 10, 11 (grad2d_column), column 9 = 0.
template <int NS = 9, bool GAP = false>
__global__ __launch_bounds__(256) void pair_reduce_kernel(int64_t n, const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ pair_base,
                                                          const float* __restrict__ part, uint32_t capacity, float* __restrict__ grad2d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float t[NS];
#pragma unroll
    for (int v = 0; v < NS; ++v) t[v] = 0.f;
    const uint32_t nt = tiles[i], pb = pair_base[i];
    for (uint32_t k = 0; k < nt && pb + k < capacity; ++k) {
        const float* row = part + (int64_t)(pb + k) * NS;
#pragma unroll
        for (int v = 0; v < NS; ++v) t[v] += row[v];
    }
    float* o = grad2d + i * 16;
    if constexpr (GAP) {
        float full[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) full[v] = 0.f;
#pragma unroll
        for (int v = 0; v < NS; ++v) full[grad2d_column<false>(v)] = t[v];
#pragma unroll
        for (int v = 0; v < 16; ++v) o[v] = full[v];
        return;
    }
#pragma unroll
    for (int v = 0; v < NS; ++v) o[v] = t[v];
#pragma unroll
    for (int v = NS; v < 16; ++v) o[v] = 0.f;        // the whole row: deterministic mode never clears grad2d (a dirty one kept its padding)
}

}  // namespace
