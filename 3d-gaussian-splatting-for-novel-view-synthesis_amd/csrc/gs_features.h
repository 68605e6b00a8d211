// gs_features.h -- per-Gaussian feature vectors through the raster traversal: raster_features_kernel (K11) and its
// adjoint raster_features_adjoint_kernel (K12).
#pragma once
#include "gs_layout.h"
#include "gs_wave.h"
#include "gs_raster.h"

using namespace gsm;
namespace {

// With the blending weight w_i(p) = alpha_i T_i [T_i > 5e-5] of Gaussian i at pixel p, exactly as K6 forms it (same lists, launch
// order, two pixels per lane -- lane_pixels, fetch_candidate and stage_chunk of gs_raster.h are K6's own -- the sub-tile queues, the
// pre-scaled conic and exp2, the v_min against alpha_max, the one select, T = T - alpha T -- GS_WALK_WEIGHT of gs_raster.h, which
// K10 uses too -- and the 16-entry alive poll):
//     K11   F[p, c] = sum_i w_i(p) f_i[c]          features [n, C] -> out [H, W, C]
//     K12   g_i[c] += sum_p w_i(p) G[p, c]         grad_out [H, W, C] -> grad_features [n, C]   (adds)
// The weights do not depend on the features, so K12 walks the lists front to back like K11; there is no suffix sum.
//
// A wave takes one (list, channel group) pair: the group index is blockIdx.y, a group is FGROUP = 8 consecutive channels held in
// registers, and a table of C channels costs ceil(C / 8) traversals.  A partial last group (nch = C - c0 < 8) reads and writes
// nothing outside [0, C): its missing channels are zeros in registers.  `vec`: C is a multiple of 4 and the arrays are 16-byte
// aligned, so a full group's row is two 16-byte accesses; otherwise the row moves float by float.
constexpr int FGROUP = 8;

struct FeatRow { f4 lo, hi; };                         // the 8 channels of a group: one 32-byte row

__device__ __forceinline__ FeatRow load_row(const float* __restrict__ p, int nch, bool vec) {
    FeatRow r;
    if (vec && nch == FGROUP) {
        r.lo = *reinterpret_cast<const f4*>(p);
        r.hi = *reinterpret_cast<const f4*>(p + 4);
    } else {
        float v[FGROUP];
#pragma unroll
        for (int c = 0; c < FGROUP; ++c) v[c] = c < nch ? p[c] : 0.0f;
        r.lo = f4{v[0], v[1], v[2], v[3]};
        r.hi = f4{v[4], v[5], v[6], v[7]};
    }
    return r;
}

// the feature row of the lane's candidate (zeros beyond the list's end, like the candidate itself)
__device__ __forceinline__ FeatRow fetch_features(int lane, uint32_t base, uint32_t end, uint32_t id, const float* __restrict__ features,
                                                  int C, int c0, int nch, bool vec) {
    if (base + (uint32_t)lane < end) return load_row(features + (int64_t)id * C + c0, nch, vec);
    const f4 z = f4{0.f, 0.f, 0.f, 0.f};
    return FeatRow{z, z};
}

// K11's LDS: K6's records and queues, and the chunk's feature rows beside them -- 64 entries x one group = 2 KB; row e lies at twice
// the byte offset of record e, so a queue entry (a record offset) finds it with one shift; row CHUNK = zeros for the null record
// (w = 0 there, and 0 x the row must not be a NaN).
struct FeatLds {
    RasterLds f;
    f4 feat[(CHUNK + 1) * 2];
};
// 6.2 KB per wave: even 24 waves per CU would fit the CU's 160 KB; the VGPRs decide (4 waves per SIMD, see the kernel)
static_assert(sizeof(FeatLds) <= 6656, "the feature kernel's LDS per wave: no limit below 24 waves per CU");

// (4 waves per SIMD as the compiler leaves it: 118 VGPRs, no spill -- K6's 76, the 16 accumulators, the 16 feature values of the two
//  entries in flight and the 8 of the next chunk's row.  A fifth wave needs 102: not tried)
__global__ __launch_bounds__(64) void raster_features_kernel(
        const DevCounts* __restrict__ counts, long long capacity, const uint2* __restrict__ ranges, const uint32_t* __restrict__ ids,
        const Rec64* __restrict__ rec, const uint32_t* __restrict__ order, int lists_x, int H, int W, float chi, float alpha_max,
        float alpha_cutoff, uint32_t id_max, const float* __restrict__ features, int C, int vec, float* __restrict__ out) {
    if (counts->n_visible <= 0 || counts->n_binned > capacity) return;      // (uniform) nothing on screen, or lists that overflowed
    __shared__ FeatLds sf;
    RasterLds& s = sf.f;
    const int lane = threadIdx.x;
    const int c0 = (int)blockIdx.y * FGROUP, nch = min(FGROUP, C - c0);
    const uint32_t list = order[blockIdx.x];
    const uint2 rg = ranges[list];
    raise_launch_priority(blockIdx.x, gridDim.x);
    const LanePixels lp = lane_pixels(list, lists_x, lane, H, W);
    const float fpx = lp.fpx;
    const v2f fpy = lp.fpy;
    v2f T = lp.T;
    v2f acc[FGROUP];
#pragma unroll
    for (int c = 0; c < FGROUP; ++c) acc[c] = v2f{0.f, 0.f};
    const float chik = chi * QK;
    bool alive_any = __any(lp.va || lp.vb);
    uint32_t base = rg.x;
    Candidate cand;
    FeatRow frow;
    if (alive_any && base < rg.y) {
        cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max);
        frow = fetch_features(lane, base, rg.y, cand.id, features, C, c0, nch, vec);
    }
    if (lane == 63) { sf.feat[2 * CHUNK] = f4{0.f, 0.f, 0.f, 0.f}; sf.feat[2 * CHUNK + 1] = f4{0.f, 0.f, 0.f, 0.f}; }   // (stage_chunk's barriers follow)
    const uint16_t* myq = &s.q[lp.grp][0];
    while (alive_any && base < rg.y) {
        uint32_t m8;
        uint64_t ranks;
        const int n = (int)min(rg.y - base, (uint32_t)CHUNK);
        const int maxc = stage_chunk<CHUNK, 0, RasterLds, false>(s, cand, n, lane, lp.ox, lp.oy, m8, ranks).maxc;
        if (lane < n) { sf.feat[2 * lane] = frow.lo; sf.feat[2 * lane + 1] = frow.hi; }      // (behind stage_chunk's first barrier: the previous chunk's reads are done)
        __syncthreads();
        base += CHUNK;
        if (base < rg.y) {                                                                  // in flight during the loop below
            cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max);
            frow = fetch_features(lane, base, rg.y, cand.id, features, C, c0, nch, vec);
        }
        // one queue entry: the group's 16 pixels against one Gaussian; its 8 channels join the running sums
        auto entry = [&](const f4& a, const f4& b, const f4& f0, const f4& f1) {
            GS_WALK_WEIGHT(a, b);
            acc[0] += w * f0.x; acc[1] += w * f0.y; acc[2] += w * f0.z; acc[3] += w * f0.w;
            acc[4] += w * f1.x; acc[5] += w * f1.y; acc[6] += w * f1.z; acc[7] += w * f1.w;
        };
        for (int k0 = 0; k0 < maxc; k0 += 16) {
          const int k1 = min(k0 + 16, maxc);
          for (int k = k0; k < k1; k += 2) {
            const uint32_t offs = *reinterpret_cast<const uint32_t*>(myq + k);       // two queue entries (an odd queue ends on the null record)
            const uint32_t o0 = offs & 0xFFFFu, o1 = offs >> 16;
            const f4 a0 = lds_at(s.r0, o0), b0 = lds_at(s.r1, o0), a1 = lds_at(s.r0, o1), b1 = lds_at(s.r1, o1);
            const f4 f00 = lds_at(sf.feat, 2u * o0), f01 = lds_at(sf.feat, 2u * o0 + 16u);
            const f4 f10 = lds_at(sf.feat, 2u * o1), f11 = lds_at(sf.feat, 2u * o1 + 16u);
            entry(a0, b0, f00, f01);
            entry(a1, b1, f10, f11);
          }
          if (!__any(T.x > 5e-5f || T.y > 5e-5f)) break;       // every 16 entries: all pixels dead
        }
        alive_any = __any(T.x > 5e-5f || T.y > 5e-5f);        // dead pixels stay dead
    }
    // every pixel inside the image, every channel of the group: zeros where nothing reached it
    const auto put = [&](int py, const float (&v)[FGROUP]) {
        float* p = out + ((int64_t)py * W + lp.px) * C + c0;
        if (vec && nch == FGROUP) {
            *reinterpret_cast<f4*>(p) = f4{v[0], v[1], v[2], v[3]};
            *reinterpret_cast<f4*>(p + 4) = f4{v[4], v[5], v[6], v[7]};
        } else {
#pragma unroll
            for (int c = 0; c < FGROUP; ++c)
                if (c < nch) p[c] = v[c];
        }
    };
    float va[FGROUP], vb[FGROUP];
#pragma unroll
    for (int c = 0; c < FGROUP; ++c) { va[c] = acc[c].x; vb[c] = acc[c].y; }
    if (lp.va) put(lp.pya, va);
    if (lp.vb) put(lp.pyb, vb);
}

// K12.  The lane holds G of its two pixels for the group's 8 channels; per queue entry it forms w G[c] for both pixels, the 8 lanes of
// a sub-tile reduce the eight sums in one reduce_scatter8 -- channel j ends in lane j of the group, which a group of eight fits
// exactly -- and every sub-tile writes its row to its own slot with plain LDS stores (no LDS atomics: see the note above
// RasterLdsBwd).  After the chunk entry `lane` combines the slots of the sub-tiles it was queued in, in sub-tile order, and the rows
// leave with float atomicAdd, 8 rows x 8 channels per instruction: the eight floats of a (list, Gaussian) pair are one contiguous
// 32-byte piece of grad_features.  A zero is never added, so a pair whose weights are all zero -- everything behind early termination
// included -- issues no atomic, and the row of a Gaussian in no list is never touched.  Float atomics add in arrival order: there is no
// deterministic twin of this kernel.
//
// The slots decide the queue cap and the occupancy: 8 sub-tiles x 24 entries x 8 channels = 6 KB at K7's cap of 24.
constexpr int MAXQ_FTA = MAXQ_BWD;
struct FeatAdjLds {
    float slots[N_SUB * MAXQ_FTA * FGROUP];              // [sub-tile][queue position][channel]
    RasterLdsB f;                                        // (the chunk's rows reuse the record arrays, dead once the chunk's loop is over)
    uint32_t eid[CHUNK];                                 // every entry's Gaussian id
};
// 9.8 KB per wave: 16 waves per CU = 4 per SIMD, the target below
static_assert(sizeof(FeatAdjLds) <= 10240, "the feature adjoint's LDS per wave: 16 waves per CU");
static_assert(sizeof(f4) * 3 * (CHUNK + 1) >= sizeof(float) * CHUNK * FGROUP, "the chunk's rows must fit into the record arrays");

// (4 waves per SIMD: LDS allows no more, and up to 128 VGPRs are then free; 83 used, no spill)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void raster_features_adjoint_kernel(
        const DevCounts* __restrict__ counts, long long capacity, const uint2* __restrict__ ranges, const uint32_t* __restrict__ ids,
        const Rec64* __restrict__ rec, const uint32_t* __restrict__ order, int lists_x, int H, int W, float chi, float alpha_max,
        float alpha_cutoff, uint32_t id_max, const float* __restrict__ grad_out, int C, int vec, float* __restrict__ grad_features) {
    if (counts->n_visible <= 0 || counts->n_binned > capacity) return;      // (uniform) nothing on screen, or lists that overflowed
    __shared__ FeatAdjLds sa;
    RasterLdsB& s = sa.f;
    const int lane = threadIdx.x;
    const int c0 = (int)blockIdx.y * FGROUP, nch = min(FGROUP, C - c0);
    const uint32_t list = order[blockIdx.x];
    const uint2 rg = ranges[list];
    if (rg.x >= rg.y) return;
    raise_launch_priority(blockIdx.x, gridDim.x);
    const LanePixels lp = lane_pixels(list, lists_x, lane, H, W);
    const int grp = lp.grp, j = lp.j;
    const float fpx = lp.fpx;
    const v2f fpy = lp.fpy;
    v2f T = lp.T;
    const float chik = chi * QK;
    bool alive_any = __any(lp.va || lp.vb);
    uint32_t base = rg.x;
    Candidate cand;
    if (alive_any) cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max);
    // upstream values of the lane's two pixels (zeros outside the image and beyond the group's channels)
    v2f G[FGROUP];
    {
        const f4 z = f4{0.f, 0.f, 0.f, 0.f};
        FeatRow ga = FeatRow{z, z}, gb = FeatRow{z, z};
        if (lp.va) ga = load_row(grad_out + ((int64_t)lp.pya * W + lp.px) * C + c0, nch, vec);
        if (lp.vb) gb = load_row(grad_out + ((int64_t)lp.pyb * W + lp.px) * C + c0, nch, vec);
        G[0] = v2f{ga.lo.x, gb.lo.x}; G[1] = v2f{ga.lo.y, gb.lo.y}; G[2] = v2f{ga.lo.z, gb.lo.z}; G[3] = v2f{ga.lo.w, gb.lo.w};
        G[4] = v2f{ga.hi.x, gb.hi.x}; G[5] = v2f{ga.hi.y, gb.hi.y}; G[6] = v2f{ga.hi.z, gb.hi.z}; G[7] = v2f{ga.hi.w, gb.hi.w};
    }
    const uint16_t* myq = &s.q[grp][0];
    float* const myslot = &sa.slots[grp * MAXQ_FTA * FGROUP + j];      // + 8 k: where lane j of the group puts channel j of iteration k
    float* const rows = reinterpret_cast<float*>(&sa.f);               // [entry][8]: over the record arrays, between a chunk's loop and the next stage
    float* const gcol = grad_features + c0 + j;                        // flush: the lane's channel of row 0
    while (alive_any && base < rg.y) {
        uint32_t m8;
        uint64_t ranks;
        const Staged sg = stage_chunk<MAXQ_FTA, 0, RasterLdsB, false>(s, cand, (int)min(rg.y - base, (uint32_t)CHUNK), lane, lp.ox, lp.oy, m8, ranks);
        const int n = sg.n, maxc = sg.maxc;
        sa.eid[lane] = cand.id;
        base += (uint32_t)n;
        if (base < rg.y) cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max);   // in flight during the loop below
        int kdone = 0;                       // iterations executed (uniform): slots [0, kdone) of every queue are valid
        // one queue entry: the group's 16 pixels against one Gaussian; the eight sums go to slot k of the group's queue
        auto entry = [&](const f4& a, const f4& b, const int k) {
            GS_WALK_WEIGHT(a, b);
            float r[FGROUP];
#pragma unroll
            for (int c = 0; c < FGROUP; ++c) r[c] = hadd(w * G[c]);
            myslot[k * FGROUP] = reduce_scatter8(r, lane);
        };
        for (int k0 = 0; k0 < maxc; k0 += 16) {
          const int k1 = min(k0 + 16, maxc);
          for (int k = k0; k < k1; k += 2) {
            const uint32_t offs = *reinterpret_cast<const uint32_t*>(myq + k);       // two queue entries (an odd queue ends on the null record)
            const uint32_t o0 = offs & 0xFFFFu, o1 = offs >> 16;
            const f4 a0 = lds_at(s.r0, o0), b0 = lds_at(s.r1, o0), a1 = lds_at(s.r0, o1), b1 = lds_at(s.r1, o1);
            entry(a0, b0, k);
            entry(a1, b1, k + 1);
          }
          kdone = k1;
          if (!__any(T.x > 5e-5f || T.y > 5e-5f)) break;       // every 16 entries: all pixels dead
        }
        alive_any = __any(T.x > 5e-5f || T.y > 5e-5f);        // dead pixels stay dead
        __syncthreads();
        {   // entry `lane`: add up the slots of the sub-tiles it was queued in  (copy: K7, K10, K12 -- the loop over t, ranks and kdone)
            f4 lo = f4{0.f, 0.f, 0.f, 0.f}, hi = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < N_SUB; ++t) {
                const int r = (int)((ranks >> (8 * t)) & 0xFFu);
                if (((m8 >> t) & 1u) && r < kdone) {
                    const f4* p = reinterpret_cast<const f4*>(&sa.slots[(t * MAXQ_FTA + r) * FGROUP]);
                    const f4 x = p[0], y = p[1];
                    lo.x += x.x; lo.y += x.y; lo.z += x.z; lo.w += x.w;
                    hi.x += y.x; hi.y += y.y; hi.z += y.z; hi.w += y.w;
                }
            }
            f4* const row = reinterpret_cast<f4*>(rows + lane * FGROUP);
            row[0] = lo; row[1] = hi;
        }
        __syncthreads();
        // the chunk's rows -> grad_features: 8 rows x 8 channels per atomic instruction, one 32-byte piece per row
        for (int t0 = 0; t0 < n; t0 += 64 / FGROUP) {
            const int e = t0 + grp;
            if (e < n && j < nch) {
                const float val = rows[e * FGROUP + j];
                if (val != 0.0f) atomicAdd(gcol + (int64_t)sa.eid[e] * C, val);
            }
        }
    }
}

}  // namespace
