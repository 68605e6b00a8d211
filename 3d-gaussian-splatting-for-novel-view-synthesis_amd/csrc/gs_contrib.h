// gs_contrib.h -- per-Gaussian contribution statistics: raster_contrib_kernel.
#pragma once
#include "gs_layout.h"
#include "gs_wave.h"
#include "gs_raster.h"

using namespace gsm;
namespace {

// K10: the forward kernel's traversal (same lists, launch order, two pixels per lane -- lane_pixels, fetch_candidate and stage_chunk
// of gs_raster.h are K6's own -- the sub-tile queues, the same alpha and T = T - alpha T (GS_WALK_WEIGHT), the same 16-entry alive poll) without
// colours and without an image.  What leaves the wave is,
// per (list, Gaussian) pair, the blending weight w = alpha T [T > 5e-5] of the pair's <= 128 pixels as
//     (sum of w, max of w, number of pixels with w > 0).
// A record is one 16-byte row per Gaussian, four 32-bit words, every one an order-independent integer:
//     words 0-1   uint64 sum_q (little endian), units of 2^-32: every pair adds round_to_nearest_even(pair_sum * 2^32);
//                 pair_sum < 2^7, so a term is below 2^39 and 2^25 of them fit
//     word 2      the float32 bits of weight_max (non-negative floats order like their bit patterns: an unsigned max)
//     word 3      uint32 pixels (wraps after 2^32 pixel hits; not guarded)
// Integer add and max commute exactly: the record is bitwise the same whatever order waves, streams, views or ranks arrive in,
// so two streams may add into one record, and there is no deterministic twin of this kernel.
//
// Inside the wave the order is fixed: a lane adds its two pixels, the 8 lanes of a sub-tile reduce in the DPP tree of all_reduce8
// ((l, 7 - l), then l ^ 2, then l ^ 1), every sub-tile writes its three values to its own slot with plain LDS stores (no LDS atomics:
// see the note above RasterLdsBwd), and after the chunk entry `lane` combines the slots of the sub-tiles it was queued in, in
// sub-tile index order.  The flush is integer global atomics, none returning: per pair an 8-byte add of sum_q and an 8-byte add of
// (pixels << 32) on words 2-3 -- two lanes of one instruction, one 16-byte request -- and a 4-byte max where it can raise word 2; a
// pair whose pixel count is 0 -- everything behind early termination included -- issues no memory operation, and the row of a
// Gaussian in no list is never touched.
//
// The queues need each entry's rank, which stage_chunk computes on its capped path only: the cap is 60 of the chunk's 64 entries, so a
// chunk is cut only where 61+ of its entries reach one sub-tile (the uncut and the cut traversal give the same w term by term).
constexpr int MAXQ_CTB = 60;                             // (even: the loop evaluates entries in pairs)
constexpr int QSLOTS_CTB = 64;                           // the loop reads entry k + 1; stage_chunk wants MAXQ + 4 slots
using RasterLdsC = RasterLdsT<QSLOTS_CTB>;
struct ContribLds {
    RasterLdsC f;
    uint32_t slots[N_SUB * MAXQ_CTB * 3];                // [sub-tile][queue position](sum bits, max bits, count)
};
// 9.9 KB per wave: 16 waves per CU = 4 per SIMD, the target below
static_assert(sizeof(ContribLds) <= 10240, "the contribution kernel's LDS per wave: 16 waves per CU");

__device__ __forceinline__ float all_reduce8_max(float x) {
    x = __builtin_fmaxf(x, dpp<0x141>(x));                                                 // row_half_mirror
    x = __builtin_fmaxf(x, dpp<0x4E>(x));
    return __builtin_fmaxf(x, dpp<0xB1>(x));
}

// (4 waves per SIMD: LDS allows no more, and up to 128 VGPRs are then free)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void raster_contrib_kernel(
        const DevCounts* __restrict__ counts, long long capacity, const uint2* __restrict__ ranges, const uint32_t* __restrict__ ids,
        const Rec64* __restrict__ rec, const uint32_t* __restrict__ order, int lists_x, int H, int W, float chi, float alpha_max,
        float alpha_cutoff, uint32_t id_max, uint32_t* __restrict__ record) {
    if (counts->n_visible <= 0 || counts->n_binned > capacity) return;      // (uniform) nothing on screen, or lists that overflowed
    __shared__ ContribLds sc;
    RasterLdsC& s = sc.f;
    const int lane = threadIdx.x;
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
    const uint16_t* myq = &s.q[grp][0];
    uint32_t* const myslot = &sc.slots[grp * MAXQ_CTB * 3 + j];     // + 3 k: where lanes 0-2 of the group put the values of iteration k
    const int gsh = grp * 8;
    while (alive_any && base < rg.y) {
        uint32_t m8;
        uint64_t ranks;
        const Staged sg = stage_chunk<MAXQ_CTB, 0, RasterLdsC, false>(s, cand, (int)min(rg.y - base, (uint32_t)CHUNK), lane, lp.ox, lp.oy, m8, ranks);
        const int maxc = sg.maxc;
        const uint32_t my_id = cand.id;
        base += (uint32_t)sg.n;
        if (base < rg.y) cand = fetch_candidate(lane, base, rg.y, ids, rec, id_max);   // in flight during the loop below
        int kdone = 0;                       // iterations executed (uniform): slots [0, kdone) of every queue are valid
        // one queue entry: the group's 16 pixels against one Gaussian; (sum, max, count) go to slot k of the group's queue
        auto entry = [&](const f4& a, const f4& b, const int k) {
            GS_WALK_WEIGHT(a, b);                                     // w of the two pixels; T advances (gs_raster.h: K11 and K12 use the same)
            const float sum = all_reduce8(hadd(w));
            const float mx = all_reduce8_max(__builtin_fmaxf(w.x, w.y));
            const unsigned long long bx = __ballot(w.x > 0.0f), by = __ballot(w.y > 0.0f);
            const uint32_t cnt = (uint32_t)__popc((uint32_t)(bx >> gsh) & 0xFFu) + (uint32_t)__popc((uint32_t)(by >> gsh) & 0xFFu);
            const uint32_t val = j == 0 ? __float_as_uint(sum) : (j == 1 ? __float_as_uint(mx) : cnt);
            if (j < 3) myslot[k * 3] = val;
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
        // entry `lane`: combine the slots of the sub-tiles it was queued in, in sub-tile order; one row per pair leaves the wave
        // (copy: K7, K10, K12 -- the loop over t, ranks and kdone)
        float tot = 0.0f, mx = 0.0f;
        uint32_t cnt = 0u;
#pragma unroll
        for (int t = 0; t < N_SUB; ++t) {
            const int r = (int)((ranks >> (8 * t)) & 0xFFu);
            if (((m8 >> t) & 1u) && r < kdone) {
                const uint32_t* p = &sc.slots[(t * MAXQ_CTB + r) * 3];
                tot += __uint_as_float(p[0]);
                mx = __builtin_fmaxf(mx, __uint_as_float(p[1]));
                cnt += p[2];
            }
        }
        // The flush.  The memory-side atomic units are paid per REQUEST -- the lanes of one instruction that fall into one row (the note at
        // K7) -- so the 8-byte add of sum_q and the add of the pixel count leave as the two halves of ONE 16-byte request: two lanes per
        // pair in one 8-byte-add instruction, the second adding (pixels << 32) to words 2-3 (word 2 gets + 0, which never carries; word 3
        // wraps like a uint32).  The rows travel through LDS, over the record array r0 (dead once the chunk's loop is over; the next
        // stage_chunk begins with a barrier).  The maximum is issued only where it can still raise word 2: the value read may be stale,
        // but word 2 only grows, so a stale read costs an atomic that changes nothing and never skips one that would.
        // Word 2 is thus reached by accesses of three kinds: the low half of the 8-byte add on words 2-3 (+ 0), the 4-byte max and the
        // 4-byte load.  The kernel relies on the L2 atomic units serialising accesses of different widths to the same bytes, which this
        // hardware does and the C++ / HIP memory model does not promise.
        uint4* const rows = reinterpret_cast<uint4*>(&s.r0[0]);
        const unsigned long long qv = cnt > 0u ? (unsigned long long)__builtin_rintf(tot * 4294967296.0f) : 0ull;
        rows[lane] = uint4{(uint32_t)qv, (uint32_t)(qv >> 32), my_id, cnt};
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint4 row = rows[32 * h + (lane >> 1)];
            if (row.w > 0u) {
                const unsigned long long v = (lane & 1) ? ((unsigned long long)row.w << 32) : ((unsigned long long)row.x | ((unsigned long long)row.y << 32));
                atomicAdd(reinterpret_cast<unsigned long long*>(record + (int64_t)row.z * 4) + (lane & 1), v);
            }
        }
        if (cnt > 0u) {
            uint32_t* wm = record + (int64_t)my_id * 4 + 2;
            if (__float_as_uint(mx) > __hip_atomic_load(wm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(wm, __float_as_uint(mx));
        }
    }
}

}  // namespace
