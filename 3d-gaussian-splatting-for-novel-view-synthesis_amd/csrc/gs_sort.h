// gs_sort.h -- K5 plan (launch order of the lists) and K4 per-list depth sort.
#pragma once
#include "gs_layout.h"
#include "gs_wave.h"

using namespace gsm;
namespace {

// ---- K5: plan ----------------------------------------------------------------------------------------
// Longest-processing-time-first launch order of the lists (1/8-octave buckets of the list length: the raster kernels
// are tail-bound, a few dense lists take 5x the mean, so they must start first), and the boundaries of the sort size
// classes inside that order.
__device__ __forceinline__ uint32_t work_bucket(uint32_t w) {
    if (w < 8u) return w;
    const uint32_t e = 31u - (uint32_t)__clz((int)w);
    return (e - 2u) * 8u + ((w >> (e - 3u)) & 7u);          // <= 239; 256 -> 48, 1024 -> 64, 4096 -> 80, 8192 -> 88
}
constexpr int SORT_CLASSES = 4;                               // list length >= 4096 | >= 1024 | >= 256 | >= 1
__device__ __forceinline__ uint32_t class_first_bucket(int c) { return c == 0 ? 80u : (c == 1 ? 64u : (c == 2 ? 48u : 1u)); }

// Counting sort of the lists by work bucket, descending.  Same-address LDS atomics serialise and neighbouring lists
// often share a bucket, so every bucket has 16 sub-counters selected by the lane (flat index = (255 - bucket) * 16 + sub:
// ascending flat index = descending bucket).
template <int THREADS, class Len>
__device__ __forceinline__ void plan_body(int nl, Len len, uint32_t* __restrict__ order, uint32_t* __restrict__ class_bounds,
                                          uint32_t* cnt, uint32_t* wsum) {
    constexpr int SUB = 16, NF = 256 * SUB, K = 16384 / THREADS, CPT = NF / THREADS;
    // K lists per thread and round, held in registers; CPT counters per thread in the scan
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = tid & (SUB - 1);
    for (int f = tid; f < NF; f += THREADS) cnt[f] = 0u;
    __syncthreads();
    const bool one_round = nl <= THREADS * K;
    uint32_t flat[K];                                          // counter index of list (round base + k * THREADS + tid), or ~0
    for (int base = 0; base < nl; base += THREADS * K) {
        uint32_t w[K];
#pragma unroll
        for (int k = 0; k < K; ++k) w[k] = base + k * THREADS + tid < nl ? len(base + k * THREADS + tid) : 0u;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            flat[k] = base + k * THREADS + tid < nl ? (255u - work_bucket(w[k])) * SUB + sub : 0xFFFFFFFFu;
            if (flat[k] != 0xFFFFFFFFu) atomicAdd(&cnt[flat[k]], 1u);
        }
    }
    __syncthreads();
    // exclusive prefix over the NF counters: thread t owns CPT consecutive ones
    uint32_t c[CPT], run = 0u;
#pragma unroll
    for (int k = 0; k < CPT; ++k) { c[k] = cnt[tid * CPT + k]; run += c[k]; }
    const uint32_t incl = wave_inclusive_scan(run);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t st = incl - run;
    for (int k = 0; k < wave; ++k) st += wsum[k];
#pragma unroll
    for (int k = 0; k < CPT; ++k) { cnt[tid * CPT + k] = st; st += c[k]; }
    __syncthreads();
    // lists in buckets >= first bucket of a class = prefix at the first sub-counter of the bucket below it
    if (tid < SORT_CLASSES) class_bounds[tid] = cnt[(256u - class_first_bucket(tid)) * SUB];
    __syncthreads();
    for (int base = 0; base < nl; base += THREADS * K) {
        if (!one_round) {                                      // more than 16384 lists: recompute the counter indices
            uint32_t w[K];
#pragma unroll
            for (int k = 0; k < K; ++k) w[k] = base + k * THREADS + tid < nl ? len(base + k * THREADS + tid) : 0u;
#pragma unroll
            for (int k = 0; k < K; ++k)
                flat[k] = base + k * THREADS + tid < nl ? (255u - work_bucket(w[k])) * SUB + sub : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (flat[k] != 0xFFFFFFFFu) order[atomicAdd(&cnt[flat[k]], 1u)] = (uint32_t)(base + k * THREADS + tid);
    }
}
constexpr int PLAN_LDS_WORDS = 256 * 16 + 16;

// the plan by itself: only when there is nothing to bin (all ranges empty)
__global__ __launch_bounds__(1024) void plan_kernel(int nl, const uint2* __restrict__ ranges, uint32_t* __restrict__ order,
                                                    uint32_t* __restrict__ class_bounds) {
    __shared__ uint32_t lds[PLAN_LDS_WORDS];
    plan_body<1024>(nl, [&](int l) { const uint2 r = ranges[l]; return r.y - r.x; }, order, class_bounds, lds, lds + 256 * 16);
}

// ---- K4: per-list depth sort ------------------------------------------------------------------------
// One workgroup per list sorts the list's payloads ascending = (depth, Gaussian index) order and writes the ids.
// Keys are unique, so the result does not depend on the arrival order of the scatter.
//
// list_sort_kernel (lists shorter than T * E): one-pass distribution sort in LDS.  The depth bits (monotone in z) are
// mapped to B >= 2 n buckets by subtracting the list minimum and shifting; count (LDS atomics) -> exclusive scan ->
// scatter gives bucket order; inside a bucket (expected occupancy <= 0.5) every element counts the smaller keys to find
// its rank.  ~8 barriers instead of the ~70 compare-exchange rounds of a bitonic network.  A list whose depths are so
// clustered that a bucket holds more than DENSE_BUCKET entries takes the bitonic network instead (exact, slower).
// Lists of 8192 and more (longer than the largest LDS class holds): the same bitonic network in place in global memory.
//
// Direction-free bitonic network: every merge of size k starts with a mirror step (i <-> block_end - i), followed by
// the half-cleaner steps j = k/4 .. 1; every compare-exchange puts the smaller key at the lower index.  With virtual
// +inf padding above n no real element is ever exchanged with the padding, so the network also runs in place.
// Synchronisation of the threads that sort one list (gs_wave.h group_sync): the workgroup, or -- when a wave sorts a list by itself inside a larger
// workgroup -- nothing but the order of the wave's own LDS instructions (the LDS executes one wave's instructions in issue
// order; the fences keep the compiler from moving accesses across).  The fences name the LDS ("local"): a plain wavefront-scope
// release also waits for the wave's outstanding GLOBAL stores (s_waitcnt vmcnt(0)) -- the large Gaussians' scatter stood 2 us per
// round on that, the wave-per-list sort once per list.
template <int THREADS, bool WAVE, class Swap>
__device__ __forceinline__ void bitonic_network(uint32_t n, uint32_t m, int tid, Swap swap_if_greater) {
    uint32_t lk = 1;                                              // log2(k)
    for (uint32_t k = 2; k <= m; k <<= 1, ++lk) {
        const uint32_t half = k >> 1, lh = lk - 1;
        for (uint32_t t = tid; t < (m >> 1); t += THREADS) {
            const uint32_t r = t & (half - 1), i = ((t >> lh) << lk) + r, l = i + (k - 1 - 2 * r);
            if (l < n) swap_if_greater(i, l);
        }
        group_sync<WAVE>();
        uint32_t lj = lh;                                         // log2(j) + 1
        for (uint32_t j = half >> 1; j > 0; j >>= 1) {
            --lj;
            for (uint32_t t = tid; t < (m >> 1); t += THREADS) {
                const uint32_t i = ((t >> lj) << (lj + 1)) + (t & (j - 1)), l = i + j;
                if (l < n) swap_if_greater(i, l);
            }
            group_sync<WAVE>();
        }
    }
}

constexpr uint32_t DENSE_BUCKET = 48;

// LDS of one sorting group: T threads, lists shorter than T * E, 2^LOG2B depth buckets
template <int T, int E, int LOG2B>
struct SortLds {
    uint64_t sk[T * E];
    uint32_t cnt[(1 << LOG2B) + T];                               // padded: counter c lives at c + c / CPT (conflict-free scan)
    uint32_t red[4 + T / 64];
};

// Sort one list: T threads (`tid` = index inside the group).  WAVE: the group is one wave of a larger workgroup (T = 64).
// GLOBAL: lists of T * E entries and more are sorted in place in global memory (only the class of the longest lists has them).
template <int T, int E, int LOG2B, bool WAVE, bool GLOBAL>
__device__ __forceinline__ void sort_list(SortLds<T, E, LOG2B>& s, int tid, uint2 rg, uint64_t* __restrict__ vals,
                                          uint32_t* __restrict__ sorted_ids) {
    static_assert(!WAVE || T == 64, "a wave-synchronised group is one wave");
    constexpr int CAP = T * E, B = 1 << LOG2B, CPT = B / T;       // CPT counters per thread in the scan
    static_assert((CPT & (CPT - 1)) == 0 && CPT >= 2, "B / T must be a power of two");
    constexpr int LOG2CPT = __builtin_ctz(CPT);
    uint64_t* const sk = s.sk;
    uint32_t* const cnt = s.cnt;
    uint32_t* const red = s.red;
    group_sync<WAVE>();                                           // the LDS arrays are reused from list to list
    uint32_t n = rg.y - rg.x;                                     // 1 <= n; n < CAP by the class bounds, except in the GLOBAL class
    uint64_t* __restrict__ g = vals + rg.x;
    uint32_t* __restrict__ out = sorted_ids + rg.x;
    if (n >= (uint32_t)CAP) {
        if (!GLOBAL) {
            n = CAP - 1;                                          // cannot happen (class bounds); memory-safe if it ever did
        } else {                                                  // longer than the LDS holds -> in place in global memory
            uint32_t m = 2;
            while (m < n) m <<= 1;
            bitonic_network<T, false>(n, m, tid, [&](uint32_t i, uint32_t l) {
                const uint64_t a = g[i], b = g[l];
                if (a > b) { g[i] = b; g[l] = a; }
            });
            for (uint32_t i = tid; i < n; i += T) out[i] = (uint32_t)g[i] & ID_MASK;
            return;
        }
    }
#define PADC(c) ((c) + ((c) >> LOG2CPT))
    uint64_t key[E];
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t i = (uint32_t)(e * T + tid);
        key[e] = i < n ? g[i] : ~0ull;
        if (i < n) { mn = min(mn, (uint32_t)(key[e] >> 32)); mx = max(mx, (uint32_t)(key[e] >> 32)); }
    }
    for (int c = tid; c < B + T; c += T) cnt[c] = 0u;
    if (tid == 0) { red[0] = 0xFFFFFFFFu; red[1] = 0u; red[2] = 0u; }
    mn = wave_min(mn);
    mx = wave_max(mx);
    group_sync<WAVE>();
    if ((tid & 63) == 0) { atomicMin(&red[0], mn); atomicMax(&red[1], mx); }
    group_sync<WAVE>();
    mn = red[0];
    const uint32_t range = red[1] - mn;
    const int bl = range ? 32 - __clz((int)range) : 0;
    const int shift = bl > LOG2B ? bl - LOG2B : 0;              // (range >> shift) < B
#pragma unroll
    for (int e = 0; e < E; ++e)
        if ((uint32_t)(e * T + tid) < n) {
            const uint32_t b = ((uint32_t)(key[e] >> 32) - mn) >> shift;
            atomicAdd(&cnt[PADC(b)], 1u);
        }
    group_sync<WAVE>();
    // exclusive scan of the B counters: thread t owns counters [t CPT, (t + 1) CPT)
    uint32_t loc[CPT], run = 0u, big = 0u;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const uint32_t v = cnt[tid * (CPT + 1) + k];
        loc[k] = run;
        run += v;
        big = max(big, v);
    }
    const uint32_t incl = wave_inclusive_scan(run);
    big = wave_max(big);
    if ((tid & 63) == 63) red[4 + (tid >> 6)] = incl;
    if ((tid & 63) == 0) atomicMax(&red[2], big);
    group_sync<WAVE>();
    uint32_t toff = incl - run;
    for (int k = 0; k < (tid >> 6); ++k) toff += red[4 + k];
    if (red[2] > DENSE_BUCKET) {                                  // clustered depths: exact fallback (uniform branch)
#pragma unroll
        for (int e = 0; e < E; ++e)
            if ((uint32_t)(e * T + tid) < n) sk[e * T + tid] = key[e];
        uint32_t m = 2;
        while (m < n) m <<= 1;
        group_sync<WAVE>();
        bitonic_network<T, WAVE>(n, m, tid, [&](uint32_t i, uint32_t l) {
            const uint64_t a = sk[i], b = sk[l];
            if (a > b) { sk[i] = b; sk[l] = a; }
        });
        for (uint32_t i = tid; i < n; i += T) out[i] = (uint32_t)sk[i] & ID_MASK;
        return;
    }
#pragma unroll
    for (int k = 0; k < CPT; ++k) cnt[tid * (CPT + 1) + k] = toff + loc[k];
    group_sync<WAVE>();
#pragma unroll
    for (int e = 0; e < E; ++e)
        if ((uint32_t)(e * T + tid) < n) {
            const uint32_t b = ((uint32_t)(key[e] >> 32) - mn) >> shift;
            sk[atomicAdd(&cnt[PADC(b)], 1u)] = key[e];
        }
    group_sync<WAVE>();
    // cnt[b] is now the END of bucket b; rank inside the bucket by counting smaller keys
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t p = (uint32_t)(e * T + tid);
        if (p < n) {
            const uint64_t k = sk[p];
            const uint32_t b = ((uint32_t)(k >> 32) - mn) >> shift;
            const uint32_t st = b ? cnt[PADC(b - 1u)] : 0u, en = cnt[PADC(b)];
            uint32_t r = st;
            for (uint32_t q = st; q < en; ++q) r += sk[q] < k ? 1u : 0u;
            out[r] = (uint32_t)k & ID_MASK;
        }
    }
#undef PADC
}

// The two classes of long lists, one workgroup per list, grid-stride over the class's lists (the grids are sized for the chip, not
// for the worst-case number of lists):
//   class 0 (4096 entries and more)  <1024, 8, 13>: 100 KB of LDS, one workgroup per CU; lists of 8192+ sort in global memory
//   class 1 (1024 .. 4095)           <512, 8, 12>:   50 KB, three per CU.  (One class for everything from 1024 up kept a whole CU busy
//                                    with every 1100-entry list: 178 us at config 5, 350 us with the footprints of a trained scene.)
// (class 0 is only launched where lists of 4096 entries are plausible -- see gsplat_bin --; otherwise class 1's launch covers it
//  (`with_class0`), sorting the odd list that long in global memory: exact, slow, rare)
template <int T, int E, int LOG2B, int CLASS>
__global__ __launch_bounds__(T) void list_sort_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ class_bounds,
                                                      const uint2* __restrict__ ranges, uint64_t* __restrict__ vals,
                                                      uint32_t* __restrict__ sorted_ids, int with_class0) {
    __shared__ SortLds<T, E, LOG2B> s;
    const uint32_t lo = (CLASS == 0 || with_class0) ? 0u : class_bounds[CLASS - 1], hi = class_bounds[CLASS];
    for (uint32_t b = lo + blockIdx.x; b < hi; b += gridDim.x)
        sort_list<T, E, LOG2B, false, true>(s, threadIdx.x, ranges[order[b]], vals, sorted_ids);
}

// classes 1 and 2 in ONE launch (each was a latency-bound kernel of its own: 16 + 12 us at config 3, the chip half empty):
// workgroups [0, mid_blocks) sort the lists of 256..1023 entries, one per workgroup; the others sort the short lists, one per
// WAVE (four per workgroup, no workgroup barrier on that path).  Same LDS footprint either way (17.6 KB).
union SortSmallLds {
    SortLds<256, 4, 11> mid;
    SortLds<64, 4, 9> small[4];
};
__global__ __launch_bounds__(256) void list_sort_small_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ class_bounds,
                                                              uint32_t mid_blocks, const uint2* __restrict__ ranges,
                                                              uint64_t* __restrict__ vals, uint32_t* __restrict__ sorted_ids) {
    __shared__ SortSmallLds s;
    if (blockIdx.x < mid_blocks) {
        const uint32_t lo = class_bounds[1], hi = class_bounds[2];
        for (uint32_t b = blockIdx.x; lo + b < hi; b += mid_blocks)
            sort_list<256, 4, 11, false, false>(s.mid, threadIdx.x, ranges[order[lo + b]], vals, sorted_ids);
    } else {
        const uint32_t lo = class_bounds[2], hi = class_bounds[3];
        const uint32_t wave = threadIdx.x >> 6, stride = (gridDim.x - mid_blocks) * 4u;
        for (uint32_t b = (blockIdx.x - mid_blocks) * 4u + wave; lo + b < hi; b += stride)
            sort_list<64, 4, 9, true, false>(s.small[wave], (int)(threadIdx.x & 63), ranges[order[lo + b]], vals, sorted_ids);
    }
}

}  // namespace
