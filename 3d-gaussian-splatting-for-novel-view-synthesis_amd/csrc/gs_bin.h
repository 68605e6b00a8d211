// gs_bin.h -- K3: two-level counting sort of the (list, Gaussian) pairs, the large Gaussians' paths included.
#pragma once
#include "gs_layout.h"
#include "gs_wave.h"
#include "gs_sort.h"

using namespace gsm;
namespace {

// Calls f(list, ordinal, a, b) for every list of a Gaussian's rectangle whose mask bit is set (row-major; ordinal 0 .. nt - 1
// counts the calls; a, b = the owning lane's values).  Rectangles of up to 32 lists only: each lane walks its own.  Larger ones
// (large Gaussians) are walked row by row by whole waves (for_each_big_row): the caller passes nt = 0 for them.
template <class F>
__device__ __forceinline__ void for_each_list(u2 rect, uint32_t nt, uint32_t mask, int lists_x, uint64_t a, uint32_t b, F f) {
    const int x0 = rect.x & 0xFFFF, y0 = rect.x >> 16, x1 = rect.y & 0xFFFF, y1 = rect.y >> 16;
    if (nt) {                                  // (load_block_pairs leaves nt = 0 for a large Gaussian)
        uint32_t k = 0, m = mask;
        // (left to itself the compiler, knowing the rectangle has at most 32 lists here, unrolls the walk into chains of predicated
        //  LDS atomics: 2 us slower in bin_count_kernel at config 3 than the plain loops)
#pragma clang loop unroll(disable)
        for (int y = y0; y <= y1; ++y)
#pragma clang loop unroll(disable)
            for (int x = x0; x <= x1; ++x, m >>= 1)
                if (m & 1u) f((uint32_t)(y * lists_x + x), k++, a, b);
    }
}

// Lane src's large Gaussian handed to every lane of the wave (through SGPRs): its payload, the rows of its rectangle and the
// constants of its row spans (gs_math.h big_span_setup).
struct BigTaken { uint64_t payload; int y0, y1; BigSpanK bk; };
__device__ __forceinline__ BigTaken take_big_lane(u2 rect, f4 uvexy, f4 k4, uint64_t payload, int src) {
    const uint32_t rx = (uint32_t)__builtin_amdgcn_readlane((int)rect.x, src), ry = (uint32_t)__builtin_amdgcn_readlane((int)rect.y, src);
    const float kk[4] = {readlane_f(k4.x, src), readlane_f(k4.y, src), readlane_f(k4.z, src), readlane_f(k4.w, src)};
    BigTaken t;
    t.payload = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(payload >> 32), src) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)payload, src);
    const int x0 = rx & 0xFFFF, x1 = ry & 0xFFFF;
    t.y0 = rx >> 16; t.y1 = ry >> 16;
    t.bk = big_span_setup(readlane_f(uvexy.x, src), readlane_f(uvexy.y, src), readlane_f(uvexy.z, src), readlane_f(uvexy.w, src), kk, x0, x1);
    return t;
}

// The lists of the LARGE Gaussians held by the lanes of one wave (`big`: rectangle of more than 32 lists and binned at all), one
// Gaussian after the other, the lanes taking the ROWS of its rectangle: f(first list of the row's span, lists in the span, payload)
// per non-empty row (gs_math.h big_row_span: the same spans the projection kernel counted into tiles[]).  Call with all 64 lanes.
// `mine`: which lanes' Gaussians this wave takes (the four waves of a big block hold the same 64 and take every fourth each).
template <class F>
__device__ __forceinline__ void for_each_big_row(bool big, u2 rect, f4 uvexy, f4 k4, uint64_t payload, int lists_x, int lane, F f,
                                                 unsigned long long mine = ~0ull) {
    unsigned long long m = __ballot(big) & mine;
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const BigTaken t = take_big_lane(rect, uvexy, k4, payload, src);
        for (int y = t.y0 + lane; y <= t.y1; y += 64) {
            const RowSpan sp = big_row_span(t.bk, y);
            if (sp.xb >= sp.xa) f((uint32_t)(y * lists_x + sp.xa), (uint32_t)(sp.xb - sp.xa + 1), t.payload);
        }
    }
}

// ---- K3: coarse bins (F11) -----------------------------------------------------------------------------
// bin_count_kernel: a block of 2048 Gaussians histograms its (list, Gaussian) pairs over the coarse bins in LDS and takes
// its share of every bin it touches with ONE returning global atomic per bin (device-scope atomics run at ~20 G/s and
// serialise per address: one per pair was 10x slower than the radix sort this replaces; one per block and bin is noise --
// once the blocks are spread over BIN_TOTAL_SHARDS words per bin).
// Needs no pair buffer, so it is queued with the colour pass behind the counters and runs during the host round trip.
struct BlockPairs {                    // the 8 Gaussians of one thread of a binning workgroup
    static constexpr int K = BIN_GAUSS / 256;
    uint32_t nt[K], mk[K];
    u2 r[K];
    uint64_t payload[K];
};

// ALL loads of the thread's Gaussians in flight together: one round trip, and the caller can put its own set-up (prefix sums,
// clearing LDS, barriers) between this and for_block_pairs.  The rectangle, mask and depth of a Gaussian that is not binned are
// stale values: read and ignored.
__device__ __forceinline__ BlockPairs load_block_pairs(int64_t n, const u2* __restrict__ rect, const uint32_t* __restrict__ tiles,
                                                       const uint32_t* __restrict__ mask, const float* __restrict__ depth, int64_t batch) {
    constexpr int K = BlockPairs::K;
    BlockPairs bp;
    float dz[K];
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t i = batch * BIN_GAUSS + k * 256 + tid;
        const bool in = i < n;
        bp.nt[k] = in ? tiles[i] : 0u;
        bp.r[k] = in ? rect[i] : u2{0u, 0u};
        if (rect_is_big(bp.r[k])) bp.nt[k] = 0u;           // a large Gaussian: binned by the big blocks (the rectangle of a Gaussian that is
                                                           // not binned at all is stale, its nt is 0 anyway)
        bp.mk[k] = in ? mask[i] : 0u;
        dz[k] = (in && depth) ? depth[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t i = batch * BIN_GAUSS + k * 256 + tid;
        bp.payload[k] = ((uint64_t)f2u(dz[k]) << 32) | (uint64_t)(uint32_t)i;
    }
    return bp;
}

template <class F>
__device__ __forceinline__ void for_block_pairs(const BlockPairs& bp, int lists_x, F f) {
#pragma unroll
    for (int k = 0; k < BlockPairs::K; ++k) for_each_list(bp.r[k], bp.nt[k], bp.mk[k], lists_x, bp.payload[k], 0u, f);
}

// What a big block (a range of 64 Gaussians held by each of its four waves, see bin_count_kernel) holds per thread.  Returns false (uniformly) when the block's range has no
// large Gaussian: the block then leaves -- at config 3 (none at all) that is all these blocks ever do.
struct BigLane { bool big; u2 rect; f4 uvexy, k4; uint64_t payload; };      // centre + extents, row-span constants (record)
__device__ __forceinline__ bool load_big_lane(int64_t i, int64_t n, const u2* __restrict__ rect, const uint32_t* __restrict__ tiles,
                                              const Rec64* __restrict__ rec, const float* __restrict__ depth, BigLane& b,
                                              const uint32_t* __restrict__ big_flag) {
    // the projection wave of this range (one uniform load): nothing large -> nothing else is even loaded
    if (!big_flag[(i - (threadIdx.x & 63)) / 64]) return false;
    b.rect = u2{0u, 0u};
    b.big = false;
    if (i < n) {
        const uint32_t nt = tiles[i];
        b.rect = rect[i];                                  // (stale for a Gaussian that is not binned: nt = 0)
        b.big = nt != 0u && rect_is_big(b.rect);
    }
    if (!__syncthreads_or(b.big)) return false;
    b.uvexy = b.k4 = f4{0.f, 0.f, 0.f, 0.f};
    b.payload = 0ull;
    if (b.big) {
        const Rec64* r = rec + i;
        const f4 q0 = r->r0, q1 = r->r1;
        b.uvexy = f4{q0.x, q0.y, q1.z, q1.w};
        b.k4 = r->pad;
        b.payload = ((uint64_t)f2u(depth ? depth[i] : 0.f) << 32) | (uint64_t)(uint32_t)i;
    }
    return true;
}

// body(range) for every range of this big block (first, first + stride, ...) whose projection wave flagged a large Gaussian.  The
// flags are read in rounds of 256 candidate ranges, one per thread (one round trip per round), and the flagged ones listed in LDS:
// a block with nothing to do -- every one of them at config 3 -- leaves after one round trip, and a scene with FEW large Gaussians
// (config 5: 156 K ranges, 200 per block) does not probe its ranges one dependent load after the other.  body may synchronise the
// workgroup (it is called uniformly).
struct FlaggedLds { uint32_t list[256]; uint32_t count; };
template <class Body>
__device__ __forceinline__ void for_flagged_ranges(const uint32_t* __restrict__ big_flag, int64_t first, int64_t stride, int64_t ranges,
                                                   FlaggedLds& fl, Body body) {
    for (int64_t base = first; base < ranges; base += 256 * stride) {
        if (threadIdx.x == 0) fl.count = 0u;
        __syncthreads();
        const int64_t r = base + (int64_t)threadIdx.x * stride;
        if (r < ranges && big_flag[r] != 0u) fl.list[atomicAdd(&fl.count, 1u)] = (uint32_t)r;
        __syncthreads();
        const uint32_t cnt = fl.count;
        for (uint32_t i = 0; i < cnt; ++i) body((int64_t)fl.list[i]);
        __syncthreads();
    }
}

// pieces of a run of consecutive lists [l0, l0 + cnt) by coarse bin: g(bin, first list of the piece, lists in the piece)
template <class G>
__device__ __forceinline__ void for_bin_pieces(uint32_t l0, uint32_t cnt, G g) {
    const uint32_t l1 = l0 + cnt - 1u;
    for (uint32_t b = l0 >> BIN_SHIFT; b <= (l1 >> BIN_SHIFT); ++b) {
        const uint32_t a = max(l0, b << BIN_SHIFT), e = min(l1, (b << BIN_SHIFT) + (1u << BIN_SHIFT) - 1u);
        g(b, a, e - a + 1u);
    }
}

__device__ __forceinline__ void bin_count_big(int64_t n, const u2* __restrict__ rect, const uint32_t* __restrict__ tiles, int lists_x, int nb,
                                                        uint32_t* __restrict__ bin_total, const Rec64* __restrict__ rec,
                                                        const uint32_t* __restrict__ big_flag, uint32_t small_blocks, uint32_t* hist) {
    const int tid = threadIdx.x;
    const int64_t ranges = (n + 63) / 64;
    const unsigned long long mine = 0x1111111111111111ull << (tid >> 6);          // this wave's quarter of the range's Gaussians
    // the block's ranges are counted into ONE histogram, flushed once (a flush per range of 64: 123 K atomics on the 79 totals of
    // config 6, +14 us)
    __shared__ FlaggedLds fl;
    bool any = false;
    for (int b = tid; b < nb; b += 256) hist[b] = 0u;
    for_flagged_ranges(big_flag, blockIdx.x - small_blocks, gridDim.x - small_blocks, ranges, fl, [&](int64_t range) {
        BigLane bl;
        if (!load_big_lane(range * 64 + (tid & 63), n, rect, tiles, rec, nullptr, bl, big_flag)) return;
        any = true;
        for_each_big_row(bl.big, bl.rect, bl.uvexy, bl.k4, 0ull, lists_x, tid & 63, [&](uint32_t l0, uint32_t cnt, uint64_t) {
            for_bin_pieces(l0, cnt, [&](uint32_t b, uint32_t, uint32_t c) { atomicAdd(&hist[b], c); });
        }, mine);
    });
    if (!any) return;                                      // (uniform; for_flagged_ranges ends with a barrier)
    for (int b = tid; b < nb; b += 256) {
        const uint32_t c = hist[b];
        if (c) atomicAdd(&bin_total[BIN_TOTAL_SHARDS * nb + b], c);      // (no offset is drawn here: bin_scatter_kernel's big blocks draw theirs)
    }
}

// Grid = the blocks of 2048 Gaussians, which bin the SMALL Gaussians (rectangles of up to 32 lists, each lane walking its own), then
// `big_blocks` blocks, which bin the LARGE ones of ranges of 64 Gaussians wave-cooperatively (for_each_big_row; every wave of the block
// holds the range's 64 Gaussians and takes every fourth): a Gaussian of a trained scene covers hundreds of lists, and 2048 of them per
// block left the chip with 49 workgroups walking half a million lists each.  (Ranges of 256 with 64 Gaussians per wave, one after the
// other, the first version: 1.5 waves per SIMD in a chain of dependent LDS atomics and shuffles -- 161 us for the scatter at config 6.)
__global__ __launch_bounds__(256) void bin_count_kernel(int64_t n, const u2* __restrict__ rect, const uint32_t* __restrict__ tiles,
                                                        const uint32_t* __restrict__ mask, int lists_x, int nb, uint32_t* __restrict__ bin_total,
                                                        uint32_t* __restrict__ block_off, uint32_t* __restrict__ list_count,
                                                        uint2* __restrict__ ranges, int nl, CounterBlock* cb, DevCounts* counts,
                                                        DevCounts* counts_mapped, const Rec64* __restrict__ rec, const uint32_t* __restrict__ big_flag, uint32_t small_blocks,
                                                        int batches) {
    // hist[nb]: dynamic LDS, sized by the launch (a static array for the largest image, 32 KB, held the two binning kernels at 3-4
    // workgroups per CU whatever the image: the blocks of the large Gaussians ran in three rounds)
    extern __shared__ uint32_t bin_lds[];
    uint32_t* const hist = bin_lds;
    const int tid = threadIdx.x;
    if (blockIdx.x >= small_blocks) {            // ---- ranges of 64 Gaussians (grid-stride): the large ones of each range
        bin_count_big(n, rect, tiles, lists_x, nb, bin_total, rec, big_flag, small_blocks, hist);
        return;
    }
    BlockPairs bp = load_block_pairs(n, rect, tiles, mask, nullptr, (int64_t)blockIdx.x * batches);
    if (cb && blockIdx.x == 0) {                 // GSPLAT_PROJECT_COUNTS_LATE: totals of the projection's sharded counters; shards cleared
        static_assert(COUNT_SHARDS == 256, "one shard per thread");
        __shared__ unsigned long long tsum[4][4];
        __shared__ uint32_t tmax[4];
        CountShard* sh = cb->shards + tid;
        unsigned long long t4[4];
        t4[0] = (unsigned long long)(uint32_t)__hip_atomic_load(&sh->survivors, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t4[1] = (unsigned long long)(uint32_t)__hip_atomic_load(&sh->visible, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t4[2] = (unsigned long long)__hip_atomic_load(&sh->ref_pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t4[3] = (unsigned long long)__hip_atomic_load(&sh->bin_pairs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t mxt = (uint32_t)__hip_atomic_load(&sh->max_tiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->survivors, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->visible, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->ref_pairs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->bin_pairs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&sh->max_tiles, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (int sft = 32; sft > 0; sft >>= 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) t4[k] += (unsigned long long)__shfl_xor((long long)t4[k], sft);
            mxt = max(mxt, (uint32_t)__shfl_xor((int)mxt, sft));
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tsum[tid >> 6][k] = t4[k];
            tmax[tid >> 6] = mxt;
        }
        __syncthreads();
        if (tid == 0) {
            DevCounts c;
            c.n_survivors = (int32_t)(tsum[0][0] + tsum[1][0] + tsum[2][0] + tsum[3][0]);
            c.n_visible = (int32_t)(tsum[0][1] + tsum[1][1] + tsum[2][1] + tsum[3][1]);
            c.n_pairs = (int64_t)(tsum[0][2] + tsum[1][2] + tsum[2][2] + tsum[3][2]);
            c.max_tiles = (int32_t)max(max(tmax[0], tmax[1]), max(tmax[2], tmax[3]));
            c.reserved = 0;
            c.n_binned = (int64_t)(tsum[0][3] + tsum[1][3] + tsum[2][3] + tsum[3][3]);
            *counts = c;
            if (counts_mapped) *counts_mapped = c;
        }
    }
    for (int l = blockIdx.x * 256 + tid; l < (nb << BIN_SHIFT); l += (int)small_blocks * 256) {     // for the split kernels
        list_count[l] = 0u;
        if (l < nl) ranges[l] = uint2{0u, 0u};
    }
    for (int b = tid; b < nb; b += 256) hist[b] = 0u;
    __syncthreads();
    for (int bt = 0;;) {
        for_block_pairs(bp, lists_x, [&](uint32_t l, uint32_t, uint64_t, uint32_t) { atomicAdd(&hist[l >> BIN_SHIFT], 1u); });
        if (++bt >= batches) break;
        bp = load_block_pairs(n, rect, tiles, mask, nullptr, (int64_t)blockIdx.x * batches + bt);
    }
    __syncthreads();
    for (int b = tid; b < nb; b += 256) {
        const uint32_t c = hist[b];
        // (the offset inside the block's SHARD of the bin: one word per bin took all 489 blocks of config 3 at about the same time)
        if (c) block_off[(int64_t)blockIdx.x * nb + b] = atomicAdd(&bin_total[(blockIdx.x % BIN_TOTAL_SHARDS) * nb + b], c);
    }
}

// bin_scatter_kernel: the same enumeration; a pair goes to bin_start[bin] + the block's offset in the bin + its arrival
// rank inside the block (LDS atomic).  The order inside a bin is arbitrary; the per-list sort by the unique payload makes
// the final order deterministic.
// The scatter of a wave's large Gaussians, one after the other: the lanes take the rows of the rectangle, every row's span is cut at the
// coarse-bin boundaries (a span of up to 33 lists crosses at most one: two rounds), each piece draws a run of slots from its bin's
// cursor in LDS -- and then the PAIRS, not the rows, are dealt to the lanes (`owner`: which lane's piece pair k belongs to), so that a
// store instruction writes up to 64 consecutive payloads instead of one 8-byte word into each of ~20 different runs.
// (every lane writing its own row's run instead: tried and dropped)
constexpr int BIG_ROUND_PAIRS = 64 * 34;             // 64 rows x the widest span a rectangle can have (radius <= 250 px: 33 lists)
__device__ __forceinline__ void scatter_big_rows(const BigLane& bl, int lists_x, int lane, uint32_t* cur, uint8_t* owner, uint32_t n_binned,
                                                 uint64_t* __restrict__ bvals, unsigned long long mine) {
    unsigned long long m = __ballot(bl.big) & mine;
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const BigTaken t = take_big_lane(bl.rect, bl.uvexy, bl.k4, bl.payload, src);
        const int y0 = t.y0, y1 = t.y1;
        const uint64_t pl = t.payload;
        for (int yb = y0; yb <= y1; yb += 64) {                         // 64 rows per pass (one pass up to 512-pixel-high rectangles)
            const int y = yb + lane;
            RowSpan sp = RowSpan{1, 0};
            if (y <= y1) sp = big_row_span(t.bk, y);
            const bool has = sp.xb >= sp.xa;
            const uint32_t l0 = has ? (uint32_t)(y * lists_x + sp.xa) : 0u, l1 = has ? (uint32_t)(y * lists_x + sp.xb) : 0u;
            const uint32_t cut = ((l0 >> BIN_SHIFT) + 1u) << BIN_SHIFT;  // first list of the next bin
            for (int round = 0; round < 2; ++round) {
                // piece of this round: [a, a + c)
                const uint32_t a = round == 0 ? l0 : cut;
                const uint32_t c = !has ? 0u : (round == 0 ? min(l1 + 1u, cut) - l0 : (l1 >= cut ? l1 + 1u - cut : 0u));
                if (!__any(c != 0u)) continue;
                const uint32_t pos = c ? atomicAdd(&cur[a >> BIN_SHIFT], c) : 0u;
                const uint32_t incl = wave_inclusive_scan(c);
                const uint32_t pre = incl - c, total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                for (uint32_t j = 0; j < c; ++j) owner[pre + j] = (uint8_t)lane;
                group_sync<true>();
                for (uint32_t k0 = 0; k0 < total; k0 += 64) {                   // (uniform trip count: a shuffle reads nothing from a lane that
                    const uint32_t k = k0 + (uint32_t)lane;                     //  has left the loop)
                    const int o = k < total ? owner[k] : 0;
                    const uint32_t j = k - (uint32_t)__shfl((int)pre, o);
                    const uint32_t dst = (uint32_t)__shfl((int)pos, o) + j, l = (uint32_t)__shfl((int)a, o) + j;
                    if (k < total && dst < n_binned) bvals[dst] = pl | ((uint64_t)(l & ((1u << BIN_SHIFT) - 1u)) << ID_BITS);
                }
                group_sync<true>();                                             // `owner` is rewritten by the next round
            }
        }
    }
}

// A bin's region of the bin-ordered array: [ small Gaussians, shard 0 | shard 1 | ... | pairs of the large ones ]; the small blocks
// place theirs with the offsets bin_count_kernel drew inside their shard (block_off), the big blocks (same split of the grid as there)
// count their range again, draw ONE offset per touched bin from the bin's cursor (the last row of bin_total) and scatter.
//
// Exclusive prefix of the bin totals (small + large) for both kinds of block: thread t owns a contiguous run of ceil(nb / 256) bins and
// calls own(b, start of bin b, total of bin b, k) for each of them (k = index inside the run; the first BIN_PRE totals are in bt[]).
// The totals of a thread's first bin are loaded up front (BIN_PRE; all there are up to 256 bins), every shard of them: one round trip.
// `shard`: the caller's own (a small block); its pairs lie behind those of the shards before it.
// How many of a thread's bins have their totals loaded up front, all shards of each in flight together.  ONE: with four (every bin of a
// thread up to 1024 bins) the scatter kernel held 4 x 9 totals and their addresses, 161 VGPRs instead of 79 -- 3 waves per SIMD, and
// the large Gaussians' blocks, which live on occupancy, paid for it (config 6: bin stage 244 -> 270 us).  With one it needs 96 (5 waves);
// an image of more than 256 bins pays one round trip per further bin of the thread.
constexpr int BIN_PRE = 1;
struct BinTotals { uint32_t before, small, all; };     // of one bin: the shards before `shard` | all shards | shards + the large Gaussians' pairs
__device__ __forceinline__ BinTotals bin_totals_of(const uint32_t* __restrict__ bin_total, int nb, int b, int shard) {
    uint32_t t[BIN_TOTAL_SHARDS + 1];
#pragma unroll
    for (int s = 0; s <= BIN_TOTAL_SHARDS; ++s) t[s] = bin_total[s * nb + b];          // (all in flight together)
    BinTotals r{0u, 0u, 0u};
#pragma unroll
    for (int s = 0; s < BIN_TOTAL_SHARDS; ++s) {
        r.before += s < shard ? t[s] : 0u;
        r.small += t[s];
    }
    r.all = r.small + t[BIN_TOTAL_SHARDS];
    return r;
}
struct BinPrefix { int per, first; uint32_t bt[BIN_PRE], small[BIN_PRE], before[BIN_PRE], run; };      // bt = small + large pairs of the bin, small = the small
                                                                                     // Gaussians' part, before = its shards before the caller's
__device__ __forceinline__ BinPrefix bin_prefix_load(const uint32_t* __restrict__ bin_total, int nb, int shard) {
    BinPrefix p;
    p.per = (nb + 255) / 256;
    p.first = (int)threadIdx.x * p.per;
    uint32_t t[BIN_PRE][BIN_TOTAL_SHARDS + 1];
#pragma unroll
    for (int k = 0; k < BIN_PRE; ++k) {
        const bool in = k < p.per && p.first + k < nb;
#pragma unroll
        for (int s = 0; s <= BIN_TOTAL_SHARDS; ++s) t[k][s] = in ? bin_total[s * nb + p.first + k] : 0u;
    }
#pragma unroll
    for (int k = 0; k < BIN_PRE; ++k) {
        p.before[k] = p.small[k] = 0u;
#pragma unroll
        for (int s = 0; s < BIN_TOTAL_SHARDS; ++s) {
            p.before[k] += s < shard ? t[k][s] : 0u;
            p.small[k] += t[k][s];
        }
        p.bt[k] = p.small[k] + t[k][BIN_TOTAL_SHARDS];
    }
    p.run = 0u;
#pragma unroll
    for (int k = 0; k < BIN_PRE; ++k) p.run += p.bt[k];
    for (int k = BIN_PRE; k < p.per; ++k) p.run += p.first + k < nb ? bin_totals_of(bin_total, nb, p.first + k, 0).all : 0u;
    return p;
}
// start of the thread's first bin (one workgroup barrier inside)
__device__ __forceinline__ uint32_t bin_prefix_scan(const BinPrefix& p, uint32_t* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_scan(p.run);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t st = incl - p.run;
    for (int k = 0; k < wave; ++k) st += wsum[k];
    return st;
}

__device__ __forceinline__ void bin_scatter_big(int64_t n, const u2* __restrict__ rect, const uint32_t* __restrict__ tiles,
                                                          const float* __restrict__ depth, int lists_x, int nb, uint32_t* __restrict__ bin_total,
                                                          uint32_t n_binned, uint64_t* __restrict__ bvals, const Rec64* __restrict__ rec,
                                                          const uint32_t* __restrict__ big_flag, uint32_t small_blocks, uint32_t* cur, uint32_t* wsum,
                                                          uint8_t* owner) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t ranges = (n + 63) / 64;
    const unsigned long long mine = 0x1111111111111111ull << (tid >> 6);          // this wave's quarter of the range's Gaussians
    __shared__ FlaggedLds fl;
    for_flagged_ranges(big_flag, blockIdx.x - small_blocks, gridDim.x - small_blocks, ranges, fl, [&](int64_t range) {
        BigLane bl;
        if (!load_big_lane(range * 64 + lane, n, rect, tiles, rec, depth, bl, big_flag)) return;
        const BinPrefix bpf = bin_prefix_load(bin_total, nb, 0);
        for (int b = tid; b < nb; b += 256) cur[b] = 0u;
        __syncthreads();
        for_each_big_row(bl.big, bl.rect, bl.uvexy, bl.k4, 0ull, lists_x, lane, [&](uint32_t l0, uint32_t cnt, uint64_t) {
            for_bin_pieces(l0, cnt, [&](uint32_t b, uint32_t, uint32_t c) { atomicAdd(&cur[b], c); });      // this range's pairs per bin
        }, mine);
        uint32_t st = bin_prefix_scan(bpf, wsum);              // (its barrier also closes the counting)
        // start of the bin + its small part + what this block draws from the large part's cursor (ONE returning atomic per touched
        // bin and block; the atomics of a thread's first BIN_PRE bins are in flight together: a range pays one round trip for them,
        // not one per bin)
        uint32_t mine4[BIN_PRE], got4[BIN_PRE];
#pragma unroll
        for (int k = 0; k < BIN_PRE; ++k) mine4[k] = (k < bpf.per && bpf.first + k < nb) ? cur[bpf.first + k] : 0u;
#pragma unroll
        for (int k = 0; k < BIN_PRE; ++k) got4[k] = mine4[k] ? atomicAdd(&bin_total[(BIN_TOTAL_SHARDS + 1) * nb + bpf.first + k], mine4[k]) : 0u;
#pragma unroll
        for (int k = 0; k < BIN_PRE; ++k) {
            if (k < bpf.per && bpf.first + k < nb) {
                if (mine4[k]) cur[bpf.first + k] = st + bpf.small[k] + got4[k];
                st += bpf.bt[k];
            }
        }
        for (int k = BIN_PRE; k < bpf.per; ++k) {                    // (more than 1024 bins: images beyond 4 M pixels)
            const int b = bpf.first + k;
            if (b < nb) {
                const uint32_t mine = cur[b];
                const BinTotals t = bin_totals_of(bin_total, nb, b, 0);
                if (mine) cur[b] = st + t.small + atomicAdd(&bin_total[(BIN_TOTAL_SHARDS + 1) * nb + b], mine);
                st += t.all;
            }
        }
        __syncthreads();
        scatter_big_rows(bl, lists_x, lane, cur, owner, n_binned, bvals, mine);
        __syncthreads();                                        // cur is cleared again by the next range
    });
}

__global__ __launch_bounds__(256) void bin_scatter_kernel(int64_t n, const u2* __restrict__ rect, const uint32_t* __restrict__ tiles,
                                                          const uint32_t* __restrict__ mask, const float* __restrict__ depth, int lists_x, int nb,
                                                          uint32_t* __restrict__ bin_total, const uint32_t* __restrict__ block_off,
                                                          uint32_t* __restrict__ bin_start, uint32_t n_binned,
                                                          uint64_t* __restrict__ bvals, const Rec64* __restrict__ rec,
                                                          const uint32_t* __restrict__ big_flag, uint32_t small_blocks, int batches) {
    extern __shared__ uint32_t bin_lds[];                  // cur[nb] (see bin_count_kernel)
    uint32_t* const cur = bin_lds;
    __shared__ uint32_t wsum[4];
    __shared__ uint8_t owner[4][BIG_ROUND_PAIRS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x >= small_blocks) {            // ---- ranges of 64 Gaussians (grid-stride): the large ones of each range
        bin_scatter_big(n, rect, tiles, depth, lists_x, nb, bin_total, n_binned, bvals, rec, big_flag, small_blocks, cur, wsum, owner[wave]);
        return;
    }
    BlockPairs bp = load_block_pairs(n, rect, tiles, mask, depth, (int64_t)blockIdx.x * batches);
    const int shard = (int)(blockIdx.x % BIN_TOTAL_SHARDS);          // (the shard bin_count_kernel drew this block's offsets from)
    const BinPrefix bpf = bin_prefix_load(bin_total, nb, shard);
    uint32_t bo[BIN_PRE];
#pragma unroll
    for (int k = 0; k < BIN_PRE; ++k) bo[k] = (k < bpf.per && bpf.first + k < nb) ? block_off[(int64_t)blockIdx.x * nb + bpf.first + k] : 0u;
    uint32_t st = bin_prefix_scan(bpf, wsum);
    for (int k = 0; k < bpf.per; ++k) {
        const int b = bpf.first + k;
        if (b < nb) {
            BinTotals t{bpf.before[k % BIN_PRE], 0u, bpf.bt[k % BIN_PRE]};
            if (k >= BIN_PRE) t = bin_totals_of(bin_total, nb, b, shard);
            const uint32_t c = t.all;
            cur[b] = st + t.before + (k < BIN_PRE ? bo[k % BIN_PRE] : block_off[(int64_t)blockIdx.x * nb + b]);   // garbage for bins this block never touches: unused
            if (blockIdx.x == 0) {
                bin_start[b] = st;
                if (b == nb - 1) bin_start[nb] = st + c;
            }
            st += c;
        }
    }
    __syncthreads();
    for (int bt = 0;;) {
        for_block_pairs(bp, lists_x, [&](uint32_t l, uint32_t, uint64_t pl, uint32_t) {
            const uint32_t pos = atomicAdd(&cur[l >> BIN_SHIFT], 1u);
            if (pos < n_binned)                             // defensive: never write past the caller's buffer
                bvals[pos] = pl | ((uint64_t)(l & ((1u << BIN_SHIFT) - 1u)) << ID_BITS);
        });
        if (++bt >= batches) break;
        bp = load_block_pairs(n, rect, tiles, mask, depth, (int64_t)blockIdx.x * batches + bt);
    }
}

// split_count_kernel / split_scatter_kernel: every bin is split into its 64 lists.  Work is cut into chunks of 4096 pairs
// of the bin-ordered array (a dense bin of 60 K pairs is shared by 15 workgroups; one workgroup per bin was tail-bound);
// a chunk that crosses bin boundaries handles one segment per bin.  Count: LDS histogram of the segment over the bin's 64
// lists, one returning global atomic per list -> the segment's offset inside each list.  Scatter: list start = bin
// start + prefix of the bin's final list counts; a pair goes to list start + segment offset + arrival rank (LDS atomic).
// The segment that begins a bin also writes the [start, end) of the bin's lists.  Segment id = chunk + bin (unique: from
// one segment to the next at least one of the two grows).
//
// Which bin holds pair p (the b with bin_start[b] <= p < bin_start[b + 1]): every thread looks at its bins, the one that finds it
// reports it -- ONE round trip (a binary search is 8 dependent loads at config 3: 4-5 us at the start of every workgroup).
// Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ int bin_of_pair_parallel(const uint32_t* __restrict__ bin_start, int nb, uint32_t p, int* slot) {
    if (threadIdx.x == 0) *slot = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < nb; t += THREADS)
        if (bin_start[t] <= p && p < bin_start[t + 1]) *slot = t;
    __syncthreads();
    return *slot;
}

__device__ __forceinline__ uint32_t local_list(uint64_t v) { return (uint32_t)(v >> ID_BITS) & ((1u << BIN_SHIFT) - 1u); }

// The grids of the two kernels come from the CAPACITY of the pair buffers (the host need not know the count); the pairs
// really binned are counts->n_binned.  More pairs than the buffers hold: only the first `capacity` are processed and the
// ranges are clipped to the buffers -- memory-safe garbage; the caller sees n_binned > capacity in the counters and renders
// the frame again with larger buffers.
__device__ __forceinline__ uint32_t pairs_to_process(const DevCounts* counts, uint32_t capacity) {
    const long long nb_ = counts->n_binned;
    return nb_ < (long long)capacity ? (uint32_t)nb_ : capacity;
}

__global__ __launch_bounds__(256) void split_count_kernel(int nb, const uint32_t* __restrict__ bin_start, const uint64_t* __restrict__ bvals,
                                                          uint32_t capacity, const DevCounts* __restrict__ counts,
                                                          uint32_t* __restrict__ list_count, uint32_t* __restrict__ seg_off) {
    constexpr int L = 1 << BIN_SHIFT, U = SPLIT_CHUNK / 256;
    __shared__ uint32_t cnt[L];
    __shared__ int s_b0;
    const int tid = threadIdx.x;
    const uint32_t n_binned = pairs_to_process(counts, capacity);
    const uint32_t c0 = blockIdx.x * (uint32_t)SPLIT_CHUNK, c1 = min(c0 + (uint32_t)SPLIT_CHUNK, n_binned);
    if (c0 >= n_binned) return;
    for (int b = bin_of_pair_parallel<256>(bin_start, nb, c0, &s_b0); b < nb && bin_start[b] < c1; ++b) {
        const uint32_t s = max(c0, bin_start[b]), e = min(c1, bin_start[b + 1]);
        if (s >= e) continue;                                  // empty bin (uniform)
        uint32_t k[U];                                          // (loads issued before the barrier: one round trip less)
#pragma unroll
        for (int u = 0; u < U; ++u) k[u] = s + u * 256 + tid < e ? local_list(bvals[s + u * 256 + tid]) : 0xFFFFFFFFu;
        if (tid < L) cnt[tid] = 0u;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k[u] != 0xFFFFFFFFu) atomicAdd(&cnt[k[u]], 1u);
        __syncthreads();
        if (tid < L) {
            const uint32_t c = cnt[tid];
            if (c) seg_off[((int64_t)blockIdx.x + b) * L + tid] = atomicAdd(&list_count[b * L + tid], c);
        }
        __syncthreads();
    }
}

// ---- K3c, second half (it carries the plan: gs_sort.h plan_body) ----------------------------------------------------
// Block 0 does not scatter: it is the PLAN (the list lengths are final after split_count_kernel, and a one-workgroup kernel of
// its own was 13 us of latency at config 3; here it runs beside the scatter).
constexpr int SPLIT_THREADS = 1024;
__global__ __launch_bounds__(SPLIT_THREADS) void split_scatter_kernel(int nl, int nb, const uint32_t* __restrict__ bin_start,
                                                            const uint64_t* __restrict__ bvals, uint32_t capacity,
                                                            const DevCounts* __restrict__ counts,
                                                            const uint32_t* __restrict__ list_count, const uint32_t* __restrict__ seg_off,
                                                            uint2* __restrict__ ranges, uint64_t* __restrict__ vals,
                                                            uint32_t* __restrict__ order, uint32_t* __restrict__ class_bounds) {
    constexpr int L = 1 << BIN_SHIFT, U = SPLIT_CHUNK / SPLIT_THREADS;
    __shared__ uint32_t lds[PLAN_LDS_WORDS];
    if (blockIdx.x == 0) {
        plan_body<SPLIT_THREADS>(nl, [&](int l) { return list_count[l]; }, order, class_bounds, lds, lds + 256 * 16);
        return;
    }
    uint32_t* const cur = lds;                               // [L]
    const int tid = threadIdx.x;
    const uint32_t n_binned = pairs_to_process(counts, capacity);
    const uint32_t chunk = blockIdx.x - 1u;
    const uint32_t c0 = chunk * (uint32_t)SPLIT_CHUNK, c1 = min(c0 + (uint32_t)SPLIT_CHUNK, n_binned);
    if (c0 >= n_binned) return;
    int* const s_b0 = reinterpret_cast<int*>(lds + L);
    for (int b = bin_of_pair_parallel<SPLIT_THREADS>(bin_start, nb, c0, s_b0); b < nb && bin_start[b] < c1; ++b) {
        const uint32_t bs = bin_start[b], s = max(c0, bs), e = min(c1, bin_start[b + 1]);
        if (s >= e) continue;
        uint64_t v[U];                                          // (loads issued before the scan and the barrier: one round trip less)
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = s + u * SPLIT_THREADS + tid < e ? bvals[s + u * SPLIT_THREADS + tid] : ~0ull;
        if (tid < L) {                                          // one wave: exclusive scan of the bin's 64 list sizes
            const uint32_t c = list_count[b * L + tid];
            const uint32_t incl = wave_inclusive_scan(c);
            const uint32_t st = bs + incl - c;
            cur[tid] = st + seg_off[((int64_t)chunk + b) * L + tid];           // garbage where the segment has no pair: unused
            const int list = b * L + tid;
            if (s == bs && list < nl) ranges[list] = uint2{min(st, capacity), min(st + c, capacity)};    // (clipped: overflow only)
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (s + u * SPLIT_THREADS + tid < e) {
                const uint32_t pos = atomicAdd(&cur[local_list(v[u])], 1u);
                if (pos < n_binned) vals[pos] = v[u];
            }
        __syncthreads();
    }
}

}  // namespace
