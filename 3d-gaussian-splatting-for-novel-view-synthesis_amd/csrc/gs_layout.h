// gs_layout.h -- layout of the caller-owned buffers, constants and grid sizes (host-side arithmetic only).
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>
#include "gs_body.h"

using namespace gsm;
namespace {

constexpr int64_t ALIGN = 256;
inline int64_t up(int64_t x) { return (x + ALIGN - 1) / ALIGN * ALIGN; }
// Hands out consecutive 256-byte-aligned parts of one buffer (base may be NULL: the pointers are then the offsets).
struct Carver {
    char* base;
    int64_t o = 0;
    template <class T> T* take(int64_t bytes) { T* r = (T*)(base + o); o += up(bytes); return r; }
};

// ---- layout of the caller-owned buffers (private to the library) ---------------------------------
struct DevCounts {           // device-side counters; copied into gsplat_counts
    int32_t n_survivors, n_visible;
    int64_t n_pairs;         // the reference's (tile, Gaussian) pairs (F11)
    int32_t max_tiles, reserved;
    int64_t n_binned;        // (list, Gaussian) pairs actually binned
};
static_assert(sizeof(DevCounts) == sizeof(gsplat_counts), "counts layout");

constexpr int COUNT_SHARDS = 256;     // per-wave counters are spread over 256 cache lines (same-address atomics serialise)
struct alignas(64) CountShard { int32_t survivors, visible, max_tiles; uint32_t ref_pairs, bin_pairs, arrived; int32_t pad[10]; };
// The caller's `scratch` of gsplat_project: counters that must be ZERO when a call starts.  The caller zeroes the block once;
// the wave of the projection kernel that finishes last adds the shards up and clears them again (no clearing kernel, no
// totals kernel: the front of the pipeline is latency-bound and every dependent launch costs ~5 us).
struct CounterBlock {
    CountShard shards[COUNT_SHARDS];
    uint32_t done;            // shards whose waves have all added their counts (arrivals are counted per shard first: ONE word takes
                              // only ~88 returning atomics per microsecond, 15 625 waves on it cost 0.18 ms)
    uint32_t pad[15];
};

// A "list" is the depth-ordered set of Gaussians of one 16 x 8-pixel region: the unit one wave64 rasterises.
// Binning is a two-level counting sort: (list, Gaussian) pairs go to coarse bins of 64 consecutive lists first
// (bin_count_kernel / bin_scatter_kernel, blocks of 2048 Gaussians with an LDS histogram, one global atomic per block and
// bin), then every bin is split into its 64 lists (split_count_kernel / split_scatter_kernel), then every list is sorted by depth.
constexpr int BIN_SHIFT = 6;                 // 64 lists per coarse bin
constexpr int BIN_TOTAL_SHARDS = 8;        // block blk of bin_count_kernel draws its offsets from shard blk % 8 of the bin totals: 489 blocks
                                             // on ONE word per bin arrive together and a word takes ~88 returning atomics per microsecond
constexpr int BIN_TOTAL_ROWS = BIN_TOTAL_SHARDS + 2;      // rows of bin_total[]: the shards | the large Gaussians' totals | their cursor
constexpr int BIN_GAUSS = 2048;              // Gaussians per block of bin_count_kernel / bin_scatter_kernel
constexpr int MAX_BINS = 8192;               // LDS histogram of the two kernels (32 KB): images up to 8192 x 8192 / 128 lists
constexpr int SPLIT_CHUNK = 4096;            // pairs per block of split_count_kernel / split_scatter_kernel
// Pair payload (64 bit): float_bits(z) << 32 | list index inside its bin << ID_BITS | Gaussian index.  z > 0, so the
// bit pattern orders like the value; inside one list the middle field is constant: sorting payloads = (depth, index) order.
constexpr int ID_BITS = 32 - BIN_SHIFT;      // 26: up to 67 M Gaussians per call
constexpr uint32_t ID_MASK = (1u << ID_BITS) - 1u;

struct ProjectState {
    Camera* cam;
    DevCounts* counts;
    Rec64* rec;
    u2* rect;                // per Gaussian: inclusive rectangle of lists
    float* depth;
    uint32_t* tiles;         // per Gaussian: number of lists (0 = contributes nowhere)
    uint32_t* mask;          // per Gaussian: which lists of the rectangle (ellipse / list test; all ones above 32 lists)
    uint32_t* bin_total;     // [BIN_TOTAL_ROWS x bins] pairs per coarse bin of the small Gaussians, one row per shard | of the large ones
                             //            (rectangles of more than 32 lists: row BIN_TOTAL_SHARDS) | the large ones' scatter cursor (the row
                             //            behind it); zero per frame
    uint32_t* bin_start;     // [bins + 1] exclusive prefix of bin_total
    uint32_t* block_off;     // [blocks x bins] where a block's pairs start inside a bin
    uint32_t* list_count;    // [bins x 64] pairs per list (split_count_kernel)
    uint2* ranges;           // [lists] start, end in the pair arrays
    uint32_t* order;         // [lists] launch order: longest list first
    uint32_t* class_bounds;  // [8] boundaries of the sort size classes inside `order`
    float* kj;               // [n][12] fused inputs, GSPLAT_PROJECT_SAVE_SH_JACOBIAN: d rgb / d logit (3), d logit / d position (9)
    uint32_t* big_flag;      // [ceil(n / 64)] does this wave of the projection kernel hold a large Gaussian (rectangle of more than 32
                             // lists)?  written by EVERY wave in every frame: the binning kernels' big blocks look here before anything else
    int64_t bytes;
};

inline int64_t n_lists(const gsplat_view* v) { return (int64_t)((v->W + LIST_W - 1) / LIST_W) * ((v->H + LIST_H - 1) / LIST_H); }
inline int64_t n_bins(int64_t nl) { return (nl + (1 << BIN_SHIFT) - 1) >> BIN_SHIFT; }
// A block of the two binning kernels takes `bin_batches(n)` batches of 2048 Gaussians, one after the other, into the same LDS
// histogram / cursors: for a very large scene this keeps the number of blocks near a thousand -- each block pays one returning global
// atomic per bin (config 5: 4883 blocks x 1012 bins = 4.9 M of them) and keeps one half-written line per bin open in the scatter.
inline int bin_batches(int64_t n) { const int64_t b = n / ((int64_t)BIN_GAUSS * 1024); return (int)(b < 1 ? 1 : (b > 4 ? 4 : b)); }
inline int64_t n_bin_blocks(int64_t n) { const int64_t per = (int64_t)BIN_GAUSS * bin_batches(n); return (n + per - 1) / per; }

ProjectState carve_project(void* base, int64_t n, int64_t nl) {
    ProjectState s;
    Carver c{(char*)base};
    const int64_t nb = n_bins(nl);
    s.cam = c.take<Camera>(sizeof(Camera));
    s.counts = c.take<DevCounts>(sizeof(DevCounts));
    s.rec = c.take<Rec64>(n * 64);
    s.rect = c.take<u2>(n * 8);
    s.depth = c.take<float>(n * 4);
    s.tiles = c.take<uint32_t>(n * 4);
    s.mask = c.take<uint32_t>(n * 4);
    s.bin_total = c.take<uint32_t>(BIN_TOTAL_ROWS * nb * 4);
    s.bin_start = c.take<uint32_t>((nb + 1) * 4);
    s.block_off = c.take<uint32_t>(n_bin_blocks(n) * nb * 4);
    s.list_count = c.take<uint32_t>((nb << BIN_SHIFT) * 4);
    s.ranges = c.take<uint2>(nl * 8);
    s.order = c.take<uint32_t>(nl * 4);
    s.class_bounds = c.take<uint32_t>(8 * 4);
    s.kj = c.take<float>(n * 48);
    s.big_flag = c.take<uint32_t>(((n + 255) / 256 * 4) * 4);      // (one word per projection wave = range of 64 Gaussians)
    s.bytes = c.o;
    return s;
}

// Binning scratch: payloads in coarse-bin order, then in list order (unsorted inside a list), and the offsets the
// chunks of the split kernels drew inside their lists.
struct BinScratch {
    uint64_t* bvals;         // [P] bin order
    uint64_t* vals;          // [P] list order
    uint32_t* seg_off;       // [(chunks + bins) x 64]
    int64_t bytes;
};

inline int64_t n_chunks(int64_t n_pairs) { return (n_pairs + SPLIT_CHUNK - 1) / SPLIT_CHUNK; }

BinScratch carve_bin_scratch(void* base, int64_t n_pairs, int64_t nb) {
    BinScratch s;
    Carver c{(char*)base};
    const int64_t np = n_pairs > 0 ? n_pairs : 1;
    s.bvals = c.take<uint64_t>(np * 8);
    s.vals = c.take<uint64_t>(np * 8);
    s.seg_off = c.take<uint32_t>((n_chunks(np) + nb) * 64 * 4);
    s.bytes = c.o;
    return s;
}

// bin_state = sorted ids [capacity] (4 B each), then one byte per pair: the sub-tile mask gsplat_rasterize_forward leaves for
// gsplat_rasterize_backward when it is given `accum`
inline uint8_t* pair_mask_of(const void* bin_state, int64_t pair_capacity) {
    return (uint8_t*)bin_state + up((pair_capacity > 0 ? pair_capacity : 1) * 4);
}
inline int64_t bin_state_bytes(int64_t pair_capacity) {
    const int64_t cap = pair_capacity > 0 ? pair_capacity : 1;
    return up(cap * 4) + up(cap);
}

// Scratch of the deterministic backward: one row of `row` floats per (list, Gaussian) pair (9; 10 with the depth / opacity
// channels), each Gaussian's first slot, sums per block.
constexpr int PB_BLOCK = 2048;                       // Gaussians per block of tile_block_sum_kernel / pair_base_kernel
struct DetScratch { float* part; uint32_t* pair_base; uint32_t* block_sum; int64_t bytes; };
DetScratch carve_det(void* base, int64_t n, int64_t capacity, int row = 9) {
    DetScratch d;
    Carver c{(char*)base};
    d.part = c.take<float>((capacity > 0 ? capacity : 1) * 4 * row);
    d.pair_base = c.take<uint32_t>((n > 0 ? n : 1) * 4);
    d.block_sum = c.take<uint32_t>(((n > 0 ? n : 1) + PB_BLOCK - 1) / PB_BLOCK * 4);
    d.bytes = c.o;
    return d;
}

// The camera-pose scratch: one 64-byte row per block of 64 Gaussians, then POSE_PARTS partial rows.
constexpr int POSE_PARTS = 256;
struct PoseScratch { f4* rows; float* part; int64_t nrows, bytes; };
PoseScratch carve_pose(void* base, int64_t n) {
    PoseScratch p;
    Carver c{(char*)base};
    p.nrows = (n + 63) / 64;
    p.rows = c.take<f4>((p.nrows > 0 ? p.nrows : 1) * 64);
    p.part = c.take<float>((int64_t)POSE_PARTS * 64);
    p.bytes = c.o;
    return p;
}

// The frame arena of the composite entries: project_state | bin_state | accum | grad2d (the last two with GSPLAT_FRAME_BACKWARD;
// -1 without).
struct FrameParts { int64_t project_state, bin_state, accum, grad2d, total; };
FrameParts frame_parts(int64_t n, int64_t pair_capacity, const gsplat_view* v, int32_t flags) {
    FrameParts f;
    Carver c{nullptr};
    const auto off = [&](int64_t bytes) { return (int64_t)reinterpret_cast<intptr_t>(c.take<char>(bytes)); };
    f.project_state = off(carve_project(nullptr, n > 0 ? n : 1, n_lists(v)).bytes);
    f.bin_state = off(bin_state_bytes(pair_capacity));
    f.accum = f.grad2d = -1;
    if (flags & GSPLAT_FRAME_BACKWARD) {
        f.accum = off((int64_t)v->H * v->W * 3 * (int64_t)sizeof(float));
        f.grad2d = off((n > 0 ? n : 1) * 16 * (int64_t)sizeof(float));
    }
    f.total = c.o;
    return f;
}
// the forward pass clears grad2d on the side unless there are so few lists that a wave's share would be long
inline bool forward_clears_grad2d(int64_t n, const gsplat_view* v) { return n <= 256 * n_lists(v); }

// ---- grid sizes ----------------------------------------------------------------------------------------
inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }
// Dynamic LDS of the two binning kernels: nb counters -- padded so that only `per_cu` of their workgroups fit a CU when the image has
// many bins.  Every resident block of bin_scatter_kernel keeps one open line per bin it writes to; with 8 blocks per CU and the 1012
// bins of a 4K image that is 2 M lines under 32 MB of L2: lines leave half written and come back (config 5: 202 us at 3 blocks per
// CU, 285 at 8); a small image has few bins and wants the occupancy (config 6: 131 us at 3, 108 at 8).
inline size_t bin_lds_bytes(size_t nb, size_t static_bytes, size_t least = 2) {
    size_t per_cu = 2048 / (nb ? nb : 1);
    if (per_cu < least) per_cu = least;
    if (per_cu >= 8) return nb * 4;
    const size_t want = (160 * 1024) / (per_cu + 1) + 1024;          // one more block must not fit
    const size_t dyn = want > static_bytes ? want - static_bytes : 0;
    return std::min(std::max(nb * 4, dyn), (size_t)(64 * 1024 - 256));
}
// workgroups of the binning kernels that look for LARGE Gaussians (ranges of 64, grid-stride): enough to fill the chip when every
// Gaussian is large, few enough to cost a scene without any (config 3: 15 625 ranges, one flag word each) almost nothing
inline unsigned big_bin_blocks(int64_t n) { return std::min((unsigned)((n + 63) / 64), 2048u); }
// (bin_count_kernel: fewer, each adding its ranges up before it touches the global totals)
inline unsigned big_count_blocks(int64_t n) { return std::min((unsigned)((n + 63) / 64), 768u); }
inline unsigned blocks64(int64_t n) { return (unsigned)((n + 63) / 64); }

}  // namespace
