// gsplat_knn.hip -- exact 3-nearest-neighbour mean squared distance of a point cloud (not in the reference): what
// the paper, simple_knn's distCUDA2 and gsplat's knn(points, 4) initialise the scales of the Gaussians from.
//
// The arithmetic and the definition are gs_knn.h (shared with the host test build).  The plan:
//   bbox     the bounding box of the finite rows and their number F: integer atomic min / max on order-preserving float bits, an
//            integer atomic add -- no float atomic anywhere in this file
//   keys     a 63-bit Morton key per row (non-finite rows: the largest key)
//   sort     stable LSD radix sort of (key, row), 8 passes of 8 bits: per-workgroup digit histogram, fixed-order scan, stable scatter
//   boxes    runs of GSPLAT_KNN_BOX sorted points: their positions as float4 (xyz + the row as bits) and the AABB of the ACTUAL points;
//            the non-finite rows (sorted positions F..n-1) get 0
//   search   one lane per query, in sorted order; own box first, then every other box whose AABB is not farther than the third-best
//            of every lane of the wave
// The sort decides how much is pruned, never the result: the search is exact whatever order the points are in.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_entry.h"
#include "gs_knn.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int BOX = GSPLAT_KNN_BOX;                          // points per box = threads of the boxes and search kernels
constexpr int BOX_WAVES = BOX / 64;
constexpr int RADIX = 256;                                   // 8-bit digits
constexpr int SORT_TILE = 2048;                              // keys per workgroup and pass
constexpr int MAX_BLOCKS = 4096;                             // the streaming kernels stride over the rest
constexpr int64_t MAX_ROWS = 0x7fffffff;

static_assert(BOX % 64 == 0 && BOX >= 64 && BOX <= 512, "a box is a whole number of waves and fits one workgroup's LDS");
static_assert(RADIX == THREADS, "one thread per digit in the histogram, the scan and the scatter");
static_assert(SORT_TILE % THREADS == 0, "a sort tile is a whole number of rounds");

// The first 256 bytes of the scratch.  lo / hi: ordered_bits() of the bounding box; zeroed (lo: all ones) by two memset nodes.
struct Header {
    uint32_t lo[3];
    uint32_t hi[3];
    uint32_t finite;                                         // F
};

struct Layout {
    int64_t bytes, keys[2], vals[2], sorted, box_lo, box_hi, hist, totals;
    int64_t sort_blocks, boxes;
};

inline int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

Layout layout(int64_t n) {
    Layout L;
    L.sort_blocks = n > 0 ? (n + SORT_TILE - 1) / SORT_TILE : 1;
    L.boxes = n > 0 ? (n + BOX - 1) / BOX : 1;
    int64_t at = 256;                                        // the header
    L.keys[0] = at; at += up256(n * 8);
    L.keys[1] = at; at += up256(n * 8);
    L.vals[0] = at; at += up256(n * 4);
    L.vals[1] = at; at += up256(n * 4);
    L.sorted = at; at += up256(n * 16);
    L.box_lo = at; at += up256(L.boxes * 16);
    L.box_hi = at; at += up256(L.boxes * 16);
    L.hist = at; at += up256(L.sort_blocks * RADIX * 4);
    L.totals = at; at += up256(RADIX * 4);
    L.bytes = at;
    return L;
}

// What a wave wrote to LDS is read by other lanes of the SAME wave (and the other way round): order the two for the compiler.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// Inclusive sum over the THREADS values of a workgroup in thread order, and their total.  Integers: any order gives the same bits.
__device__ __forceinline__ uint32_t block_scan_inclusive(uint32_t v, uint32_t* wave_total, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += t;
    }
    __syncthreads();                                         // the previous use of wave_total has been read
    if (lane == 63) wave_total[w] = v;
    __syncthreads();
    uint32_t add = 0;
    total = 0;
    for (int k = 0; k < WAVES; ++k) { if (k < w) add += wave_total[k]; total += wave_total[k]; }
    return v + add;
}

// ---- bounding box ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void knn_bbox_kernel(int64_t n, const float* __restrict__ pos, Header* hdr) {
    __shared__ uint32_t part[WAVES][7];
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u}, cnt = 0u;
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
        const float p[3] = {pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2]};
        if (!gsknn::finite_row(p[0], p[1], p[2])) continue;
        ++cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t o = gsknn::ordered_bits(p[a]);
            lo[a] = o < lo[a] ? o : lo[a];
            hi[a] = o > hi[a] ? o : hi[a];
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const uint32_t l = (uint32_t)__shfl_xor((int)lo[a], s), h = (uint32_t)__shfl_xor((int)hi[a], s);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
        cnt += (uint32_t)__shfl_xor((int)cnt, s);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int a = 0; a < 3; ++a) { part[w][a] = lo[a]; part[w][3 + a] = hi[a]; }
        part[w][6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < WAVES; ++k) {
            for (int a = 0; a < 3; ++a) {
                lo[a] = part[k][a] < lo[a] ? part[k][a] : lo[a];
                hi[a] = part[k][3 + a] > hi[a] ? part[k][3 + a] : hi[a];
            }
            cnt += part[k][6];
        }
        if (cnt != 0u) {
            for (int a = 0; a < 3; ++a) { atomicMin(&hdr->lo[a], lo[a]); atomicMax(&hdr->hi[a], hi[a]); }
            atomicAdd(&hdr->finite, cnt);
        }
    }
}

// ---- keys ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void knn_key_kernel(int64_t n, const float* __restrict__ pos, const Header* __restrict__ hdr,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = gsknn::ordered_float(hdr->lo[a]); hi[a] = gsknn::ordered_float(hdr->hi[a]); }
    const int64_t stride = (int64_t)gridDim.x * THREADS;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
        keys[i] = gsknn::morton_key(pos[i * 3], pos[i * 3 + 1], pos[i * 3 + 2], lo, hi);      // (a non-finite row never reads lo / hi)
        vals[i] = (uint32_t)i;
    }
}

// ---- stable LSD radix sort, one 8-bit pass: histogram, scan, scatter -------------------------------------------------------
// hist[d * sort_blocks + b] = the number of keys of tile b whose digit is d.
__global__ __launch_bounds__(THREADS) void knn_sort_hist_kernel(int64_t n, const uint64_t* __restrict__ keys, int shift, int64_t sort_blocks,
                                                                uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[RADIX];
    cnt[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_TILE / THREADS; ++r) {
        const int64_t i = base + (int64_t)r * THREADS + threadIdx.x;
        if (i < n) atomicAdd(&cnt[(uint32_t)(keys[i] >> shift) & (RADIX - 1)], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * sort_blocks + blockIdx.x] = cnt[threadIdx.x];
}

// One workgroup per digit: its row of the histogram becomes the exclusive sum over the tiles, in tile order; totals[d] = the row's sum.
__global__ __launch_bounds__(THREADS) void knn_sort_scan_kernel(int64_t sort_blocks, uint32_t* __restrict__ hist, uint32_t* __restrict__ totals) {
    __shared__ uint32_t wave_total[WAVES];
    uint32_t* row = hist + (int64_t)blockIdx.x * sort_blocks;
    uint32_t carry = 0u;
    for (int64_t b0 = 0; b0 < sort_blocks; b0 += THREADS) {
        const int64_t i = b0 + threadIdx.x;
        const uint32_t v = i < sort_blocks ? row[i] : 0u;
        uint32_t total;
        const uint32_t incl = block_scan_inclusive(v, wave_total, total);
        if (i < sort_blocks) row[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// Tile b writes its keys of digit d from (sum of totals below d) + hist[d][b] on, in the order it holds them: rounds of THREADS keys,
// the waves of a round one after the other, the lanes of a wave ranked among the lanes with the same digit (eight ballots).
__global__ __launch_bounds__(THREADS) void knn_sort_scatter_kernel(int64_t n, const uint64_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                                   int shift, int64_t sort_blocks, const uint32_t* __restrict__ hist,
                                                                   const uint32_t* __restrict__ totals, uint64_t* __restrict__ keys_out,
                                                                   uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t next[RADIX];
    __shared__ uint32_t wave_total[WAVES];
    {
        const uint32_t t = totals[threadIdx.x];
        uint32_t total;
        const uint32_t incl = block_scan_inclusive(t, wave_total, total);
        next[threadIdx.x] = incl - t + hist[(int64_t)threadIdx.x * sort_blocks + blockIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
    for (int r = 0; r < SORT_TILE / THREADS; ++r) {
        if (base + (int64_t)r * THREADS >= n) break;                                   // (the same in every thread)
        const int64_t i = base + (int64_t)r * THREADS + threadIdx.x;
        const bool valid = i < n;
        const uint64_t key = valid ? keys_in[i] : 0ull;
        const uint32_t val = valid ? vals_in[i] : 0u;
        const uint32_t digit = (uint32_t)(key >> shift) & (RADIX - 1);
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (digit >> bit) & 1u;
            const uint64_t m = __ballot(valid && set);
            peers &= set ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull)), same = (uint32_t)__popcll(peers);
        uint32_t off = 0u;
        for (int w = 0; w < WAVES; ++w) {
            if (wave == w) {
                if (valid) off = next[digit];
                wave_lds_sync();
                if (valid && rank == 0u) next[digit] = off + same;
            }
            __syncthreads();
        }
        if (valid) { keys_out[off + rank] = key; vals_out[off + rank] = val; }
    }
}

// ---- boxes -----------------------------------------------------------------------------------------------------------------
// Workgroup b: the sorted positions b BOX .. of the finite rows as float4 (xyz, row) and their AABB; a non-finite row gets its 0.
__global__ __launch_bounds__(BOX) void knn_boxes_kernel(int64_t n, const float* __restrict__ pos, const Header* __restrict__ hdr,
                                                        const uint32_t* __restrict__ vals, float4* __restrict__ sorted,
                                                        float4* __restrict__ box_lo, float4* __restrict__ box_hi, float* __restrict__ dist2) {
    __shared__ float part[BOX_WAVES][6];
    const int64_t F = hdr->finite, p = (int64_t)blockIdx.x * BOX + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (p < n) {
        const uint32_t row = vals[p];
        if (p < F) {
            const float x = pos[(int64_t)row * 3], y = pos[(int64_t)row * 3 + 1], z = pos[(int64_t)row * 3 + 2];
            sorted[p] = make_float4(x, y, z, gsknn::bits_float(row));
            lo[0] = hi[0] = x; lo[1] = hi[1] = y; lo[2] = hi[2] = z;
        } else {
            dist2[row] = 0.f;
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float l = __shfl_xor(lo[a], s), h = __shfl_xor(hi[a], s);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) { part[w][a] = lo[a]; part[w][3 + a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x == 0 && (int64_t)blockIdx.x * BOX < F) {
        for (int k = 1; k < BOX_WAVES; ++k)
            for (int a = 0; a < 3; ++a) {
                lo[a] = part[k][a] < lo[a] ? part[k][a] : lo[a];
                hi[a] = part[k][3 + a] > hi[a] ? part[k][3 + a] : hi[a];
            }
        box_lo[blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.f);
        box_hi[blockIdx.x] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// The wave copies box b's points into ITS part of the LDS and every lane runs its query over them, each point read at a wave-uniform
// address (a broadcast), four points per wait.  The slots past the box's last point are filled with points at +inf: their d2 is +inf,
// which insert3 ignores, so the loop runs over whole groups of four.  SELF: b is the wave's own box, and the lane's own sorted
// position is left out -- by index, so a duplicate of the query counts at distance 0.
template <bool SELF>
__device__ __forceinline__ void scan_box(const float4* __restrict__ sorted, int64_t F, int64_t b, float4* buf, const float4& q, int64_t self,
                                         float& b0, float& b1, float& b2) {
    const int lane = threadIdx.x & 63;
    const int64_t first = b * BOX;
    const int cnt = F - first < BOX ? (int)(F - first) : BOX;
    float4 in[BOX_WAVES];
#pragma unroll
    for (int k = 0; k < BOX_WAVES; ++k) {                    // (all loads in flight before the first write)
        const int j = k * 64 + lane;
        in[k] = sorted[first + (j < cnt ? j : cnt - 1)];
        if (j >= cnt) in[k] = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    }
    wave_lds_sync();                                         // every lane is done with what the buffer held
#pragma unroll
    for (int k = 0; k < BOX_WAVES; ++k) buf[k * 64 + lane] = in[k];
    wave_lds_sync();
    for (int j = 0; j < cnt; j += 4) {
        float4 c[4] = {buf[j], buf[j + 1], buf[j + 2], buf[j + 3]};
        // keep each read one 16-byte access (the 12-byte one the compiler would narrow it to takes twice the LDS cycles)
        asm volatile("" : "+v"(c[0].w), "+v"(c[1].w), "+v"(c[2].w), "+v"(c[3].w));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float d = gsknn::dist2_points(q.x, q.y, q.z, c[k].x, c[k].y, c[k].z);
            if (SELF) d = first + j + k == self ? INFINITY : d;
            gsknn::insert3(b0, b1, b2, d);
        }
    }
}

// Workgroup b: the queries of box b, one per lane.  Its own box first (a tight third-best at once), then every other box: the AABBs are
// staged in LDS BOX at a time and read at a wave-uniform address; a box is skipped when its distance is STRICTLY greater than the
// third-best of every lane of the wave (one ballot).  dist2_box never exceeds dist2_points to a point inside (gs_knn.h), so a box that
// holds one of a lane's three nearest -- or a point that ties with the third -- is never skipped by that lane's wave.
__global__ __launch_bounds__(BOX) void knn_search_kernel(const Header* __restrict__ hdr, const float4* __restrict__ sorted,
                                                         const float4* __restrict__ box_lo, const float4* __restrict__ box_hi,
                                                         float* __restrict__ dist2) {
    __shared__ float4 aabb[BOX * 2];
    __shared__ float4 stage[BOX_WAVES][BOX];
    const int64_t F = hdr->finite, own = blockIdx.x, first = own * BOX;
    if (first >= F) return;                                  // (the whole workgroup: the grid is sized for n, F is known on the device only)
    const int64_t boxes = (F + BOX - 1) / BOX, self = first + threadIdx.x;
    const bool valid = self < F;
    const float4 q = sorted[valid ? self : first];
    float4* buf = stage[threadIdx.x >> 6];
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    scan_box<true>(sorted, F, own, buf, q, self, b0, b1, b2);
    for (int64_t c0 = 0; c0 < boxes; c0 += BOX) {
        const int cnt = boxes - c0 < BOX ? (int)(boxes - c0) : BOX;
        __syncthreads();                                     // the previous chunk has been read
        if ((int)threadIdx.x < cnt) {
            aabb[threadIdx.x * 2] = box_lo[c0 + threadIdx.x];
            aabb[threadIdx.x * 2 + 1] = box_hi[c0 + threadIdx.x];
        }
        __syncthreads();
        for (int c = 0; c < cnt; ++c) {
            if (c0 + c == own) continue;
            const float4 lo = aabb[c * 2], hi = aabb[c * 2 + 1];
            const float gap = gsknn::dist2_box(q.x, q.y, q.z, lo.x, lo.y, lo.z, hi.x, hi.y, hi.z);
            if (__ballot(valid && !(gap > b2)) == 0ull) continue;
            scan_box<false>(sorted, F, c0 + c, buf, q, self, b0, b1, b2);
        }
    }
    if (valid) dist2[gsknn::float_bits(q.w)] = gsknn::mean_smallest(b0, b1, b2, F - 1);
}

unsigned stream_blocks(int64_t items) {
    const int64_t b = (items + THREADS - 1) / THREADS;
    return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

}  // namespace

extern "C" {

int64_t gsplat_knn_scratch_bytes(int64_t n) {
    if (n < 0 || n > MAX_ROWS) return -1;
    return layout(n).bytes;
}

int gsplat_knn_mean_dist2(int64_t n, const float* points, float* dist2, void* scratch, void* stream) {
    const char* E = "gsplat_knn_mean_dist2";
    if (n < 0 || n > MAX_ROWS) return bad_arg(E, "n must be in [0, 2^31)");
    if (n == 0) return GSPLAT_OK;
    if (!points) return bad_arg(E, "points is NULL");
    if (!dist2) return bad_arg(E, "dist2 is NULL");
    if (!scratch) return bad_arg(E, "scratch is NULL");
    if (!aligned(points, 4)) return bad_arg(E, "points must be 4-byte aligned");
    if (!aligned(dist2, 4)) return bad_arg(E, "dist2 must be 4-byte aligned");
    if (!aligned(scratch, 256)) return bad_arg(E, "scratch must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const Layout L = layout(n);
    char* s = (char*)scratch;
    Header* hdr = (Header*)s;
    uint64_t* keys[2] = {(uint64_t*)(s + L.keys[0]), (uint64_t*)(s + L.keys[1])};
    uint32_t* vals[2] = {(uint32_t*)(s + L.vals[0]), (uint32_t*)(s + L.vals[1])};
    float4* sorted = (float4*)(s + L.sorted);
    float4 *box_lo = (float4*)(s + L.box_lo), *box_hi = (float4*)(s + L.box_hi);
    uint32_t *hist = (uint32_t*)(s + L.hist), *totals = (uint32_t*)(s + L.totals);

    (void)hipMemsetAsync(hdr, 0, 256, st);
    (void)hipMemsetAsync(hdr->lo, 0xff, sizeof(hdr->lo), st);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(stream_blocks(n)), dim3(THREADS), 0, st, n, points, hdr);
    hipLaunchKernelGGL(knn_key_kernel, dim3(stream_blocks(n)), dim3(THREADS), 0, st, n, points, (const Header*)hdr, keys[0], vals[0]);
    int from = 0;
    for (int shift = 0; shift < 64; shift += 8, from ^= 1) {
        hipLaunchKernelGGL(knn_sort_hist_kernel, dim3((unsigned)L.sort_blocks), dim3(THREADS), 0, st, n, (const uint64_t*)keys[from], shift,
                           L.sort_blocks, hist);
        hipLaunchKernelGGL(knn_sort_scan_kernel, dim3(RADIX), dim3(THREADS), 0, st, L.sort_blocks, hist, totals);
        hipLaunchKernelGGL(knn_sort_scatter_kernel, dim3((unsigned)L.sort_blocks), dim3(THREADS), 0, st, n, (const uint64_t*)keys[from],
                           (const uint32_t*)vals[from], shift, L.sort_blocks, (const uint32_t*)hist, (const uint32_t*)totals, keys[from ^ 1],
                           vals[from ^ 1]);
    }
    hipLaunchKernelGGL(knn_boxes_kernel, dim3((unsigned)L.boxes), dim3(BOX), 0, st, n, points, (const Header*)hdr, (const uint32_t*)vals[from],
                       sorted, box_lo, box_hi, dist2);
    hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)L.boxes), dim3(BOX), 0, st, (const Header*)hdr, (const float4*)sorted,
                       (const float4*)box_lo, (const float4*)box_hi, dist2);
    return launch_err(E);
}

}  // extern "C"
