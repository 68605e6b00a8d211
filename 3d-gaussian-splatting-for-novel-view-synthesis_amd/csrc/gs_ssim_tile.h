// gs_ssim_tile.h -- the tile pieces the SSIM kernels share: the training loss (gsplat_loss.hip: loss_stats_kernel,
// loss_grad_kernel) and the held-out metric (gsplat_metrics.hip: metrics_stats_kernel) filter the same 32 x 16 tile with the same taps
// through the same LDS layout, so the metric cannot drift from the loss it reports on.  Device code only.
//
// What is here: the tile geometry and the LDS pitches, the taps, the walk over a region with its 5-pixel halo, the horizontal pass
// (one thread's row of N planes; the five planes x, y, x^2, y^2, (x - y)^2 of the statistics kernels) and the vertical pass (gather,
// taps).
// What is NOT here, on purpose: what a kernel makes of mu1, mu2, e11, e22, edd -- the loss takes two v_rcp_f32 and writes three
// derivative maps, the metric divides in IEEE with contraction off -- and its accumulators, mask and correction.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int TW = 32, TH = 16, R = 5, TAPS = 11;
constexpr int W1 = TW + 2 * R, H1 = TH + 2 * R;      // region with one halo   42 x 26
constexpr int THREADS = 256;
constexpr int G = 4;                                 // outputs per thread along a row in the horizontal passes
constexpr int GV = 2;                                // rows per thread in the vertical passes
static_assert(TW % G == 0 && TH % GV == 0 && (TH / GV) * TW == THREADS, "tile shape vs register blocking");

// LDS access patterns.  Horizontal passes: lanes run over ROWS (row index fastest), every lane reads G + 10 = 14 consecutive words of
// its own row as 3 x 16 + 8 bytes and writes G = 4 words as 16 bytes; the row pitches are multiples of 4 words (alignment) chosen so
// that the 8 lanes a 16-byte access serves per cycle fall on 8 disjoint groups of 4 banks (44 r mod 32 = 0, 12, 24, 4, 16, 28, 8, 20;
// 36 r mod 32 = 0, 4, ... 28).  (Odd pitches with 4-byte accesses, the first version: 14 + 14 instead of 4 + 4 LDS instructions per
// thread and pass, 30-37 % of the LDS cycles bank conflicts.)  Vertical passes: lanes run over the 32 columns of a row group, two
// row groups per wave: consecutive words.
constexpr int XP = 44;           // pitch of the input planes / the map planes (W1 = 42 columns)
constexpr int HP = 36;           // pitch of the horizontally filtered planes (TW = 32 columns)
static_assert(XP >= W1 && XP % 4 == 0 && HP >= TW && HP % 4 == 0, "row pitches: 16-byte rows");

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));
// 14 consecutive floats of an LDS row from a 16-byte aligned position
__device__ __forceinline__ void load14(const float* p, float (&a)[G + 10]) {
    const f4v v0 = *reinterpret_cast<const f4v*>(p), v1 = *reinterpret_cast<const f4v*>(p + 4), v2 = *reinterpret_cast<const f4v*>(p + 8);
    const f2v v3 = *reinterpret_cast<const f2v*>(p + 12);
    a[0] = v0.x; a[1] = v0.y; a[2] = v0.z; a[3] = v0.w; a[4] = v1.x; a[5] = v1.y; a[6] = v1.z; a[7] = v1.w;
    a[8] = v2.x; a[9] = v2.y; a[10] = v2.z; a[11] = v2.w; a[12] = v3.x; a[13] = v3.y;
}
static_assert(G == 4, "load14 / the 16-byte stores assume four outputs per thread");

__device__ __forceinline__ void gauss_taps(float g[TAPS]) {
    // losses.py:131-155: exp(-(i - 5)^2 / (2 * 1.5^2)), normalised
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < TAPS; ++i) { const float d = (float)(i - R); g[i] = expf(-(d * d) / 4.5f); s += g[i]; }
    const float inv = 1.0f / s;
    // (the same eleven values in every lane: kept in SGPRs, they cost no vector register)
#pragma unroll
    for (int i = 0; i < TAPS; ++i) g[i] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(g[i] * inv)));
}

struct alignas(16) StatsLds {
    float x[3][H1][XP], y[3][H1][XP];     // the three channels of the region, de-interleaved
    float h[5][H1][HP];                   // horizontally filtered x, y, xx, yy, (x - y)^2 of the channel being processed
};
static_assert(sizeof(StatsLds) <= 52 * 1024, "three workgroups per CU");

// The walk over the H1 x W1 region of a tile with its halo: (r, c) of this thread's region pixels e = tid + 256 k, k = 0 .. REGION_SLOTS - 1
// -- stepped, not divided: 256 = 6 * 42 + 4.  The last slot runs past the region for most threads: r >= H1 there.
//     RegionWalk p(tid);
//     for (int k = 0; k < REGION_SLOTS; ++k, p.next()) ... p.r, p.c ...           (fully unrolled)
// A kernel stages its region in TWO such loops over register arrays of its own: the first loads into them -- EVERY load of the
// workgroup in flight together (one exposed round trip per workgroup; fetched channel by channel, with the next channel's prefetch in
// registers, a workgroup waited for memory three times: 87 -> 63 us was the LDS side, this is the other half) -- and the second stores
// them to LDS.  (An iterator, not a function that takes the loop body: with the bodies in closures the compiler groups the register
// arrays and the image addresses differently and loss_stats_kernel grows by 9 to 107 instructions; this way it is the same code.
// For the same reason gy = y0 - R + p.r, gx = x0 - R + p.c and the test "r < H1 && gy, gx inside the image" stay written out at the
// three sites ON PURPOSE: from a helper the kernel is one instruction longer.)
constexpr int REGION_SLOTS = (H1 * W1 + THREADS - 1) / THREADS;
struct RegionWalk {
    int r, c;
    __device__ __forceinline__ explicit RegionWalk(int tid) : r(tid / W1), c(tid - r * W1) {}
    __device__ __forceinline__ void next() {
        r += 6; c += 4;
        if (c >= W1) { c -= W1; ++r; }
    }
};
static_assert(THREADS == 6 * W1 + 4, "RegionWalk::next");

// Horizontal pass: thread i < H1 * (TW / G) of the workgroup filters columns c .. c + G of row r, r = i % H1 (rows fastest across
// lanes), c = (i / H1) * G: load14 of each input plane, then G outputs of each of N planes from their G + 10 inputs -> h[k][r][c .. c + G)
template <int N>
__device__ __forceinline__ void filter_row(const float (&g)[TAPS], const float (&v)[N][G + 10], float (&h)[N][H1][HP], int r, int c) {
    f4v out[N];
#pragma unroll
    for (int o = 0; o < G; ++o) {
        float a[N];
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] = 0.f;
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const float w = g[t];
#pragma unroll
            for (int k = 0; k < N; ++k) a[k] += w * v[k][o + t];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) out[k][o] = a[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) *reinterpret_cast<f4v*>(&h[k][r][c]) = out[k];
}

// The five planes x, y, x^2, y^2, (x - y)^2 of the statistics kernels from v[0] = x and v[1] = y (the products formed once per input)
__device__ __forceinline__ void stats_planes(float (&v)[5][G + 10]) {
#pragma unroll
    for (int t = 0; t < G + 10; ++t) { const float d = v[0][t] - v[1][t]; v[2][t] = v[0][t] * v[0][t]; v[3][t] = v[1][t] * v[1][t]; v[4][t] = d * d; }
}

// Vertical pass: column c of N filtered planes [H1][HP] from row r0 down, GV + 10 rows (top = &h[0][r0][c]), and output row o of
// them (for N = 5: mu1, mu2, e11, e22, edd)
template <int N>
__device__ __forceinline__ void gather_column(const float* top, float (&v)[N][GV + 10]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int t = 0; t < GV + 10; ++t) v[k][t] = top[(k * H1 + t) * HP];
}
template <int N>
__device__ __forceinline__ void filter_column(const float (&g)[TAPS], const float (&v)[N][GV + 10], int o, float (&out)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = 0.f;
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
        const float w = g[t];
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] += w * v[k][o + t];
    }
}

}  // namespace
