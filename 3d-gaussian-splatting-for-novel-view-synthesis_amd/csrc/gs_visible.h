// gs_visible.h -- the visible set of a frame: visible_set_kernel.
#pragma once
#include "gs_layout.h"

using namespace gsm;
namespace {

// A record is one byte per Gaussian.  Behind ONE frame, every Gaussian binned into at least one list (tiles[i] != 0: the rows
// densify_stats_kernel counts, and the only rows that can have a non-zero gradient) gets visible[i] = 1.  One Gaussian per lane.
// The record is never read and 0 is never stored: every store writes the same value, so frames on two streams may add into one
// record with no ordering between them (bits would need atomics for that; a byte costs 1 MB per million Gaussians and makes the
// data-parallel reduction a plain MAX).  The frame's own device counters decide, uniformly for the whole grid, whether anything is
// added, as in densify_stats_kernel: a frame with nothing on screen, or one whose pairs outgrew the pair capacity, adds nothing.
__global__ __launch_bounds__(256) void visible_set_kernel(int64_t n, const DevCounts* __restrict__ counts, long long capacity,
                                                          const uint32_t* __restrict__ tiles, uint8_t* __restrict__ visible) {
    if (counts->n_visible <= 0 || counts->n_binned > capacity) return;      // (uniform)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (tiles[i] != 0u) visible[i] = 1;
}

}  // namespace
