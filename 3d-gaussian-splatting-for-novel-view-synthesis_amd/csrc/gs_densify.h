// gs_densify.h -- screen-space densification statistics: densify_stats_kernel, densify_stats_merge_kernel.
#pragma once
#include "gs_layout.h"

using namespace gsm;
namespace {

// A record is one f4 row per Gaussian: (grad_sum, count, extent_max, 0).
//
// densify_stats_kernel: behind the raster backward of ONE frame, every Gaussian binned into at least one list (tiles[i] != 0) adds
//     grad_sum  += sqrt((g_u W/2)^2 + (g_v H/2)^2)      g_u = o (A11 Mx + A12 My), g_v = o (A12 Mx + A22 My): the gradient of the
//                                                       projected centre in the moments form of project_backward_core (gs_body.h),
//                                                       (Mx, My) = columns 0-1 of grad2d; NDC units
//     count     += 1
//     extent_max = max(extent_max, min(max(ex, ey), 250))      (ex, ey): the record's half-extents of {q <= chi_square_clip}
// One Gaussian per lane, no LDS, no atomics.  A row of a Gaussian that is not visible is neither read nor written.  The frame's
// own device counters decide, uniformly for the whole grid, whether anything is added: a frame with nothing on screen, or one whose
// pairs outgrew the pair capacity (its grad2d is garbage; the condition of the folded Adam step, gs_project_backward.h), adds nothing.
//
// ORDERING: the accumulation is a plain read-modify-write of the row.  Calls that add into the same record must be ordered on one
// stream (or by events); two streams that add into one record at the same time lose updates.
constexpr float DENSIFY_EXTENT_MAX = 250.f;      // 2.5 sqrt(1e4): the largest radius of the reference (eigenvalues clamped at 1e4)

//
// ABS (gsplat_densify_stats_abs): behind an absolute-gradient raster backward, columns 10-11 of grad2d hold
// Sx = sum |a (A11 du + A12 dv)|, Sy = sum |a (A12 du + A22 dv)| over the Gaussian's pixels, and
//     grad_sum  += sqrt((o Sx W/2)^2 + (o Sy H/2)^2)
// -- the per-pixel gradients of the centre added by magnitude, nothing left to cancel.  Everything else is the same.
template <bool ABS = false>
__global__ __launch_bounds__(256) void densify_stats_kernel(int64_t n, const DevCounts* __restrict__ counts, long long capacity,
                                                            const uint32_t* __restrict__ tiles, const Rec64* __restrict__ rec,
                                                            const float* __restrict__ grad2d, float half_w, float half_h,
                                                            f4* __restrict__ stats) {
    if (counts->n_visible <= 0 || counts->n_binned > capacity) return;      // (uniform)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || tiles[i] == 0u) return;
    const f4 r0 = rec[i].r0, r1 = rec[i].r1;          // (u, v, A11, A12), (A22, opacity, ex, ey)
    float gu, gv;
    if constexpr (ABS) {
        gu = r1.y * grad2d[i * 16 + 10] * half_w;
        gv = r1.y * grad2d[i * 16 + 11] * half_h;
    } else {
        const float mx = grad2d[i * 16], my = grad2d[i * 16 + 1];
        gu = r1.y * (r0.z * mx + r0.w * my) * half_w;
        gv = r1.y * (r0.w * mx + r1.x * my) * half_h;
    }
    f4 s = stats[i];
    s.x += sqrtf(gu * gu + gv * gv);
    s.y += 1.f;
    s.z = fmaxf(s.z, fminf(fmaxf(r1.z, r1.w), DENSIFY_EXTENT_MAX));
    stats[i] = s;
}

// total (+)= pass -- (sum, sum, max) -- for the rows the pass touched (count > 0), which are written back as zeros: a pass record is
// zero again after a merge, without a clearing launch.  A row the pass did not touch costs one 16-byte read.
__global__ __launch_bounds__(256) void densify_stats_merge_kernel(int64_t n, f4* __restrict__ pass, f4* __restrict__ total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const f4 p = pass[i];
    if (!(p.y > 0.f)) return;
    f4 t = total[i];
    t.x += p.x;
    t.y += p.y;
    t.z = fmaxf(t.z, p.z);
    total[i] = t;
    pass[i] = f4{0.f, 0.f, 0.f, 0.f};
}

}  // namespace
