// gsplat_pose_delta.hip -- per-view camera-pose corrections (not in the reference): the composition of a pose with its
// nine-float correction, its two gradients, the table's decay term, and the host entries that launch them.
//
// The kernels and the per-view arithmetic are gs_pose_delta.h (the arithmetic is shared with the host test build).  One lane per
// view, one launch per entry, no scratch and no atomics: the same bits on every call, every stream and every launch.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_entry.h"
#include "gs_pose_delta.h"

namespace {

using namespace gspd;

constexpr int64_t MAX_VIEWS = (int64_t)1 << 30;            // 2^24 workgroups of 64 lanes

unsigned view_blocks(int64_t n) { return (unsigned)((n + POSE_DELTA_THREADS - 1) / POSE_DELTA_THREADS); }

}  // namespace

extern "C" {

int gsplat_pose_delta_forward(const float* c2w, const float* delta, int64_t batch, float* out, void* stream) {
    const char* E = "gsplat_pose_delta_forward";
    if (!c2w) return bad_arg(E, "c2w is NULL");
    if (!delta) return bad_arg(E, "delta is NULL");
    if (!out) return bad_arg(E, "out is NULL");
    if (batch < 1) return bad_arg(E, "batch must be > 0");
    if (batch > MAX_VIEWS) return bad_arg(E, "batch must be <= 2^30");
    for (const void* p : {(const void*)c2w, (const void*)delta, (const void*)out})
        if (!aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    hipLaunchKernelGGL(pose_delta_forward_kernel, dim3(view_blocks(batch)), dim3(POSE_DELTA_THREADS), 0, (hipStream_t)stream, c2w, delta, batch, out);
    return launch_err("gsplat_pose_delta_forward launch");
}

int gsplat_pose_delta_backward(const float* c2w, const float* delta, const float* grad_out, int64_t batch, float* grad_c2w, float* grad_delta,
                               const int32_t* row_index, int32_t flags, void* stream) {
    const char* E = "gsplat_pose_delta_backward";
    if (flags & ~GSPLAT_POSE_DELTA_ACCUMULATE) return bad_arg(E, "unknown flag");
    if (!c2w) return bad_arg(E, "c2w is NULL");
    if (!delta) return bad_arg(E, "delta is NULL");
    if (!grad_out) return bad_arg(E, "grad_out is NULL");
    if (batch < 1) return bad_arg(E, "batch must be > 0");
    if (batch > MAX_VIEWS) return bad_arg(E, "batch must be <= 2^30");
    for (const void* p : {(const void*)c2w, (const void*)delta, (const void*)grad_out, (const void*)grad_c2w, (const void*)grad_delta,
                          (const void*)row_index})
        if (p && !aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    if (!grad_c2w && !grad_delta) return GSPLAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(view_blocks(batch)), block(POSE_DELTA_THREADS);
    const int add = (int)(flags & GSPLAT_POSE_DELTA_ACCUMULATE);
    if (grad_c2w && grad_delta)
        hipLaunchKernelGGL((pose_delta_backward_kernel<true, true>), grid, block, 0, st, c2w, delta, grad_out, batch, grad_c2w, grad_delta, row_index, add);
    else if (grad_c2w)
        hipLaunchKernelGGL((pose_delta_backward_kernel<true, false>), grid, block, 0, st, c2w, delta, grad_out, batch, grad_c2w, grad_delta, row_index, add);
    else
        hipLaunchKernelGGL((pose_delta_backward_kernel<false, true>), grid, block, 0, st, c2w, delta, grad_out, batch, grad_c2w, grad_delta, row_index, add);
    return launch_err("gsplat_pose_delta_backward launch");
}

int gsplat_pose_delta_decay(const float* delta, int64_t n_views, float reg, float* grad, void* stream) {
    const char* E = "gsplat_pose_delta_decay";
    if (!delta) return bad_arg(E, "delta is NULL");
    if (!grad) return bad_arg(E, "grad is NULL");
    if (n_views < 1) return bad_arg(E, "n_views must be > 0");
    if (n_views > MAX_VIEWS) return bad_arg(E, "n_views must be <= 2^30");
    if (!aligned(delta, 4) || !aligned(grad, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    hipLaunchKernelGGL(pose_delta_decay_kernel, dim3(view_blocks(n_views)), dim3(POSE_DELTA_THREADS), 0, (hipStream_t)stream, delta, n_views, reg, grad);
    return launch_err("gsplat_pose_delta_decay launch");
}

}  // extern "C"
