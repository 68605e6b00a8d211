// gsplat_exposure.hip -- per-view exposure compensation (not in the reference): the affine colour transform of a rendered
// frame, its two gradients, and the host entries that launch them.
//
// The kernels and the per-pixel arithmetic are gs_exposure.h (the arithmetic is shared with the host test build).  The gradient of
// the parameters is a full-frame reduction formed in a fixed order without float atomics: the same bits on every call, every stream
// and every launch.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_entry.h"
#include "gs_exposure.h"

namespace {

using namespace gsexp;

constexpr int64_t MAX_BATCH = 65535;                       // the grid's y extent
constexpr int64_t MAX_BLOCKS = 0x3FFFFFFF;                 // workgroups per image

int64_t image_blocks(int32_t H, int32_t W) { return ((int64_t)H * W + EXPOSURE_BLOCK_PIX - 1) / EXPOSURE_BLOCK_PIX; }

// the shape checks every entry shares; NULL when the shape is good
const char* shape_error(int64_t batch, int32_t H, int32_t W) {
    if (H <= 0) return "H must be > 0";
    if (W <= 0) return "W must be > 0";
    if (batch <= 0) return "batch must be > 0";
    if (batch > MAX_BATCH) return "batch must be <= 65535 (the grid's y extent)";
    if (image_blocks(H, W) > MAX_BLOCKS) return "the image is too large";
    return nullptr;
}

// 16-byte accesses: every array on a 16-byte boundary, and every image of a batch too (an image is 12 H W bytes)
int can_vectorise(std::initializer_list<const void*> ptrs, int64_t batch, int64_t pixels) {
    for (const void* q : ptrs)
        if (q && !aligned(q, 16)) return 0;
    return batch == 1 || pixels % 4 == 0;
}

}  // namespace

extern "C" {

// scratch = partial[image][workgroup of 1024 pixels][12] floats, rounded up to 256 bytes
int64_t gsplat_exposure_scratch_bytes(int64_t batch, int32_t H, int32_t W) {
    if (shape_error(batch, H, W)) return -1;
    return 256 * ((batch * image_blocks(H, W) * EXPOSURE_PARAMS * (int64_t)sizeof(float) + 255) / 256);
}

int gsplat_exposure_forward(const float* image, const float* params, int64_t batch, int32_t H, int32_t W, float* out, void* stream) {
    const char* E = "gsplat_exposure_forward";
    if (!image) return bad_arg(E, "image is NULL");
    if (!params) return bad_arg(E, "params is NULL");
    if (!out) return bad_arg(E, "out is NULL");
    if (const char* what = shape_error(batch, H, W)) return bad_arg(E, what);
    for (const void* p : {(const void*)image, (const void*)params, (const void*)out})
        if (!aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    const int64_t n = (int64_t)H * W;
    hipLaunchKernelGGL(exposure_forward_kernel, dim3((unsigned)image_blocks(H, W), (unsigned)batch), dim3(EXPOSURE_THREADS), 0, (hipStream_t)stream,
                       image, params, n, can_vectorise({image, out}, batch, n), out);
    return launch_err("gsplat_exposure_forward launch");
}

int gsplat_exposure_backward(const float* image, const float* params, const float* grad_out, int64_t batch, int32_t H, int32_t W,
                             float* grad_image, float* grad_params, const int32_t* row_index, int32_t flags, void* scratch, void* stream) {
    const char* E = "gsplat_exposure_backward";
    if (flags & ~GSPLAT_EXPOSURE_ACCUMULATE) return bad_arg(E, "unknown flag");
    if (!image) return bad_arg(E, "image is NULL");
    if (!params) return bad_arg(E, "params is NULL");
    if (!grad_out) return bad_arg(E, "grad_out is NULL");
    if (const char* what = shape_error(batch, H, W)) return bad_arg(E, what);
    if (grad_params && !scratch) return bad_arg(E, "scratch is NULL (grad_params needs gsplat_exposure_scratch_bytes of it)");
    for (const void* p : {(const void*)image, (const void*)params, (const void*)grad_out, (const void*)grad_image, (const void*)grad_params,
                          (const void*)row_index, (const void*)scratch})
        if (p && !aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    if (!grad_image && !grad_params) return GSPLAT_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)H * W, blocks = image_blocks(H, W);
    const dim3 grid((unsigned)blocks, (unsigned)batch), block(EXPOSURE_THREADS);
    const int vec = can_vectorise({image, grad_out, grad_image}, batch, n);
    float* partial = (float*)scratch;
    if (grad_image && grad_params)
        hipLaunchKernelGGL((exposure_backward_kernel<true, true>), grid, block, 0, st, image, params, grad_out, n, vec, grad_image, partial);
    else if (grad_image)
        hipLaunchKernelGGL((exposure_backward_kernel<true, false>), grid, block, 0, st, image, params, grad_out, n, vec, grad_image, partial);
    else
        hipLaunchKernelGGL((exposure_backward_kernel<false, true>), grid, block, 0, st, image, params, grad_out, n, vec, grad_image, partial);
    if (grad_params)
        hipLaunchKernelGGL(exposure_finish_kernel, dim3((unsigned)batch), block, 0, st, (const float*)partial, (int)blocks, row_index,
                           (int)(flags & GSPLAT_EXPOSURE_ACCUMULATE), grad_params);
    return launch_err("gsplat_exposure_backward launch");
}

}  // extern "C"
