// gsplat_bilagrid.hip -- per-view bilateral grids (not in the reference): the slice of a grid of affine colour transforms
// at (x, y, luminance) applied to a rendered frame, its two gradients, the total variation of a table of grids, and the host entries
// that launch them.
//
// The kernels and the per-pixel arithmetic are gs_bilagrid.h (the arithmetic is shared with the host test build).  The gradient of a
// grid is a gather -- one workgroup per spatial vertex, sums in a fixed order, no float atomics: the same bits on every call, every
// stream and every launch.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"
#include "gs_entry.h"
#include "gs_bilagrid.h"

namespace {

using namespace gsbila;

constexpr int64_t MAX_BATCH = 65535;                       // the grid's y and z extents
constexpr int64_t MAX_BLOCKS = 0x3FFFFFFF;                 // workgroups along x
constexpr int32_t MAX_SIDE = 1 << 20;                      // H, W: pixel centres and cell boundaries stay apart in fp32 (gs_bilagrid.h, support())

const char* grid_error(int32_t X, int32_t Y, int32_t L) {
    if (X < BILAGRID_MIN || X > BILAGRID_MAX_XY) return "X must be in [2, 64]";
    if (Y < BILAGRID_MIN || Y > BILAGRID_MAX_XY) return "Y must be in [2, 64]";
    if (L < BILAGRID_MIN || L > BILAGRID_MAX_L) return "L must be in [2, 16]";
    return nullptr;
}

int64_t image_blocks(int32_t H, int32_t W) { return ((int64_t)H * W + BILAGRID_BLOCK_PIX - 1) / BILAGRID_BLOCK_PIX; }

// the shape checks the two slice entries share; NULL when the shape is good
const char* shape_error(int64_t batch, int32_t H, int32_t W, int32_t X, int32_t Y, int32_t L) {
    if (H <= 0 || H > MAX_SIDE) return "H must be in [1, 1048576]";
    if (W <= 0 || W > MAX_SIDE) return "W must be in [1, 1048576]";
    if (batch <= 0) return "batch must be > 0";
    if (batch > MAX_BATCH) return "batch must be <= 65535 (the grid's y extent)";
    if ((int64_t)H * W > 0x7FFFFFFF) return "the image is too large (H W must be < 2^31)";
    return grid_error(X, Y, L);
}

// the TV launch: one workgroup per chunk of 256 elements of a plane (image, channel) of L Y X elements
int64_t tv_chunks(int32_t X, int32_t Y, int32_t L) { return ((int64_t)L * Y * X + BILAGRID_THREADS - 1) / BILAGRID_THREADS; }
int64_t tv_blocks(int64_t V, int32_t X, int32_t Y, int32_t L) { return V * BILAGRID_CHANNELS * tv_chunks(X, Y, L); }

const char* tv_shape_error(int64_t V, int32_t X, int32_t Y, int32_t L) {
    if (V <= 0) return "V must be > 0";
    if (const char* what = grid_error(X, Y, L)) return what;
    if (V > MAX_BLOCKS / BILAGRID_CHANNELS) return "V is too large (the table must fit one launch)";
    return nullptr;
}

}  // namespace

extern "C" {

int gsplat_bilagrid_forward(const float* image, const float* grids, int64_t batch, int32_t H, int32_t W, int32_t X, int32_t Y, int32_t L,
                            float* out, void* stream) {
    const char* E = "gsplat_bilagrid_forward";
    if (!image) return bad_arg(E, "image is NULL");
    if (!grids) return bad_arg(E, "grids is NULL");
    if (!out) return bad_arg(E, "out is NULL");
    if (const char* what = shape_error(batch, H, W, X, Y, L)) return bad_arg(E, what);
    for (const void* p : {(const void*)image, (const void*)grids, (const void*)out})
        if (!aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    hipLaunchKernelGGL((bilagrid_pixel_kernel<false>), dim3((unsigned)image_blocks(H, W), (unsigned)batch), dim3(BILAGRID_THREADS), 0,
                       (hipStream_t)stream, image, grids, (const float*)nullptr, H, W, X, Y, L, out);
    return launch_err("gsplat_bilagrid_forward launch");
}

int gsplat_bilagrid_backward(const float* image, const float* grids, const float* grad_out, int64_t batch, int32_t H, int32_t W, int32_t X,
                             int32_t Y, int32_t L, float* grad_image, float* grad_grids, const int32_t* row_index, int32_t flags, void* stream) {
    const char* E = "gsplat_bilagrid_backward";
    if (flags & ~GSPLAT_BILAGRID_ACCUMULATE) return bad_arg(E, "unknown flag");
    if (!image) return bad_arg(E, "image is NULL");
    if (!grids) return bad_arg(E, "grids is NULL");
    if (!grad_out) return bad_arg(E, "grad_out is NULL");
    if (const char* what = shape_error(batch, H, W, X, Y, L)) return bad_arg(E, what);
    for (const void* p : {(const void*)image, (const void*)grids, (const void*)grad_out, (const void*)grad_image, (const void*)grad_grids,
                          (const void*)row_index})
        if (p && !aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    if (!grad_image && !grad_grids) return GSPLAT_OK;
    hipStream_t st = (hipStream_t)stream;
    if (grad_image)
        hipLaunchKernelGGL((bilagrid_pixel_kernel<true>), dim3((unsigned)image_blocks(H, W), (unsigned)batch), dim3(BILAGRID_THREADS), 0, st,
                           image, grids, grad_out, H, W, X, Y, L, grad_image);
    if (grad_grids)
        hipLaunchKernelGGL(bilagrid_gather_kernel, dim3((unsigned)X, (unsigned)Y, (unsigned)batch), dim3(BILAGRID_GATHER_THREADS), 0, st, image, grad_out,
                           H, W, X, Y, L, row_index, (int)(flags & GSPLAT_BILAGRID_ACCUMULATE), grad_grids);
    return launch_err("gsplat_bilagrid_backward launch");
}

// scratch = one double per workgroup (V 12 planes, ceil(L Y X / 256) chunks each), rounded up to 256 bytes
int64_t gsplat_bilagrid_tv_scratch_bytes(int64_t V, int32_t X, int32_t Y, int32_t L) {
    if (tv_shape_error(V, X, Y, L)) return -1;
    return 256 * ((tv_blocks(V, X, Y, L) * (int64_t)sizeof(double) + 255) / 256);
}

int gsplat_bilagrid_tv(const float* grids, int64_t V, int32_t X, int32_t Y, int32_t L, float scale, float* loss_out, float* grad, int32_t flags,
                       void* scratch, void* stream) {
    const char* E = "gsplat_bilagrid_tv";
    if (flags & ~GSPLAT_BILAGRID_ACCUMULATE) return bad_arg(E, "unknown flag");
    if (!grids) return bad_arg(E, "grids is NULL");
    if (const char* what = tv_shape_error(V, X, Y, L)) return bad_arg(E, what);
    if (loss_out && !scratch) return bad_arg(E, "scratch is NULL (loss_out needs gsplat_bilagrid_tv_scratch_bytes of it)");
    for (const void* p : {(const void*)grids, (const void*)loss_out, (const void*)grad})
        if (p && !aligned(p, 4)) return bad_arg(E, "every array must be 4-byte aligned");
    if (scratch && !aligned(scratch, 8)) return bad_arg(E, "scratch must be 8-byte aligned");
    if (!loss_out && !grad) return GSPLAT_OK;
    hipStream_t st = (hipStream_t)stream;
    // tv = sum over the axes of c[axis] sum d^2,  c[axis] = 1 / (V 12 pairs along the axis);  the gradient's factor is 2 scale c[axis]
    const double per = 1.0 / ((double)V * BILAGRID_CHANNELS);
    const double c[3] = {per / ((double)(L - 1) * Y * X), per / ((double)L * (Y - 1) * X), per / ((double)L * Y * (X - 1))};
    const int64_t blocks = tv_blocks(V, X, Y, L);
    double* partial = loss_out ? (double*)scratch : nullptr;
    hipLaunchKernelGGL(bilagrid_tv_kernel, dim3((unsigned)(V * BILAGRID_CHANNELS), (unsigned)tv_chunks(X, Y, L)), dim3(BILAGRID_THREADS), 0, st, grids, X, Y, L, (float)(2.0 * scale * c[0]),
                       (float)(2.0 * scale * c[1]), (float)(2.0 * scale * c[2]), c[0], c[1], c[2], (int)(flags & GSPLAT_BILAGRID_ACCUMULATE), grad,
                       partial);
    if (loss_out)
        hipLaunchKernelGGL(bilagrid_tv_finish_kernel, dim3(1), dim3(BILAGRID_THREADS), 0, st, (const double*)partial, blocks, (double)scale, loss_out);
    return launch_err("gsplat_bilagrid_tv launch");
}

}  // extern "C"
