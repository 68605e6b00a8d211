// gs_exposure.h -- per-view exposure compensation (not in the reference): an affine colour transform per training image,
// applied to the rendered frame before the loss, with the gradients of the frame and of the twelve parameters.
//
//   E = [M | t], twelve floats, row-major 3 x 4.  For every pixel colour c:
//     o_r      = fma(M_r0, c_0, fma(M_r1, c_1, fma(M_r2, c_2, t_r)))                      (no clamp)
//     g_c[k]   = fma(M_0k, g_o[0], fma(M_1k, g_o[1], M_2k g_o[2]))
//     g_E[r,k] = sum over the pixels of g_o[r] c_k  (k < 3),   g_E[r,3] = sum over the pixels of g_o[r]
//   With that nesting the identity (M = I, t = 0) returns every finite c and every finite g_o bit for bit: the terms with a zero
//   coefficient are +-0, and x + (+-0) = x  (a c of -0 comes back as +0: the same number).
//
// The per-pixel arithmetic is `GS_HD`: the kernels below inline it and g++ compiles it into a host test library
// (csrc/host_exposure_check.cpp).  The host build is a TEST of this file, never a fallback.
//
// Streaming kernels in the shape of gs_aux_loss.h, over the flat pixel index of ONE image (grid.y = the image: the twelve parameters
// are per image, so a workgroup never straddles two): thread i of an image owns pixels 4 i .. 4 i + 3 -- three 16-byte accesses per
// array where every array is 16-byte aligned, every image starts on such a boundary and the four pixels exist, element by element
// otherwise (an unaligned pointer, the ragged end).  Either way a thread handles its four pixels in index order, so the alignment of
// a buffer changes no bit of the result.
//   exposure_forward_kernel    out = E c
//   exposure_backward_kernel   g_image (if asked for), and the workgroup's twelve sums -> partial[image][block][12] (if asked for)
//   exposure_finish_kernel     ONE workgroup per image adds that image's partial rows in a fixed order, in double, and stores the
//                              twelve floats to (or adds them to) the destination row
//
// The order of the sums (no float atomics anywhere): a thread adds its four pixels in index order (the first fma rounds the product
// alone, the other three add: 3 additions); the wave adds its 64 lanes through the __shfl_xor ladder (6 additions); lanes 0..11 of
// wave 0, one sum each, add the four waves' sums from LDS in wave order (3 additions) -- EXPOSURE_SUM_DEPTH = 12 fp32 additions above
// a rounded product.
// The partial rows are added in double and rounded to fp32 once.  Nothing in that order depends on which workgroup ran first, on
// the stream or on the launch: the gradient is the same bits every time.
#pragma once
#include "gs_math.h"
#if defined(__HIPCC__)
#include "gs_blocksum.h"
#endif

namespace gsexp {

constexpr int EXPOSURE_THREADS = 256;
constexpr int EXPOSURE_PIX = 4;                                              // pixels per thread
constexpr int EXPOSURE_BLOCK_PIX = EXPOSURE_THREADS * EXPOSURE_PIX;          // 1024 pixels per workgroup, 256 per wave
constexpr int EXPOSURE_SUM_DEPTH = 12;                                       // fp32 additions between a product and its workgroup's sum
constexpr int EXPOSURE_PARAMS = 12;

// o = E c
GS_HD void apply_pixel(const float* E, const float* c, float* o) {
    for (int r = 0; r < 3; ++r)
        o[r] = __builtin_fmaf(E[r * 4], c[0], __builtin_fmaf(E[r * 4 + 1], c[1], __builtin_fmaf(E[r * 4 + 2], c[2], E[r * 4 + 3])));
}

// g_c = M^T g_o
GS_HD void backward_pixel(const float* E, const float* go, float* gc) {
    for (int k = 0; k < 3; ++k) gc[k] = __builtin_fmaf(E[k], go[0], __builtin_fmaf(E[4 + k], go[1], E[8 + k] * go[2]));
}

// s[r][k] += g_o[r] c_k, s[r][3] += g_o[r]: one pixel joins a thread's twelve sums
GS_HD void accumulate_pixel(const float* c, const float* go, float* s) {
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) s[r * 4 + k] = __builtin_fmaf(go[r], c[k], s[r * 4 + k]);
        s[r * 4 + 3] += go[r];
    }
}

#if defined(__HIPCC__)

typedef float exp_f4 __attribute__((ext_vector_type(4)));

// the twelve colour floats of four consecutive pixels from pixel `i` of an image of n pixels (absent pixels: 0)
__device__ __forceinline__ void load_pixels(const float* __restrict__ p, int64_t i, int64_t n, bool vec, float (&v)[3 * EXPOSURE_PIX]) {
    if (vec && i + EXPOSURE_PIX <= n) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const exp_f4 t = *reinterpret_cast<const exp_f4*>(p + i * 3 + q * 4);
            v[q * 4] = t.x; v[q * 4 + 1] = t.y; v[q * 4 + 2] = t.z; v[q * 4 + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3 * EXPOSURE_PIX; ++k) v[k] = i + k / 3 < n ? p[i * 3 + k] : 0.f;
    }
}

__device__ __forceinline__ void store_pixels(float* __restrict__ p, int64_t i, int64_t n, bool vec, const float (&v)[3 * EXPOSURE_PIX]) {
    if (vec && i + EXPOSURE_PIX <= n) {
#pragma unroll
        for (int q = 0; q < 3; ++q) *reinterpret_cast<exp_f4*>(p + i * 3 + q * 4) = exp_f4{v[q * 4], v[q * 4 + 1], v[q * 4 + 2], v[q * 4 + 3]};
    } else {
#pragma unroll
        for (int k = 0; k < 3 * EXPOSURE_PIX; ++k)
            if (i + k / 3 < n) p[i * 3 + k] = v[k];
    }
}

// n: pixels of ONE image; grid = (workgroups per image, images)
__global__ __launch_bounds__(EXPOSURE_THREADS) void exposure_forward_kernel(const float* __restrict__ image, const float* __restrict__ params,
                                                                            int64_t n, int vec, float* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * EXPOSURE_THREADS + threadIdx.x) * EXPOSURE_PIX;
    if (i >= n) return;
    const int64_t base = (int64_t)blockIdx.y * n * 3;
    float E[EXPOSURE_PARAMS], c[3 * EXPOSURE_PIX], o[3 * EXPOSURE_PIX];
#pragma unroll
    for (int k = 0; k < EXPOSURE_PARAMS; ++k) E[k] = params[(int64_t)blockIdx.y * EXPOSURE_PARAMS + k];       // (wave-uniform: scalar loads)
    load_pixels(image + base, i, n, vec, c);
#pragma unroll
    for (int k = 0; k < EXPOSURE_PIX; ++k) apply_pixel(E, c + 3 * k, o + 3 * k);
    store_pixels(out + base, i, n, vec, o);
}

// IMG: write g_image; PAR: write the workgroup's twelve sums to partial[(image * gridDim.x + block) * 12]
template <bool IMG, bool PAR>
__global__ __launch_bounds__(EXPOSURE_THREADS) void exposure_backward_kernel(const float* __restrict__ image, const float* __restrict__ params,
                                                                             const float* __restrict__ g_out, int64_t n, int vec,
                                                                             float* __restrict__ g_image, float* __restrict__ partial) {
    __shared__ float red[EXPOSURE_THREADS / 64][EXPOSURE_PARAMS];
    const int tid = threadIdx.x;
    const int64_t i = ((int64_t)blockIdx.x * EXPOSURE_THREADS + tid) * EXPOSURE_PIX;
    const int64_t base = (int64_t)blockIdx.y * n * 3;
    float s[EXPOSURE_PARAMS];
#pragma unroll
    for (int k = 0; k < EXPOSURE_PARAMS; ++k) s[k] = 0.f;
    if (i < n) {
        float go[3 * EXPOSURE_PIX];
        load_pixels(g_out + base, i, n, vec, go);                   // (past the end: 0, which adds nothing)
        if (IMG) {
            float E[EXPOSURE_PARAMS], gc[3 * EXPOSURE_PIX];
#pragma unroll
            for (int k = 0; k < EXPOSURE_PARAMS; ++k) E[k] = params[(int64_t)blockIdx.y * EXPOSURE_PARAMS + k];
#pragma unroll
            for (int k = 0; k < EXPOSURE_PIX; ++k) backward_pixel(E, go + 3 * k, gc + 3 * k);
            store_pixels(g_image + base, i, n, vec, gc);
        }
        if (PAR) {
            float c[3 * EXPOSURE_PIX];
            load_pixels(image + base, i, n, vec, c);
#pragma unroll
            for (int k = 0; k < EXPOSURE_PIX; ++k)
                if (i + k < n) accumulate_pixel(c + 3 * k, go + 3 * k, s);
        }
    }
    if (!PAR) return;
    // the workgroup's twelve sums, in a fixed order
    gsblk::sum(s, red);
    if (tid < EXPOSURE_PARAMS)
        partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * EXPOSURE_PARAMS + tid] = gsblk::column<EXPOSURE_THREADS / 64>(red, tid);
}

// One workgroup per image.  row_index (device, int32, may be NULL): image b goes to row row_index[b] of dest, else to row b; a negative
// index drops the row.  add: dest += the twelve floats, else dest = them.
__global__ __launch_bounds__(EXPOSURE_THREADS) void exposure_finish_kernel(const float* __restrict__ partial, int n_blocks,
                                                                           const int32_t* __restrict__ row_index, int add, float* __restrict__ dest) {
    __shared__ double red[EXPOSURE_THREADS / 64][EXPOSURE_PARAMS];
    const int tid = threadIdx.x;
    const float* rows = partial + (int64_t)blockIdx.x * n_blocks * EXPOSURE_PARAMS;
    double s[EXPOSURE_PARAMS];
#pragma unroll
    for (int k = 0; k < EXPOSURE_PARAMS; ++k) s[k] = 0.0;
    for (int b = tid; b < n_blocks; b += EXPOSURE_THREADS) {
#pragma unroll
        for (int k = 0; k < EXPOSURE_PARAMS; ++k) s[k] += (double)rows[(int64_t)b * EXPOSURE_PARAMS + k];
    }
    // (copy: gsblk::sum and gsblk::column of gs_blocksum.h, spelled out -- through the helpers this kernel, alone among their users,
    //  comes out one VGPR and three s_waitcnt larger; the order of the additions is the same)
#pragma unroll
    for (int k = 0; k < EXPOSURE_PARAMS; ++k)
        for (int sft = 32; sft > 0; sft >>= 1) s[k] += __shfl_xor(s[k], sft);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < EXPOSURE_PARAMS; ++k) red[tid >> 6][k] = s[k];
    }
    __syncthreads();
    if (tid < EXPOSURE_PARAMS) {
        double x = red[0][tid];
        for (int w = 1; w < EXPOSURE_THREADS / 64; ++w) x += red[w][tid];
        const int64_t row = row_index ? (int64_t)row_index[blockIdx.x] : (int64_t)blockIdx.x;
        if (row >= 0) {
            float* d = dest + row * EXPOSURE_PARAMS + tid;
            *d = add ? *d + (float)x : (float)x;
        }
    }
}

#endif  // __HIPCC__

}  // namespace gsexp
