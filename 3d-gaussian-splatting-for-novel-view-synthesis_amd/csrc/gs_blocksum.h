// gs_blocksum.h -- the fixed-order sum of one value per lane over a workgroup.  Device code only; needs nothing but HIP.
//
// Every loss, metric and gradient sum of the small units is formed the same way, and the ORDER of its additions is what makes it the
// same bits on every call, stream and rank:
//   ladder   a wave adds its 64 lanes through __shfl_xor 32, 16, 8, 4, 2, 1 (6 additions; every lane ends with the wave's sum).
//            NOT gs_wave.h's wave_sum / wave_sum_f: those go through DPP and add in another order -- other bits.
//   stage    lane 0 of each wave leaves its wave's K sums in red[wave][0..K)
//   column   after a __syncthreads(): x = red[0][k]; x += red[1][k]; ... in wave order (WAVES - 1 additions).  No leading "0 +": a sum
//            that is -0.0 in every wave (an fma that underflowed from below) stays -0.0.
// sum() is ladder, stage and the __syncthreads(); a kernel that sums two types at once (doubles and an integer count) calls the
// ladders, then the stages, then ONE barrier of its own.  Who calls column -- thread k for column k, or thread 0 for all of them -- is the
// caller's choice and changes no bit.
#pragma once
#include <hip/hip_runtime.h>

namespace gsblk {

template <typename T>
__device__ __forceinline__ T ladder(T v) {
    for (int sft = 32; sft > 0; sft >>= 1) v += __shfl_xor(v, sft);
    return v;
}

template <typename T, int K>
__device__ __forceinline__ void stage(const T (&v)[K], T (*red)[K]) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
}

template <int WAVES, typename T, int K>
__device__ __forceinline__ T column(const T (*red)[K], int k) {
    T x = red[0][k];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) x += red[w][k];
    return x;
}

template <typename T, int K>
__device__ __forceinline__ void sum(const T (&v)[K], T (*red)[K]) {
    T w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) w[k] = ladder(v[k]);
    stage(w, red);
    __syncthreads();
}

// one value per lane: red is T[WAVES]
template <typename T>
__device__ __forceinline__ void stage(T v, T* red) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
}
template <int WAVES, typename T>
__device__ __forceinline__ T column(const T* red) {
    T x = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) x += red[w];
    return x;
}
template <typename T>
__device__ __forceinline__ void sum(T v, T* red) {
    stage(ladder(v), red);
    __syncthreads();
}

}  // namespace gsblk
