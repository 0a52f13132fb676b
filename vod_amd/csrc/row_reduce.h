// Device helpers shared by the row-per-workgroup loss kernels (kernels_retrieval.hip, kernels_marginal.hip): encoding loads and
// the wave / 256-thread block reductions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vodhip {

template <int DT>
__device__ __forceinline__ float ld_enc(const void* p, int64_t i) {
    if constexpr (DT == 2) {
        return ((const float*)p)[i];
    } else if constexpr (DT == 0) {
        return (float)((const _Float16*)p)[i];
    } else {
        return (float)((const __bf16*)p)[i];
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// block-wide reductions through a 4-float LDS scratch (256 threads = 4 waves)
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ bool finite_f(float v) { return !(__builtin_isinf(v) || v != v); }

}  // namespace vodhip
