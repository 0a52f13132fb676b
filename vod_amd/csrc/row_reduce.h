// Device helpers shared by the row-per-workgroup kernels (kernels_retrieval.hip, kernels_marginal.hip, kernels_pool.hip): encoding
// loads and stores, 16-byte pack / unpack, mask tests and the wave / 256-thread block reductions.
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

// an attention-mask element of `eb` bytes is live when any of its bits is set
__device__ __forceinline__ bool mask_live(const void* mask, int64_t i, int eb) {
    switch (eb) {
        case 1: return ((const uint8_t*)mask)[i] != 0;
        case 2: return ((const uint16_t*)mask)[i] != 0;
        case 4: return ((const uint32_t*)mask)[i] != 0;
        default: return ((const uint64_t*)mask)[i] != 0;
    }
}

template <int DT>
constexpr int elems_per_vec() { return DT == 2 ? 4 : 8; }

// 16 bytes of logits -> 4 (f32) or 8 (f16 / bf16) floats
template <int DT>
__device__ __forceinline__ void unpack16(const uint4& raw, float* v) {
    const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
    if constexpr (DT == 2) {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __builtin_bit_cast(float, w[u]);
    } else {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint16_t h = (uint16_t)(w[u >> 1] >> (16 * (u & 1)));
            if constexpr (DT == 0) v[u] = (float)__builtin_bit_cast(_Float16, h);
            else v[u] = __builtin_bit_cast(float, (unsigned)h << 16);
        }
    }
}

template <int DT>
__device__ __forceinline__ uint16_t to_bits16(float v) {
    if constexpr (DT == 0) return __builtin_bit_cast(uint16_t, (_Float16)v);
    else return __builtin_bit_cast(uint16_t, (__bf16)v);  // round to nearest even
}

template <int DT>
__device__ __forceinline__ uint4 pack16(const float* v) {
    unsigned w[4];
    if constexpr (DT == 2) {
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = __builtin_bit_cast(unsigned, v[u]);
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = (unsigned)to_bits16<DT>(v[2 * u]) | ((unsigned)to_bits16<DT>(v[2 * u + 1]) << 16);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int DT>
__device__ __forceinline__ void st_enc(void* p, int64_t i, float v) {
    if constexpr (DT == 2) ((float*)p)[i] = v;
    else if constexpr (DT == 0) ((_Float16*)p)[i] = (_Float16)v;
    else ((__bf16*)p)[i] = (__bf16)v;
}

}  // namespace vodhip
