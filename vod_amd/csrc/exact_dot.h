// The score function of VODHIP_EXACT_F32 stores, shared by every kernel that scores a (query, float32 row) pair: the re-scoring of a
// search (kernels_exact.hip) and the listed-row scoring (kernels_listed.hip).  include/vodhip.h promises "the same bits from every
// path": the arithmetic below is that promise - one fma order per component, one order of the partial sums.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vodhip {

// every lane ends with the same value: the pairs of a butterfly step add the same two numbers, and the step order is fixed
__device__ __forceinline__ float wave_sum_fixed(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// THE score function of exact mode: lane l accumulates columns 4l .. 4l+3 (mod 256) in increasing column order with one fma chain
// per component, the four chains are added as (0 + 1) + (2 + 3), the 64 lane sums by the butterfly above.  Zero padded columns add
// exact zeros, so the value depends on the row and the query alone.  NC rows at once: their loads are in flight together.
template <int NC>
__device__ __forceinline__ void exact_dot(const float* __restrict__ plane, int64_t stride, const int (&rows)[NC], const float* qs,
                                          int dim_pad, int lane, float (&out)[NC]) {
    float acc[NC][4];
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n][0] = acc[n][1] = acc[n][2] = acc[n][3] = 0.f;
    for (int c = lane * 4; c < dim_pad; c += 256) {
        const float4 qv = *reinterpret_cast<const float4*>(qs + c);
        float4 xv[NC];
#pragma unroll
        for (int n = 0; n < NC; ++n)
            xv[n] = rows[n] >= 0 ? *reinterpret_cast<const float4*>(plane + (size_t)rows[n] * stride + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int n = 0; n < NC; ++n) {
            acc[n][0] = __builtin_fmaf(xv[n].x, qv.x, acc[n][0]);
            acc[n][1] = __builtin_fmaf(xv[n].y, qv.y, acc[n][1]);
            acc[n][2] = __builtin_fmaf(xv[n].z, qv.z, acc[n][2]);
            acc[n][3] = __builtin_fmaf(xv[n].w, qv.w, acc[n][3]);
        }
    }
#pragma unroll
    for (int n = 0; n < NC; ++n) out[n] = wave_sum_fixed((acc[n][0] + acc[n][1]) + (acc[n][2] + acc[n][3]));
}

// the same function with every load of the NC rows issued before the first fma (dim_pad <= 256 * NI): one memory latency per group of
// rows instead of one per 256 columns.  Same fma order per component -> the same bits as exact_dot.
template <int NC, int NI>
__device__ __forceinline__ void exact_dot_preload(const float* __restrict__ plane, int64_t stride, const int (&rows)[NC], const float* qs,
                                                  int dim_pad, int lane, float (&out)[NC]) {
    float4 xv[NI][NC];
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int c = lane * 4 + it * 256;
#pragma unroll
        for (int n = 0; n < NC; ++n)
            xv[it][n] = (c < dim_pad && rows[n] >= 0) ? *reinterpret_cast<const float4*>(plane + (size_t)rows[n] * stride + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float acc[NC][4];
#pragma unroll
    for (int n = 0; n < NC; ++n) acc[n][0] = acc[n][1] = acc[n][2] = acc[n][3] = 0.f;
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int c = lane * 4 + it * 256;
        if (c < dim_pad) {
            const float4 qv = *reinterpret_cast<const float4*>(qs + c);
#pragma unroll
            for (int n = 0; n < NC; ++n) {
                acc[n][0] = __builtin_fmaf(xv[it][n].x, qv.x, acc[n][0]);
                acc[n][1] = __builtin_fmaf(xv[it][n].y, qv.y, acc[n][1]);
                acc[n][2] = __builtin_fmaf(xv[it][n].z, qv.z, acc[n][2]);
                acc[n][3] = __builtin_fmaf(xv[it][n].w, qv.w, acc[n][3]);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NC; ++n) out[n] = wave_sum_fixed((acc[n][0] + acc[n][1]) + (acc[n][2] + acc[n][3]));
}

}  // namespace vodhip
