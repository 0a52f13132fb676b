// The L2 metric of the flat index (VODHIP_L2): three small kernels around the unchanged inner-product scan.
//   ingest bias    |x~|^2 of every ingested row as stored -> the three bias terms in columns [dim, dim + 3) (l2_bias.h)
//   query staging  queries rounded to the store dtype + the three constants -> [nq, dim + 3], and |q~|^2 per query
//   finish         similarity-form results s = q~.x~ - |x~|^2 / 2 -> squared distances max(0, |q~|^2 - 2 s), pads +inf
// Both squared norms are float32 sums in ONE order that depends on `dim` alone: lane l of a wavefront adds the squares of the
// 8-element chunks l, l + 64, l + 128, ... of the row, in column order, then the 64 lane sums meet in a butterfly (xor 32, 16, ..,
// 1).  The square of a 16-bit value is exact in float32, so fused or separate multiply-add give the same bits.
// The host-only part (vodhip_debug_l2_split) also compiles as plain C++: tests/sanitize/l2_split_check.cpp.
#include "../../include/vodhip.h"
#include "l2_bias.h"

extern "C" int vodhip_debug_l2_split(float c, int dtype, uint16_t terms[3], float consts[3]) {
    if ((dtype != VODHIP_F16 && dtype != VODHIP_BF16) || !terms || !consts) return -1;
    uint16_t bits[3];
    vodhip::l2_query_consts(dtype, consts, bits);
    return vodhip::l2_split(c, dtype, terms);
}

#if defined(__HIP__)
#include "mips_common.h"

namespace vodhip {

namespace {

template <int DT>
__device__ __forceinline__ float l2_from_bits(uint16_t b) {
    if constexpr (DT == 0) return (float)__builtin_bit_cast(_Float16, b);
    else return __uint_as_float((unsigned int)b << 16);
}

// the 64 lane sums of a wavefront -> one value in every lane, fixed order
__device__ __forceinline__ float l2_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// One wavefront per stored row (4 per workgroup).  `rows` points at the first ingested row; columns >= dim of it are zero (the row
// conversion wrote them), and stride is a multiple of 64 elements, so every 16-byte chunk is aligned and inside the row.
template <int DT>
__global__ void __launch_bounds__(256) l2_bias_kernel(uint16_t* __restrict__ rows, int64_t n_rows, int dim, int64_t stride,
                                                      unsigned int* __restrict__ saturated) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (wave-uniform)
    uint16_t* x = rows + row * stride;
    float acc = 0.f;
    for (int c0 = lane * 8; c0 < dim; c0 += 64 * 8) {
        const uint4 w = *(const uint4*)(x + c0);
        const unsigned int u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = l2_from_bits<DT>((uint16_t)(u[e >> 1] >> ((e & 1) * 16)));
            if (c0 + e < dim) acc = fmaf(v, v, acc);
        }
    }
    const float n2 = l2_wave_sum(acc);
    if (lane == 0) {
        uint16_t t[3];
        if (l2_split(-0.5f * n2, DT, t)) atomicAdd(saturated, 1u);
        x[dim] = t[0];
        x[dim + 1] = t[1];
        x[dim + 2] = t[2];
    }
}

// One wavefront per query: [nq, dim] of q_dtype -> staged [nq, dim + 3] of the store dtype, and qn[nq] = |q~|^2 in the order of
// the ingest kernel (lane l takes the chunks l, l + 64, ...; columns of a chunk in order).
template <int DT>
__global__ void __launch_bounds__(256) l2_stage_queries_kernel(const void* __restrict__ q_src, int q_dtype, int64_t nq, int dim,
                                                               uint16_t* __restrict__ staged, float* __restrict__ qn) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq) return;
    uint16_t* out = staged + row * (int64_t)(dim + L2_BIAS_COLS);
    float acc = 0.f;
    for (int c0 = lane * 8; c0 < dim; c0 += 64 * 8) {
        for (int e = 0; e < 8 && c0 + e < dim; ++e) {
            const int64_t at = row * dim + c0 + e;
            float f;
            if (q_dtype == 2) f = ((const float*)q_src)[at];
            else if (q_dtype == 0) f = (float)(((const _Float16*)q_src)[at]);
            else f = (float)(((const __bf16*)q_src)[at]);
            float v;
            out[c0 + e] = store_bits(f, DT, &v);  // (saturating, as the scan rounds its queries: mips_common.h)
            acc = fmaf(v, v, acc);
        }
    }
    const float n2 = l2_wave_sum(acc);
    if (lane == 0) {
        float a[3];
        uint16_t bits[3];
        l2_query_consts(DT, a, bits);
        out[dim] = bits[0];
        out[dim + 1] = bits[1];
        out[dim + 2] = bits[2];
        qn[row] = n2;
    }
}

// sim [nq, k] (similarity form, pads -inf) -> dist [nq, k]: max(0, |q~|^2 - 2 s); a pad gets +inf
__global__ void __launch_bounds__(256) l2_finish_kernel(const float* __restrict__ sim, const float* __restrict__ qn, int64_t nq, int k, float* __restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * k) return;
    const float s = sim[i];
    float d = __builtin_inff();
    if (s != -__builtin_inff()) d = fmaxf(0.f, qn[i / k] - 2.f * s);
    dist[i] = d;
}

}  // namespace

hipError_t launch_l2_bias(void* rows, int store_dtype, int64_t n_rows, int64_t dim, int64_t stride, unsigned int* saturated,
                          hipStream_t stream) {
    if (n_rows == 0) return hipSuccess;
    if (dim + L2_BIAS_COLS > stride || stride % 64 != 0 || dim > (1ll << 30)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n_rows + 3) / 4);
    if (store_dtype == 0)
        hipLaunchKernelGGL(l2_bias_kernel<0>, dim3(blocks), dim3(256), 0, stream, (uint16_t*)rows, n_rows, (int)dim, stride, saturated);
    else
        hipLaunchKernelGGL(l2_bias_kernel<1>, dim3(blocks), dim3(256), 0, stream, (uint16_t*)rows, n_rows, (int)dim, stride, saturated);
    return hipGetLastError();
}

hipError_t launch_l2_stage_queries(const void* q_src, int q_dtype, int64_t nq, int64_t dim, int store_dtype, void* staged, float* qn,
                                   hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    if (dim > (1ll << 30)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((nq + 3) / 4);
    if (store_dtype == 0)
        hipLaunchKernelGGL(l2_stage_queries_kernel<0>, dim3(blocks), dim3(256), 0, stream, q_src, q_dtype, nq, (int)dim, (uint16_t*)staged, qn);
    else
        hipLaunchKernelGGL(l2_stage_queries_kernel<1>, dim3(blocks), dim3(256), 0, stream, q_src, q_dtype, nq, (int)dim, (uint16_t*)staged, qn);
    return hipGetLastError();
}

hipError_t launch_l2_finish(const float* sim, const float* qn, int64_t nq, int k, float* dist, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    const int64_t n = nq * k;
    hipLaunchKernelGGL(l2_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sim, qn, nq, k, dist);
    return hipGetLastError();
}

}  // namespace vodhip
#endif  // __HIP__
