// In-place update of stored rows (include/vodhip.h H2u): SET  x[row] = src  or ADD  x[row] = x[row] + alpha * src, for listed rows
// (row = ids[j] - id_base) or a contiguous range (row = row_begin + j), with every plane the store keeps written in the same launch.
// The result is the bytes `add` writes for the same final rows: each piece below restates the ingest kernel it stands in for -
//   16-bit plane   convert_rows_kernel (kernels_mips.hip): store_bits of every value, columns >= dim zero;
//   L2 store       l2_bias_kernel (kernels_l2.hip): |x~|^2 of the values as stored, lane l adds the squares of the chunks l, l + 64, ..
//                  in column order, the xor 32 .. 1 butterfly, l2_split -> columns [dim, dim + 3); a saturated split is counted;
//   exact store    ingest_exact_kernel (kernels_exact.hip): the float32 plane with its zero pad columns, row_n2 / row_d2 from the
//                  same fma chains and wave_sum_fixed, atomicMax on the two maxima words under the same conditions.
// Geometry as there: one wavefront per slot, four slots per 256-thread workgroup, a lane owns the 8-element chunks lane, lane + 64, ..
// of the row; 16-byte loads and stores (32 bytes of float32), element by element when dim % 8 != 0 or the source is misaligned.
//
// ADD in float32, two roundings: p = alpha * src, t = old + p (compiled with contraction off: never fused into an fma), `old` the float32
// plane of an exact store and the 16-bit row widened anywhere else.
//
// An L2 row's bias columns share a 16-byte chunk with its last data columns (dim = 509: columns 504 .. 511).  The bias is known only
// after the whole row was summed, and a lane cannot keep an unbounded number of chunks in registers: the one or two chunks that
// overlap [dim, dim + 3) are left out of the first pass (their values are summed, not stored), and their owning lanes form them again
// behind the butterfly - the same loads (an ADD's `old` is still there: the chunk was not stored), the same arithmetic - and store
// them with the bias in place.  Every byte of the row is stored exactly once.
//
// LISTED form, duplicates: the last slot that lists a row writes it, as NumPy's x[ids] = rows.  The claim launch (one thread per slot)
// does atomicMax(&owner[row], slot + 1) on an int32 word per capacity row; in the write launch the slot whose number the word holds
// writes the row and puts the word back to 0, every other slot of that row counts itself a duplicate and leaves.  No sort, no race
// (a loser reads the winner's number or the 0 behind it: neither is its own), the same bytes on every repeat, the table all zero
// after every call.  A slot whose id is negative or outside [id_base, id_base + ntotal) counts itself skipped (the pad rule of
// vodhip_index_score_ids).  Only those two rare events cost an atomic: the rows written are n - skipped - duplicates.
#include <algorithm>

#include "exact_dot.h"
#include "l2_bias.h"
#include "mips_common.h"

namespace vodhip {

namespace {

template <int DT>
__device__ __forceinline__ float upd_from_bits(uint16_t b) {
    if constexpr (DT == 0) return (float)__builtin_bit_cast(_Float16, b);
    else return (float)__builtin_bit_cast(__bf16, b);
}

// l2_split (l2_bias.h) with its three steps written out: the rolled loop there indexes `terms` and the constants by the loop counter,
// which puts them in scratch (8 bytes per lane in l2_bias_kernel).  The same operations in the same order, hence the same bits.
template <int DT>
__device__ __forceinline__ int update_l2_split(float c, uint16_t& t0, uint16_t& t1, uint16_t& t2) {
    float a[3];
    uint16_t abits[3];
    l2_query_consts(DT, a, abits);
    const float lim = l2_split_limit(DT);
    float t;
    if (!(c >= -lim && c <= lim)) {  // (also NaN)
        t0 = l2_round_term(-lim / a[0], DT, &t);
        t1 = t2 = 0;
        return 1;
    }
    float r = c;
    t0 = l2_round_term(r / a[0], DT, &t);
    r -= a[0] * t;
    t1 = l2_round_term(r / a[1], DT, &t);
    r -= a[1] * t;
    t2 = l2_round_term(r / a[2], DT, &t);
    return 0;
}

// the new float32 values t[0 .. 8) of columns c0 .. c0 + 7 of `row`; columns >= dim are +0
template <int SRC, int DST, int MODE, int KIND>
__device__ __forceinline__ void update_chunk(const UpdateArgs& a, int64_t src_row, int64_t row, int64_t c0, bool vec, float (&t)[8]) {
    float in[8];
    if (vec && c0 < a.dim) {
        if constexpr (SRC == 2) {
            const float4 lo = *reinterpret_cast<const float4*>((const float*)a.src + src_row * a.dim + c0);
            const float4 hi = *reinterpret_cast<const float4*>((const float*)a.src + src_row * a.dim + c0 + 4);
            in[0] = lo.x, in[1] = lo.y, in[2] = lo.z, in[3] = lo.w, in[4] = hi.x, in[5] = hi.y, in[6] = hi.z, in[7] = hi.w;
        } else {
            const uint4 raw = *reinterpret_cast<const uint4*>((const uint16_t*)a.src + src_row * a.dim + c0);
            const unsigned int u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) in[e] = upd_from_bits<SRC>((uint16_t)(u[e >> 1] >> ((e & 1) * 16)));
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t c = c0 + e;
            float v = 0.f;
            if (c < a.dim) {
                if constexpr (SRC == 2) v = ((const float*)a.src)[src_row * a.dim + c];
                else v = upd_from_bits<SRC>(((const uint16_t*)a.src)[src_row * a.dim + c]);
            }
            in[e] = v;
        }
    }
    if constexpr (MODE == 1) {
        float old[8];
        if constexpr (KIND == UPDATE_EXACT) {
            const float4 lo = *reinterpret_cast<const float4*>(a.data32 + row * a.stride + c0);
            const float4 hi = *reinterpret_cast<const float4*>(a.data32 + row * a.stride + c0 + 4);
            old[0] = lo.x, old[1] = lo.y, old[2] = lo.z, old[3] = lo.w, old[4] = hi.x, old[5] = hi.y, old[6] = hi.z, old[7] = hi.w;
        } else {
            const uint4 raw = *reinterpret_cast<const uint4*>(a.data + row * a.stride + c0);
            const unsigned int u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) old[e] = upd_from_bits<DST>((uint16_t)(u[e >> 1] >> ((e & 1) * 16)));
        }
        // (written as * and + under contract(off): __fmul_rn / __fadd_rn are inline * and + that carry the default contraction mode of
        // their header with them, and the compiler fused them into one v_pk_fma_f32)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma clang fp contract(off)
            const float p = a.alpha * in[e];
            t[e] = c0 + e < a.dim ? old[e] + p : 0.f;  // (an L2 row's bias is no `old`)
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = in[e];
    }
}

template <int SRC, int DST, int MODE, int KIND>
__global__ __launch_bounds__(256) void update_rows_kernel(const UpdateArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t local = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (local >= a.n_slots) return;  // (wave-uniform, as every branch before the row loop)
    const int64_t j = a.slot_begin + local;
    int64_t row = a.row_begin + j;
    if (a.ids != nullptr) {
        const int64_t id = a.ids[j];
        row = id - a.id_base;
        if (id < 0 || row < 0 || row >= a.ntotal) {
            if (lane == 0) atomicAdd(a.counts + 0, 1u);
            return;
        }
        if (a.owner[row] != (int)(j + 1)) {  // a later slot lists the row too: that one writes it
            if (lane == 0) atomicAdd(a.counts + 1, 1u);
            return;
        }
    }
    const bool vec = (a.dim & 7) == 0 && ((uintptr_t)a.src & (SRC == 2 ? 31 : 15)) == 0;
    // L2: the chunks that hold a bias column (one, or two when [dim, dim + 3) straddles a chunk edge); dim + 3 <= stride
    const int64_t bias_a = a.dim & ~(int64_t)7, bias_b = (a.dim + L2_BIAS_COLS - 1) & ~(int64_t)7;
    float n2 = 0.f, d2 = 0.f;
    for (int64_t c0 = (int64_t)lane * 8; c0 < a.stride; c0 += 512) {
        float t[8];
        uint16_t h[8];
        update_chunk<SRC, DST, MODE, KIND>(a, local, row, c0, vec, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float r;
            h[e] = store_bits(t[e], DST, &r);  // (finite values beyond the store dtype's range saturate: mips_common.h)
            if constexpr (KIND == UPDATE_EXACT) {
                n2 = __builtin_fmaf(t[e], t[e], n2);
                d2 = __builtin_fmaf(t[e] - r, t[e] - r, d2);
            }
            if constexpr (KIND == UPDATE_L2) {
                if (c0 + e < a.dim) n2 = fmaf(r, r, n2);
            }
        }
        if (KIND != UPDATE_L2 || (c0 != bias_a && c0 != bias_b)) *reinterpret_cast<uint4*>(a.data + row * a.stride + c0) = *reinterpret_cast<const uint4*>(h);
        if constexpr (KIND == UPDATE_EXACT) {
            *reinterpret_cast<float4*>(a.data32 + row * a.stride + c0) = make_float4(t[0], t[1], t[2], t[3]);
            *reinterpret_cast<float4*>(a.data32 + row * a.stride + c0 + 4) = make_float4(t[4], t[5], t[6], t[7]);
        }
    }
    if constexpr (KIND == UPDATE_L2) {
        n2 = wave_sum_fixed(n2);  // (l2_wave_sum of kernels_l2.hip: the same butterfly)
        uint16_t b0, b1, b2;
        const int saturated = update_l2_split<DST>(-0.5f * n2, b0, b1, b2);
        if (lane == 0 && saturated) atomicAdd(a.l2_sat, 1u);
#pragma unroll 1
        for (int64_t c0 = bias_a; c0 <= bias_b; c0 += 8) {
            if ((int)((c0 >> 3) & 63) != lane) continue;
            float t[8];
            uint16_t h[8];
            update_chunk<SRC, DST, MODE, KIND>(a, local, row, c0, vec, t);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float r;
                h[e] = store_bits(t[e], DST, &r);
                const int64_t c = c0 + e;
                if (c >= a.dim && c < a.dim + L2_BIAS_COLS) h[e] = c == a.dim ? b0 : (c == a.dim + 1 ? b1 : b2);
            }
            *reinterpret_cast<uint4*>(a.data + row * a.stride + c0) = *reinterpret_cast<const uint4*>(h);
        }
    }
    if constexpr (KIND == UPDATE_EXACT) {
        n2 = wave_sum_fixed(n2);
        d2 = wave_sum_fixed(d2);
        if (lane == 0) {
            a.row_n2[row] = n2;
            a.row_d2[row] = d2;
        }
        if (lane == 0 && n2 < __builtin_inff()) {  // (false for NaN too)
            if (__float_as_uint(n2) > __hip_atomic_load(a.norm_stats + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a.norm_stats + 0, __float_as_uint(n2));
            if (d2 < __builtin_inff() && __float_as_uint(d2) > __hip_atomic_load(a.norm_stats + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(a.norm_stats + 1, __float_as_uint(d2));
        }
    }
    if (a.ids != nullptr && lane == 0) a.owner[row] = 0;  // the table is all zero again when the call's last launch ends
}

__global__ __launch_bounds__(256) void update_claim_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t id_base, int64_t ntotal,
                                                           int* __restrict__ owner) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t id = ids[j], row = id - id_base;
    if (id < 0 || row < 0 || row >= ntotal) return;
    atomicMax(owner + row, (int)(j + 1));
}

// the maxima of the finite per-row statistics of the rows now stored (ingest_exact_kernel's conditions: a row with a non-finite
// |x|^2 moves neither maximum)
__global__ __launch_bounds__(256) void update_maxima_kernel(const float* __restrict__ row_n2, const float* __restrict__ row_d2, int64_t n,
                                                            unsigned int* __restrict__ st) {
    float mn = 0.f, md = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x = row_n2[i], y = row_d2[i];
        if (!(x < __builtin_inff())) continue;
        mn = fmaxf(mn, x);
        if (y < __builtin_inff()) md = fmaxf(md, y);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mn = fmaxf(mn, __shfl_xor(mn, m, 64));
        md = fmaxf(md, __shfl_xor(md, m, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (__float_as_uint(mn) > __hip_atomic_load(st + EXS_MAX_N2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st + EXS_MAX_N2, __float_as_uint(mn));
        if (__float_as_uint(md) > __hip_atomic_load(st + EXS_MAX_D2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(st + EXS_MAX_D2, __float_as_uint(md));
    }
}

template <int SRC, int DST, int MODE>
hipError_t launch_update_kind(const UpdateArgs& a, unsigned blocks, hipStream_t stream) {
    if (a.kind == UPDATE_PLAIN) hipLaunchKernelGGL((update_rows_kernel<SRC, DST, MODE, UPDATE_PLAIN>), dim3(blocks), dim3(256), 0, stream, a);
    else if (a.kind == UPDATE_L2) hipLaunchKernelGGL((update_rows_kernel<SRC, DST, MODE, UPDATE_L2>), dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((update_rows_kernel<SRC, DST, MODE, UPDATE_EXACT>), dim3(blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_update_claim(const int64_t* ids, int64_t n, int64_t id_base, int64_t ntotal, int* owner, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!ids || !owner || n >= (1ll << 31) - 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(update_claim_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ids, n, id_base, ntotal, owner);
    return hipGetLastError();
}

hipError_t launch_update_rows(const UpdateArgs& a, hipStream_t stream) {
    if (a.n_slots == 0) return hipSuccess;
    if (!a.src || !a.data || a.dim <= 0 || a.stride % 64 != 0 || a.dim + (a.kind == UPDATE_L2 ? L2_BIAS_COLS : 0) > a.stride) return hipErrorInvalidValue;
    if (a.kind < UPDATE_PLAIN || a.kind > UPDATE_EXACT || (a.mode != 0 && a.mode != 1)) return hipErrorInvalidValue;
    if (a.kind == UPDATE_EXACT && (!a.data32 || !a.row_n2 || !a.row_d2 || !a.norm_stats)) return hipErrorInvalidValue;
    if (a.kind == UPDATE_L2 && !a.l2_sat) return hipErrorInvalidValue;
    if (a.ids ? (!a.owner || !a.counts) : (a.row_begin + a.slot_begin < 0 || a.row_begin + a.slot_begin + a.n_slots > a.ntotal)) return hipErrorInvalidValue;
    if (a.n_slots > 4ll * 0x7fffffff) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.n_slots + 3) / 4);
#define VOD_UPD(S, D)                                                                          \
    if (a.src_dtype == S && a.store_dtype == D)                                                \
        return a.mode == 0 ? launch_update_kind<S, D, 0>(a, blocks, stream) : launch_update_kind<S, D, 1>(a, blocks, stream);
    VOD_UPD(0, 0) VOD_UPD(1, 0) VOD_UPD(2, 0) VOD_UPD(0, 1) VOD_UPD(1, 1) VOD_UPD(2, 1)
#undef VOD_UPD
    return hipErrorInvalidValue;
}

hipError_t launch_update_maxima(const float* row_n2, const float* row_d2, int64_t n_rows, unsigned int* stats, hipStream_t stream) {
    if (hipError_t e = hipMemsetAsync(stats + EXS_MAX_N2, 0, 2 * sizeof(unsigned int), stream); e != hipSuccess) return e;
    if (n_rows <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<int64_t>(1024, (n_rows + 255) / 256);
    hipLaunchKernelGGL(update_maxima_kernel, dim3(blocks), dim3(256), 0, stream, row_n2, row_d2, n_rows, stats);
    return hipGetLastError();
}

}  // namespace vodhip
