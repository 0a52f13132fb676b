// What the whole-store scans with a second MFMA product share: posterior_mean (kernels_posterior.hip), posterior_expectation
// (kernels_readout.hip), its gradient in the query (kernels_readout_grad.hip), its adjoint in the value table (kernels_readout_adjoint.hip)
// and key_gradient (kernels_key_grad.hip).  Each of them scores a tile with scan_k_loop (store_scan.h) on 256 streamed rows x 64 resident
// columns, turns the scores into 16-bit weights and contracts the weights with 64-column slices of a second operand on the MFMA.
//
// SHARED HERE: the slice-image geometry, the fp16 weight scale, the vector typedefs of the transposed reads, acc_scale, and the whole host side: the dispatch over (store dtype, subset), over the
// slices of a launch and over full chunks + remainder, and the argument checks.
// NOT SHARED, on purpose: the second product itself (slice staging, weight packing, transposed reads, register-class pins, wave sum) is
// spelled out in each kernel.  A build with those pieces as __forceinline__ helpers gave the same bytes and the same resources, but hipcc
// allocates and schedules every one of these 1-wave-per-SIMD kernels anew when ANY helper replaces its local text - even the index
// decode of the store loop alone - and the result measured 0.1 - 1.4 % slower than the local code in four of the five operations (7 - 8 %
// for posterior_mean on the two-offset staging): profiles/scan_contract_refactor.md.  What is here leaves every kernel's device code
// unchanged, instruction for instruction.
//   image     a slice = 64 columns of the 256 streamed rows, in the K loop's LDS image: 128-byte rows, 16-byte slot s of row r holds
//             chunk s ^ ((r >> 1) & 7).  Up to 4 slices lie side by side from the start of the dynamic LDS, over the K loop's ring.
//   weights   fp16 weights are multiplied by 2^15 before the rounding, so that they are NORMAL fp16 numbers down to 2^-29 of the
//             largest (<= 1 -> 32768 < 65504); the sum is multiplied by 2^-15 in float32, both exact.  bf16 needs no scale.
#pragma once
#include "store_scan.h"

namespace vodhip {

constexpr int CT_BN = 64;                           // resident columns of a workgroup (queries, or stored rows with the operands exchanged)
constexpr int CT_SLICE_BYTES = SCAN_BM * 128;       // one slice image
constexpr int CT_MAX_SLICES = 4;
constexpr int CT_IMG = CT_MAX_SLICES * CT_SLICE_BYTES;  // the slices of the second product: the start of every kernel's dynamic LDS
static_assert(SCAN_BK == 64, "a slice row is one 128-byte LDS row of the K loop");
static_assert(CT_IMG >= scan_ring_bytes(CT_BN), "the ring fits under the slices");

// the fp16 weight scale 2^15 and its inverse (DT 0 = fp16, 1 = bf16: no scale)
constexpr int CT_FP16_SHIFT = 15;
constexpr float CT_FP16_SCALE = 32768.f;
static_assert(CT_FP16_SCALE == (float)(1 << CT_FP16_SHIFT), "one scale");

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// acc * f for an MFMA accumulator block that stays in the accumulation registers (AGPRs): the block is copied into 16 vector registers,
// multiplied there and copied back, one block at a time.  Written as a plain product the compiler keeps every block in the vector
// registers the K loop needs (measured: 1.1 KB of scratch per lane at NSL = 4); the empty asm statements pin the register class.
__device__ __forceinline__ void acc_scale(f32x16& acc, float f) {
    f32x16 a = acc;
    asm volatile("" : "+a"(a));
    f32x16 v = a;
    asm volatile("" : "+v"(v));
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] *= f;
    asm volatile("" : "+v"(v));
    a = v;
    asm volatile("" : "+a"(a));
    acc = a;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
// f(dt, subset) with the two compile-time tags of the instantiation
template <class F>
hipError_t contract_dispatch(int store_dtype, bool subset, F&& f) {
    auto with_subset = [&](auto dt) { return subset ? f(dt, std::true_type{}) : f(dt, std::false_type{}); };
    return store_dtype == 0 ? with_subset(std::integral_constant<int, 0>{}) : with_subset(std::integral_constant<int, 1>{});
}
// f(nsl) with n = 1 .. NMAX slices as a compile-time tag
template <int NMAX, class F>
hipError_t slices_dispatch(int n, F&& f) {
    static_assert(NMAX >= 1 && NMAX <= CT_MAX_SLICES, "1 .. 4 slices");
    if (n == 1) return f(std::integral_constant<int, 1>{});
    if constexpr (NMAX >= 2) if (n == 2) return f(std::integral_constant<int, 2>{});
    if constexpr (NMAX >= 3) if (n == 3) return f(std::integral_constant<int, 3>{});
    if constexpr (NMAX >= 4) if (n == 4) return f(std::integral_constant<int, 4>{});
    return hipErrorInvalidValue;
}
// n_slices in chunks of NFULL: f(nsl, first_chunk, n_chunks) for the full chunks in one launch, then for the last narrower chunk (if any)
template <int NFULL, class F>
hipError_t chunks_dispatch(int n_slices, F&& f) {
    const int n_full = n_slices / NFULL, rem = n_slices % NFULL;
    if (n_full > 0)
        if (hipError_t e = f(std::integral_constant<int, NFULL>{}, 0, n_full); e != hipSuccess) return e;
    if (rem == 0) return hipSuccess;
    return slices_dispatch<(NFULL > 1 ? NFULL - 1 : 1)>(rem, [&](auto nsl) { return f(nsl, n_full, 1); });
}

// the store of a scan: dim_pad a positive multiple of 64, ntotal within the 32-bit row arithmetic of the kernels
inline bool scan_store_ok(const ScanInputs& s) { return s.dim_pad % 64 == 0 && s.dim_pad > 0 && s.ntotal >= 0 && s.ntotal < (1ll << 31) - 512; }
// a value table (or a weight matrix) of n_cols columns padded to c_pad = 64 | 128 | 192 | 256
inline bool readout_cols_ok(int c_pad, int n_cols) { return c_pad % 64 == 0 && c_pad >= 64 && c_pad <= 64 * CT_MAX_SLICES && n_cols >= 1 && n_cols <= c_pad; }

}  // namespace vodhip
