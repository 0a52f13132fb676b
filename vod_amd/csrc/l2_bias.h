// The bias columns of an L2 store (VODHIP_L2): the split of c = -|x~|^2 / 2 into three store-dtype terms and the three query
// constants they meet in the contraction, so that  sum_i const_i * term_i = c  rides in the scan's own inner product:
//     |q - x|^2 = |q|^2 - 2 (q.x + c),      q.x + c = < [x, t0, t1, t2], [q, a0, a1, a2] >.
// Host + device, no HIP call: the ingest kernel (kernels_l2.hip), vodhip_debug_l2_split and the CPU tests run the same code.
//
// Every rounding below is round-to-nearest-even of a float32 to the store dtype's significand (fp16: 11 bits, bf16: 8), done on
// the float32's bits.  A term is either ZERO or NORMAL in the store dtype, and so is every constant: how the MFMA treats subnormal
// 16-bit A / B operands is not documented, so none is ever stored.  Every remainder r - a * t is exact in float32 (it is a
// multiple of the float32's last place below half a unit of t's last place).
//
//   fp16:  a = (2^8, 2^-3, 2^-14).  Term i covers magnitudes a_i * [2^-14, 65504]: [2^-6, 2^24), [2^-17, 2^13), [2^-28, 2^2).
//          A remainder below a term's range leaves that term zero and goes to the next one whole.  For |c| >= 2^-6 the three
//          terms hold 11 + 11 + 2 bits: the sum is c exactly, unless the last remainder is below 2^-28 and is dropped.  Below
//          2^-6 the first term is zero and two terms hold 22 of the 24 bits: the rest, at most 2^-29, is dropped.
//          Residual bound  r(c) = 2^-28  (absolute; <= 1 ulp of c in float32 for |c| >= 2^-5; 0 for half-integers below 2^23).
//          Limit: |c| <= 65504 * 2^8 = 16769024, i.e. |x~|^2 <= 33538048 (just under 2^25).
//   bf16:  a = (1, 1, 1).  The terms hold 8 + 8 + 8 bits: the sum is c exactly, unless a remainder is below 2^-126 (the smallest
//          normal bf16) and is dropped.  Residual bound  r(c) = 2^-126.  Limit: |c| <= 2^120 (so that |q|^2 - 2 s stays finite).
//
// Beyond the limit (or for a NaN / infinite |x~|^2) the bias SATURATES: t0 = -limit / a0, t1 = t2 = 0, and the caller counts the
// row ("l2_saturated_rows").  Such a row scores q.x~ - limit instead of q.x~ - |x~|^2 / 2: it ranks behind every row within the
// limit as long as q.x~ itself stays well below the limit (|q~| |x~| < 1.6e7 for fp16); the counter is how a caller learns of it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VOD_L2_HD __host__ __device__ inline
#else
#define VOD_L2_HD inline
#endif

namespace vodhip {

constexpr int L2_BIAS_COLS = 3;

VOD_L2_HD float l2_bits_to_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
VOD_L2_HD uint32_t l2_float_to_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
// 2^e as a float32, -126 <= e <= 127
VOD_L2_HD float l2_pow2(int e) { return l2_bits_to_float((uint32_t)(e + 127) << 23); }

// the three query constants of a store dtype (0 = fp16, 1 = bf16), as float32 values and as store-dtype bits
VOD_L2_HD void l2_query_consts(int store_dtype, float consts[3], uint16_t bits[3]) {
    if (store_dtype == 0) {
        consts[0] = 256.f;             // 2^8
        consts[1] = 0.125f;            // 2^-3
        consts[2] = 6.103515625e-05f;  // 2^-14, the smallest normal fp16
        bits[0] = 0x5C00;
        bits[1] = 0x3000;
        bits[2] = 0x0400;
    } else {
        consts[0] = consts[1] = consts[2] = 1.f;
        bits[0] = bits[1] = bits[2] = 0x3F80;
    }
}

// the largest |c| the split represents, and the bound on |c - sum_i const_i * term_i| below it
VOD_L2_HD float l2_split_limit(int store_dtype) { return store_dtype == 0 ? 16769024.f : l2_pow2(120); }
VOD_L2_HD float l2_split_residual(int store_dtype) { return store_dtype == 0 ? l2_pow2(-28) : l2_pow2(-126); }

// One term: v rounded to the store dtype (round-to-nearest-even), or zero when |v| is below the dtype's smallest normal.  The
// caller keeps |v| within the dtype's finite range.  *rounded receives the value the bits stand for.
VOD_L2_HD uint16_t l2_round_term(float v, int store_dtype, float* rounded) {
    const uint32_t u = l2_float_to_bits(v);
    const uint32_t sign = u & 0x80000000u, mag = u & 0x7fffffffu;
    if (store_dtype == 0) {
        if (mag < 0x38800000u) {  // |v| < 2^-14
            *rounded = 0.f;
            return 0;
        }
        const uint32_t r = (mag + 0xFFFu + ((mag >> 13) & 1u)) & ~0x1FFFu;  // 10 fraction bits; a carry moves into the exponent
        *rounded = l2_bits_to_float(sign | r);
        return (uint16_t)((sign >> 16) | ((r - 0x38000000u) >> 13));  // exponent re-biased 127 -> 15
    }
    if (mag < 0x00800000u) {  // |v| < 2^-126
        *rounded = 0.f;
        return 0;
    }
    const uint32_t r = (mag + 0x7FFFu + ((mag >> 16) & 1u)) & ~0xFFFFu;
    *rounded = l2_bits_to_float(sign | r);
    return (uint16_t)((sign | r) >> 16);
}

// c = -|x~|^2 / 2 -> the three stored terms.  Returns 1 when the bias saturated (|c| beyond the limit, or not finite).
VOD_L2_HD int l2_split(float c, int store_dtype, uint16_t terms[3]) {
    float a[3];
    uint16_t abits[3];
    l2_query_consts(store_dtype, a, abits);
    const float lim = l2_split_limit(store_dtype);
    if (!(c >= -lim && c <= lim)) {  // (also NaN)
        float t;
        terms[0] = l2_round_term(-lim / a[0], store_dtype, &t);
        terms[1] = terms[2] = 0;
        return 1;
    }
    float r = c;
    for (int i = 0; i < 3; ++i) {
        float t;
        terms[i] = l2_round_term(r / a[i], store_dtype, &t);  // (a power of two: the quotient is exact)
        r -= a[i] * t;                                        // exact
    }
    return 0;
}

}  // namespace vodhip
