// The exact divergence between TWO retriever posteriors over the WHOLE store (vodhip_index_posterior_divergence, include/vodhip.h H2d):
//   p(z) = softmax(beta_a s_a),  r(z) = softmax(beta_b s_b),  s_a = <a~, x~_z>,  s_b = <b~, x~_z>  over the rows eligible for the pair,
//   (max_a, log_rel_a, mean_rel_a = E_p[s_a] - max_a, cross_rel_ab = E_p[s_b] - max_b)  and the mirror  (max_b, log_rel_b, mean_rel_b,
//   cross_rel_ba = E_r[s_a] - max_a),
// from which H(p), H(p, r) = log_rel_b - beta_b cross_rel_ab and KL(p || r) follow without a beta * max cancellation.  It is the
// posterior_stats scan (kernels_stats.hip) over 2 nq staged queries with the cross moments in place of the second moments.
//
// THE PAIR LAYOUT.  A lane's two accumulator columns are columns fr and 32 + fr of its wave's 64 staged queries (store_scan.h: NJ == 2
// in both instantiations).  Pair p of a launch stages its query a at column p % 32 of the 64-column block p / 32 and its query b at
// column 32 + p % 32 of the same block: every lane then holds s_a and s_b of the same stored row in the same registers of acc[.][0] and
// acc[.][1], and the cross sums are lane-local.  The K loop is scan_k_loop, unchanged: the score contract holds.
//   stage    div_stage_kernel: scan_stage_kernel's rounding and padding behind that row map
//   scan     TWO partials per (tile, pair): (m_a, l_a, a_a, c_ab) and (m_b, l_b, a_b, c_ba).  m, l, a are formed with the instructions
//            and in the order of stats_scan_kernel; c_ab = sum e_a (s_b - m_b) with m_b the tile's own maximum of side b: every term
//            is <= 0, a same-sign sum like a, under the same `live` rule (a row whose e_a is 0 adds +0: 0 * -inf is never formed).
//            A row is eligible for the pair when it is eligible for both columns; labels and q < nq are tested on the pair index.
//            A tile in which side b has no finite score (m_b not finite) takes s_b - m_b as -inf: c_ab = -inf if side a has mass.
//   finish   one workgroup per pair: per side max and L as the log-partition finish forms them, A and L' as stats_finish_kernel, and
//            C_ab = sum_t c^a_t (c_ab_t + (m_b_t - M_b) l_a_t) in double, ONE thread adding in increasing tile order; tiles with
//            l_a_t == 0 or c^a_t == 0 are left out, a tile with mass whose m_b_t is -inf contributes -inf.
//            mean_rel = A / L', cross_rel = C / L', each rounded to float32 once.
// A side with no eligible row (or all -inf) is (-inf, -inf, NaN), one with a +inf score (+inf, +inf, NaN); BOTH cross words are NaN
// then, and the other side's own three words are what they are without it.  Floating-point contraction is off in this file.
// ONE order per pair, fixed by ntotal and dim_pad alone: no atomics, the same bits in any batch, at any position, in both instantiations.
#include "store_scan.h"

#pragma clang fp contract(off)

namespace vodhip {

namespace {

// staged row R of [nq_pad][dim_pad]: pair (R / 64) * 32 + R % 32 of the launch, side (R % 64) / 32; rounding and padding as
// scan_stage_kernel (kernels_partition.hip)
__global__ void __launch_bounds__(256) div_stage_kernel(const void* __restrict__ qa_src, const void* __restrict__ qb_src, int q_dtype,
                                                        int64_t q_first, int64_t npairs, int64_t dim, uint16_t* __restrict__ q_pad,
                                                        int store_dtype, int64_t nq_pad, int64_t dim_pad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t chunks_per_row = dim_pad / 8;
    if (i >= nq_pad * chunks_per_row) return;
    const int64_t row = i / chunks_per_row;
    const int64_t c0 = (i % chunks_per_row) * 8;
    const int64_t pair = (row >> 6) * 32 + (row & 31);
    const void* q_src = (row & 32) ? qb_src : qa_src;
    uint16_t out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t c = c0 + e;
        uint16_t v = 0;
        if (pair < npairs && c < dim) {
            const int64_t at = (q_first + pair) * dim + c;
            float f;
            if (q_dtype == 2) f = ((const float*)q_src)[at];
            else if (q_dtype == 0) f = (float)(((const _Float16*)q_src)[at]);
            else f = (float)(((const __bf16*)q_src)[at]);
            float rounded;
            v = store_bits(f, store_dtype, &rounded);
        }
        out[e] = v;
    }
    *(uint4*)(q_pad + row * dim_pad + c0) = *(const uint4*)out;
}

// X, Q as partition_scan_kernel (Q in the pair layout); part: [n_qtiles * BN / 2 pairs][n_xtiles][2 sides] (m, l, a, c)
template <int DT, int BN, int WN, bool SUBSET>
__global__ __launch_bounds__(scan_threads(WN), 1)
void div_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles,
                     int npairs, float beta_a, float beta_b, float4* __restrict__ part, FilterExtra ex) {
    constexpr int WM = SCAN_WM;
    constexpr int TM = SCAN_BM / WM, TN = BN / WN;
    constexpr int MI = TM / 32, NJ = TN / 32;
    static_assert(NJ == 2 && TN == 64, "a lane's two columns are the two sides of one pair");
    static_assert(4 * WM * BN * (int)sizeof(float) <= scan_ring_bytes(BN) / SCAN_NSTAGE, "the reduction arrays reuse the first ring slot");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    int qt, xt;
    if (!scan_block_tile(blockIdx.x, n_qtiles, n_xtiles, &qt, &xt)) return;
    const int x0 = xt * SCAN_BM;
    const int q0 = qt * BN;

    f32x16 acc[MI][NJ];
    scan_k_loop<DT, BN, WN>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 31, fh = lane >> 5;

    // ---- epilogue
    __syncthreads();  // every wave has read its last fragments: the first ring slot becomes the four reduction arrays
    float* red_m = reinterpret_cast<float*>(smem);  // [WM][BN]
    float* red_l = red_m + WM * BN;                 // [WM][BN]
    float* red_a = red_l + WM * BN;                 // [WM][BN]
    float* red_c = red_a + WM * BN;                 // [WM][BN]
    const float inf = __builtin_inff();
    const int rlane = x0 + wm * TM + 4 * fh;        // the lane's row of (block 0, register 0)
    const int pair = (q0 + wn * TN) / 2 + fr;       // the lane's pair of the launch: 64-column block (q0 + wn * 64) / 64, column fr
    // eligible for the pair: for both columns (in range, neither score NaN), then the pair's labels
    unsigned okm = 0u;
    if (pair < npairs) {
        okm = scan_eligible_mask<false>(acc[0][0], acc[1][0], rlane, ntotal, pair, ex) &
              scan_eligible_mask<false>(acc[0][1], acc[1][1], rlane, ntotal, pair, ex);
        if constexpr (SUBSET) {  // rolled: one label test per row that is still in
            unsigned m2 = okm;
            while (m2) {
                const int b = __builtin_ctz(m2);
                m2 &= m2 - 1;
                if (!subset_allows(ex, pair, scan_lane_row(rlane, b))) okm &= ~(1u << b);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        float mx = -inf;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = (okm & (1u << (i * 16 + r))) ? fmaxf(mx, acc[i][j][r]) : mx;
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (fh == 0) red_m[wm * BN + col] = mx;
    }
    __syncthreads();
    float tile_m[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        float m = red_m[col];
#pragma unroll
        for (int w = 1; w < WM; ++w) m = fmaxf(m, red_m[w * BN + col]);
        tile_m[j] = m;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        const float beta = j == 0 ? beta_a : beta_b;
        const float m = tile_m[j], mo = tile_m[1 - j];  // this side's maximum, the other side's
        const bool fin = m > -inf && m < inf;
        const bool fin_o = mo > -inf && mo < inf;
        float l = 0.f, a = 0.f, c = 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = acc[i][j][r] - m;
                const float e = expf(beta * d);
                const bool on = fin && (okm & (1u << (i * 16 + r)));
                l += on ? e : 0.f;
                const bool live = on && e > 0.f;  // (e > 0: d is finite)
                const float t = e * d;
                a += live ? t : 0.f;
                const float dc = fin_o ? acc[i][1 - j][r] - mo : -inf;  // (<= 0, -inf for a -inf score; never inf - inf)
                const float u = e * dc;
                c += live ? u : 0.f;
            }
        l += __shfl_xor(l, 32, 64);  // (h = 0) + (h = 1): the same value in both lanes
        a += __shfl_xor(a, 32, 64);
        c += __shfl_xor(c, 32, 64);
        if (fh == 0) {
            red_l[wm * BN + col] = l;
            red_a[wm * BN + col] = a;
            red_c[wm * BN + col] = c;
        }
    }
    __syncthreads();
    if (wm == 0 && fh == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = wn * TN + j * 32 + fr;
            float l = red_l[col], a = red_a[col], c = red_c[col];
#pragma unroll
            for (int w = 1; w < WM; ++w) {
                l += red_l[w * BN + col];
                a += red_a[w * BN + col];
                c += red_c[w * BN + col];
            }
            if (tile_m[j] == inf) l = inf;
            part[((size_t)pair * n_xtiles + xt) * 2 + j] = make_float4(tile_m[j], l, a, c);
        }
    }
}

// One workgroup per pair, as stats_finish_kernel: the two maxima, then the terms of a chunk of tiles by all threads and ONE thread that
// adds them in increasing tile order - L in float32 (the log-partition finish's adds: the same bits), A, C and L' in double.
constexpr int DFIN_T = 256, DFIN_CHUNK = 512;
__global__ void __launch_bounds__(DFIN_T) div_finish_kernel(const float4* __restrict__ part, int64_t n_tiles, float beta_a, float beta_b,
                                                            float* __restrict__ o_max_a, float* __restrict__ o_log_rel_a,
                                                            float* __restrict__ o_mean_rel_a, float* __restrict__ o_cross_ab,
                                                            float* __restrict__ o_max_b, float* __restrict__ o_log_rel_b,
                                                            float* __restrict__ o_mean_rel_b, float* __restrict__ o_cross_ba) {
    __shared__ float sv[2][DFIN_CHUNK];
    __shared__ double sl[2][DFIN_CHUNK], sa[2][DFIN_CHUNK], sc[2][DFIN_CHUNK];
    __shared__ float red[2][DFIN_T / 64];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float4* p = part + q * n_tiles * 2;
    const float inf = __builtin_inff();
    float M[2] = {-inf, -inf};
    for (int64_t t = tid; t < n_tiles; t += DFIN_T) {
        M[0] = fmaxf(M[0], p[2 * t].x);
        M[1] = fmaxf(M[1], p[2 * t + 1].x);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) M[s] = fmaxf(M[s], __shfl_xor(M[s], k, 64));
        if ((tid & 63) == 0) red[s][tid >> 6] = M[s];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; ++s) M[s] = fmaxf(fmaxf(red[s][0], red[s][1]), fmaxf(red[s][2], red[s][3]));
    const bool fin[2] = {M[0] != inf && M[0] != -inf, M[1] != inf && M[1] != -inf};  // (uniform over the workgroup)
    const float beta[2] = {beta_a, beta_b};
    float L[2] = {0.f, 0.f};
    double Ld[2] = {0.0, 0.0}, A[2] = {0.0, 0.0}, C[2] = {0.0, 0.0};
    if (fin[0] || fin[1]) {
        for (int64_t c0 = 0; c0 < n_tiles; c0 += DFIN_CHUNK) {
            const int n = (int)(n_tiles - c0 < DFIN_CHUNK ? n_tiles - c0 : DFIN_CHUNK);
            for (int i = tid; i < n; i += DFIN_T) {
                const float4 w[2] = {p[2 * (c0 + i)], p[2 * (c0 + i) + 1]};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const float4 v = w[s];
                    float tv = 0.f;
                    double tl = 0.0, ta = 0.0, tc = 0.0;
                    if (fin[s]) {
                        const float c = expf(beta[s] * (v.x - M[s]));
                        tv = v.y * c;  // (an empty tile is (-inf, 0): 0 * 0)
                        if (v.y != 0.f && c != 0.f) {  // (c > 0: D is finite)
                            const double D = (double)v.x - (double)M[s], l = (double)v.y, a = (double)v.z, cd = (double)c;
                            tl = cd * l;
                            ta = cd * (a + D * l);
                            if (fin[1 - s]) {
                                const float mo = w[1 - s].x;  // the other side's maximum of this tile
                                if (mo == -inf) tc = -(double)inf;  // mass on rows the other side scores -inf
                                else {
                                    const double Do = (double)mo - (double)M[1 - s], x = (double)v.w;
                                    tc = cd * (x + Do * l);
                                }
                            }
                        }
                    }
                    sv[s][i] = tv;
                    sl[s][i] = tl;
                    sa[s][i] = ta;
                    sc[s][i] = tc;
                }
            }
            __syncthreads();
            if (tid == 0)
                for (int i = 0; i < n; ++i) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        L[s] += sv[s][i];
                        Ld[s] += sl[s][i];
                        A[s] += sa[s][i];
                        C[s] += sc[s][i];
                    }
                }
            __syncthreads();
        }
    }
    if (tid == 0) {
        const float nan = __builtin_nanf("");
        float* o_max[2] = {o_max_a, o_max_b};
        float* o_rel[2] = {o_log_rel_a, o_log_rel_b};
        float* o_mean[2] = {o_mean_rel_a, o_mean_rel_b};
        float* o_cross[2] = {o_cross_ab, o_cross_ba};
        const bool both = fin[0] && fin[1];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            o_max[s][q] = M[s];
            if (fin[s]) {
                const double mean = A[s] / Ld[s];
                o_rel[s][q] = logf(L[s]);
                o_mean[s][q] = (float)mean;
            } else {
                o_rel[s][q] = M[s];
                o_mean[s][q] = nan;
            }
            o_cross[s][q] = both ? (float)(C[s] / Ld[s]) : nan;
        }
    }
}

}  // namespace

hipError_t launch_posterior_divergence(const DivergenceArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = scan_nq_pad(2 * nq);
    const int64_t n_tiles = scan_tiles(a.ntotal);
    if (a.dim_pad % 64 != 0 || a.dim_pad <= 0 || a.ntotal < 0 || a.ntotal >= (1ll << 31) - 512 || nq > (1 << 19)) return hipErrorInvalidValue;
    if (n_tiles > 0) {
        const int64_t n = nq_pad * (a.dim_pad / 8);
        hipLaunchKernelGGL(div_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.q_src, a.q_src_b, a.q_dtype, q_first, nq, a.dim,
                           (uint16_t*)a.q_stage, a.store_dtype, nq_pad, a.dim_pad);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        const FilterExtra ex = scan_filter_extra(a, q_first);
        const hipError_t e = scan_dispatch(a.store_dtype, nq_pad, ex.row_label != nullptr, [&](auto dt, auto bn, auto wn, auto subset) {
            const int n_qtiles = (int)(nq_pad / bn.value);
            return scan_launch<bn.value, wn.value>(div_scan_kernel<dt.value, bn.value, wn.value, subset.value>, scan_grid((int)n_tiles, n_qtiles), stream,
                                                   (const uint16_t*)a.store, (const uint16_t*)a.q_stage, (int)a.dim_pad, (int)a.ntotal, (int)n_tiles,
                                                   n_qtiles, (int)nq, a.beta_a, a.beta_b, (float4*)a.part, ex);
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(div_finish_kernel, dim3((unsigned)nq), dim3(DFIN_T), 0, stream, (const float4*)a.part, n_tiles, a.beta_a, a.beta_b,
                       a.out[0] + q_first, a.out[1] + q_first, a.out[2] + q_first, a.out[3] + q_first, a.out[4] + q_first, a.out[5] + q_first,
                       a.out[6] + q_first, a.out[7] + q_first);
    return hipGetLastError();
}

}  // namespace vodhip
