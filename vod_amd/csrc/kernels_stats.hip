// The moments of the score under the retriever's posterior over the WHOLE store (vodhip_index_posterior_stats, include/vodhip.h H2t):
//   p(z | q) = exp(beta s_z - log Z_beta(q)),  s_z = <q~, x~_z>,
//   max_score, log_rel   the two words of the log-partition scan (kernels_partition.hip), bit for bit
//   mean_rel = E_p[s] - max_score <= 0,   var = Var_p[s] >= 0
// so that E_p[s] = d log Z / d beta, Var_p[s] = d^2 log Z / d beta^2 and the entropy H(p) = log_rel - beta * mean_rel (two
// non-negative terms).  It is the log-partition scan with two more accumulators: with d = s - m <= 0 and e = exp(beta d),
//   scan     ONE partial (m, l, a, b) per (tile, query): m and l as partition_scan_kernel forms them (the same instructions in the same
//            order), a = sum e d <= 0, b = sum e d^2 >= 0 - same-sign sums, no cancellation
//   finish   max_score and log_rel as partition_finish_kernel forms them; with D_t = m_t - max_score <= 0, c_t = exp(beta D_t):
//            A = sum_t c_t (a_t + D_t l_t),  B = sum_t c_t (b_t + 2 D_t a_t + D_t^2 l_t),  L' = sum_t c_t l_t  in double,
//            mean_rel = A / L',  var = max(0, B / L' - (A / L')^2), each rounded to float32 once.
//
// ONE order per query, fixed by ntotal and dim_pad alone (the rules of kernels_partition.hip): a lane adds its terms in register order
// starting from 0 (a row that is not eligible, or whose e is 0, adds +0: 0 * -inf is never formed), the two lane halves add as
// (h = 0) + (h = 1), the four row waves as ((w0 + w1) + w2) + w3; the finish forms a tile's three terms in double from the float32
// words (c_t is the float32 expf the log-partition finish uses) and ONE thread adds them in increasing tile order; tiles with l_t == 0
// or c_t == 0 are left out (0 * inf is never formed).  Floating-point contraction is off in this file: e * d and t * d are rounded
// products in every instantiation.
// No eligible row (or scores that are all -inf): (-inf, -inf, NaN, NaN).  A +inf score: (+inf, +inf, NaN, NaN).  Eligible rows that
// all score the same: every d and every D_t is 0, so mean_rel == 0 and var == 0 exactly.
#include "store_scan.h"

#pragma clang fp contract(off)

namespace vodhip {

namespace {

// X, Q as partition_scan_kernel; part: [n_qtiles * BN][n_xtiles] (m, l, a, b)
template <int DT, int BN, int WN, bool SUBSET>
__global__ __launch_bounds__(scan_threads(WN), 1)
void stats_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles,
                       int nq, float beta, float4* __restrict__ part, FilterExtra ex) {
    constexpr int WM = SCAN_WM;
    constexpr int TM = SCAN_BM / WM, TN = BN / WN;
    constexpr int MI = TM / 32, NJ = TN / 32;
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
    float* red_b = red_a + WM * BN;                 // [WM][BN]
    const float inf = __builtin_inff();
    const int rlane = x0 + wm * TM + 4 * fh;        // the lane's row of (block 0, register 0)
    unsigned okm[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        const int q = q0 + col;
        const unsigned mask = q < nq ? scan_eligible_mask<SUBSET>(acc[0][j], acc[1][j], rlane, ntotal, q, ex) : 0u;
        float mx = -inf;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = (mask & (1u << (i * 16 + r))) ? fmaxf(mx, acc[i][j][r]) : mx;
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (fh == 0) red_m[wm * BN + col] = mx;
        okm[j] = mask;
    }
    __syncthreads();
    float tile_m[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        float m = red_m[col];
#pragma unroll
        for (int w = 1; w < WM; ++w) m = fmaxf(m, red_m[w * BN + col]);
        const bool fin = m > -inf && m < inf;
        float l = 0.f, a = 0.f, b = 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d = acc[i][j][r] - m;
                const float e = expf(beta * d);
                const bool on = fin && (okm[j] & (1u << (i * 16 + r)));
                l += on ? e : 0.f;
                const bool live = on && e > 0.f;  // (e > 0: d is finite)
                const float t = e * d;
                a += live ? t : 0.f;
                b += live ? t * d : 0.f;
            }
        l += __shfl_xor(l, 32, 64);  // (h = 0) + (h = 1): the same value in both lanes
        a += __shfl_xor(a, 32, 64);
        b += __shfl_xor(b, 32, 64);
        if (fh == 0) {
            red_l[wm * BN + col] = l;
            red_a[wm * BN + col] = a;
            red_b[wm * BN + col] = b;
        }
        tile_m[j] = m;
    }
    __syncthreads();
    if (wm == 0 && fh == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = wn * TN + j * 32 + fr;
            float l = red_l[col], a = red_a[col], b = red_b[col];
#pragma unroll
            for (int w = 1; w < WM; ++w) {
                l += red_l[w * BN + col];
                a += red_a[w * BN + col];
                b += red_b[w * BN + col];
            }
            if (tile_m[j] == inf) l = inf;
            part[(size_t)(q0 + col) * n_xtiles + xt] = make_float4(tile_m[j], l, a, b);
        }
    }
}

// One workgroup per query, as partition_finish_kernel: the maximum, then the terms of a chunk of tiles by all threads and ONE thread
// that adds them in increasing tile order - L in float32 (the log-partition finish's adds: the same bits), A, B and L' in double.
constexpr int SFIN_T = 256, SFIN_CHUNK = 1024;
__global__ void __launch_bounds__(SFIN_T) stats_finish_kernel(const float4* __restrict__ part, int64_t n_tiles, float beta,
                                                              float* __restrict__ out_max, float* __restrict__ out_log_rel,
                                                              float* __restrict__ out_mean_rel, float* __restrict__ out_var) {
    __shared__ float sv[SFIN_CHUNK];
    __shared__ double sl[SFIN_CHUNK], sa[SFIN_CHUNK], sb[SFIN_CHUNK];
    __shared__ float red[SFIN_T / 64];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float4* p = part + q * n_tiles;
    const float inf = __builtin_inff();
    float m = -inf;
    for (int64_t t = tid; t < n_tiles; t += SFIN_T) m = fmaxf(m, p[t].x);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m == inf || m == -inf) {  // (uniform over the workgroup)
        if (tid == 0) {
            const float nan = __builtin_nanf("");
            out_max[q] = m;
            out_log_rel[q] = m;
            out_mean_rel[q] = nan;
            out_var[q] = nan;
        }
        return;
    }
    float L = 0.f;
    double Ld = 0.0, A = 0.0, B = 0.0;
    for (int64_t c0 = 0; c0 < n_tiles; c0 += SFIN_CHUNK) {
        const int n = (int)(n_tiles - c0 < SFIN_CHUNK ? n_tiles - c0 : SFIN_CHUNK);
        for (int i = tid; i < n; i += SFIN_T) {
            const float4 v = p[c0 + i];
            const float c = expf(beta * (v.x - m));
            sv[i] = v.y * c;  // (an empty tile is (-inf, 0): 0 * 0)
            double tl = 0.0, ta = 0.0, tb = 0.0;
            if (v.y != 0.f && c != 0.f) {  // (c > 0: D is finite)
                const double D = (double)v.x - (double)m, l = (double)v.y, a = (double)v.z, b = (double)v.w, cd = (double)c;
                tl = cd * l;
                ta = cd * (a + D * l);
                tb = cd * (b + 2.0 * D * a + D * D * l);
            }
            sl[i] = tl;
            sa[i] = ta;
            sb[i] = tb;
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < n; ++i) {
                L += sv[i];
                Ld += sl[i];
                A += sa[i];
                B += sb[i];
            }
        __syncthreads();
    }
    if (tid == 0) {
        const double mean = A / Ld;
        const double var = B / Ld - mean * mean;
        out_max[q] = m;
        out_log_rel[q] = logf(L);
        out_mean_rel[q] = (float)mean;
        out_var[q] = (float)(var > 0.0 ? var : 0.0);
    }
}

}  // namespace

hipError_t launch_posterior_stats(const StatsArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = scan_nq_pad(nq);
    const int64_t n_tiles = scan_tiles(a.ntotal);
    if (a.dim_pad % 64 != 0 || a.dim_pad <= 0 || a.ntotal < 0 || a.ntotal >= (1ll << 31) - 512 || nq > (1 << 20)) return hipErrorInvalidValue;
    if (n_tiles > 0) {
        if (hipError_t e = launch_scan_stage(a, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
        const FilterExtra ex = scan_filter_extra(a, q_first);
        const hipError_t e = scan_dispatch(a.store_dtype, nq_pad, ex.row_label != nullptr, [&](auto dt, auto bn, auto wn, auto subset) {
            const int n_qtiles = (int)(nq_pad / bn.value);
            return scan_launch<bn.value, wn.value>(stats_scan_kernel<dt.value, bn.value, wn.value, subset.value>, scan_grid((int)n_tiles, n_qtiles), stream,
                                                   (const uint16_t*)a.store, (const uint16_t*)a.q_stage, (int)a.dim_pad, (int)a.ntotal, (int)n_tiles,
                                                   n_qtiles, (int)nq, a.beta, (float4*)a.part, ex);
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(stats_finish_kernel, dim3((unsigned)nq), dim3(SFIN_T), 0, stream, (const float4*)a.part, n_tiles, a.beta, a.out_max + q_first,
                       a.out_log_rel + q_first, a.out_mean_rel + q_first, a.out_var + q_first);
    return hipGetLastError();
}

}  // namespace vodhip
