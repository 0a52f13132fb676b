// The exact softmax normaliser of the retriever over the WHOLE store (vodhip_index_log_partition, include/vodhip.h H2p):
//   log Z_beta(q) = log sum_{rows z < ntotal, eligible} exp(beta <q~, x~_z>) = beta * max_score + log_rel,
//   max_score = max_z <q~, x~_z>,  log_rel = log sum_z exp(beta (<q~, x~_z> - max_score)) >= 0.
// Three kernels:
//   stage    queries -> [nq_pad][dim_pad] of the store dtype (launch_scan_stage: the one staging kernel of every whole-store scan)
//   scan     the shared scan core (store_scan.h: K loop, C layout and eligibility rule) over a 256-row tile x 64 | 128 queries with a
//            max-stabilised sum of exponentials as its epilogue: ONE partial (m, l) per (tile, query), m = the tile's maximum,
//            l = sum exp(beta (s - m))
//   finish   folds a query's partials into (max_score, log_rel)
//
// ONE summation order per query, fixed by ntotal (and dim_pad, the length of the K loop) alone - not by nq, by the other queries of the
// batch, by the query tile width or by the grid:
//   score   the scan core's (store_scan.h);
//   tile t  holds rows [256 t, 256 t + 256).  Wave w of its 4 row waves holds rows 64 w .. 64 w + 63: lane half h (lane >> 5) of the
//           query's two lanes holds, in register order (block i = 0, 1; register r = 0 .. 15), the rows 64 w + 32 i + 4 h + (r & 3) +
//           8 (r >> 2).  m = the maximum over the tile's eligible rows (a maximum has no order).  Each lane adds its terms
//           exp(beta (s - m)) in register order starting from 0 (an ineligible row adds +0), the two halves add as (h = 0) + (h = 1),
//           the four waves as ((w0 + w1) + w2) + w3.
//   finish  max_score = the maximum of the tile maxima; L = sum over t = 0, 1, .. in increasing order of l_t * exp(beta (m_t - max_score)),
//           starting from 0; log_rel = log L.  The tile that holds the maximum contributes l_t >= 1 times exactly 1: log_rel >= 0.
// The 64-query and the 128-query instantiation differ in the number of query columns a workgroup carries, not in any of the above, so a
// query's two words are the same bits alone, as row 217 of 300, and on every repeat (there are no atomics).
// expf and logf are the library functions (1 ulp each in the HIP math accuracy table), not the native approximations.
// No eligible row: (-inf, -inf).  A +inf score: (+inf, +inf).  Scores that are all -inf count as no row.
#include "store_scan.h"

namespace vodhip {

namespace {

__global__ void __launch_bounds__(256) scan_stage_kernel(const void* __restrict__ q_src, int q_dtype, int64_t q_first, int64_t nq, int64_t dim,
                                                         uint16_t* __restrict__ q_pad, int store_dtype, int64_t nq_pad, int64_t dim_pad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t chunks_per_row = dim_pad / 8;
    if (i >= nq_pad * chunks_per_row) return;
    const int64_t row = i / chunks_per_row;
    const int64_t c0 = (i % chunks_per_row) * 8;
    uint16_t out[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t c = c0 + e;
        uint16_t v = 0;
        if (row < nq && c < dim) {
            const int64_t at = (q_first + row) * dim + c;
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

// X: the store [>= n_xtiles * 256 rows][dim_pad]; Q: the staged queries [n_qtiles * BN][dim_pad]; part: [n_qtiles * BN][n_xtiles] (m, l)
template <int DT, int BN, int WN, bool SUBSET>
__global__ __launch_bounds__(scan_threads(WN), 1)
void partition_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles,
                           int nq, float beta, float2* __restrict__ part, FilterExtra ex) {
    constexpr int WM = SCAN_WM;
    constexpr int TM = SCAN_BM / WM, TN = BN / WN;
    constexpr int MI = TM / 32, NJ = TN / 32;
    static_assert(2 * WM * BN * (int)sizeof(float) <= scan_ring_bytes(BN) / SCAN_NSTAGE, "the reduction arrays reuse the first ring slot");

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
    __syncthreads();  // every wave has read its last fragments: the first ring slot becomes the two reduction arrays
    float* red_m = reinterpret_cast<float*>(smem);  // [WM][BN]
    float* red_l = red_m + WM * BN;                 // [WM][BN]
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
        float l = 0.f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = expf(beta * (acc[i][j][r] - m));
                l += (fin && (okm[j] & (1u << (i * 16 + r)))) ? e : 0.f;
            }
        l += __shfl_xor(l, 32, 64);  // (h = 0) + (h = 1): the same value in both lanes
        if (fh == 0) red_l[wm * BN + col] = l;
        tile_m[j] = m;
    }
    __syncthreads();
    if (wm == 0 && fh == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = wn * TN + j * 32 + fr;
            float l = red_l[col];
#pragma unroll
            for (int w = 1; w < WM; ++w) l += red_l[w * BN + col];
            if (tile_m[j] == inf) l = inf;
            part[(size_t)(q0 + col) * n_xtiles + xt] = make_float2(tile_m[j], l);
        }
    }
}

// One workgroup per query; part row q holds the query's partials in tile order.  The maximum has no order; the terms
// v_t = l_t * exp(beta (m_t - max)) are computed by all threads, FIN_CHUNK tiles at a time, and ONE thread adds them in increasing
// tile order (the adds are the only ordered part, and they read LDS).
constexpr int FIN_T = 256, FIN_CHUNK = 2048;
__global__ void __launch_bounds__(FIN_T) partition_finish_kernel(const float2* __restrict__ part, int64_t n_tiles, float beta,
                                                                 float* __restrict__ out_max, float* __restrict__ out_log_rel) {
    __shared__ float sv[FIN_CHUNK];
    __shared__ float red[FIN_T / 64];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float2* p = part + q * n_tiles;
    const float inf = __builtin_inff();
    float m = -inf;
    for (int64_t t = tid; t < n_tiles; t += FIN_T) m = fmaxf(m, p[t].x);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (m == inf || m == -inf) {  // (uniform over the workgroup)
        if (tid == 0) {
            out_max[q] = m;
            out_log_rel[q] = m;
        }
        return;
    }
    float L = 0.f;
    for (int64_t c0 = 0; c0 < n_tiles; c0 += FIN_CHUNK) {
        const int n = (int)(n_tiles - c0 < FIN_CHUNK ? n_tiles - c0 : FIN_CHUNK);
        for (int i = tid; i < n; i += FIN_T) {
            const float2 v = p[c0 + i];
            sv[i] = v.y * expf(beta * (v.x - m));  // (an empty tile is (-inf, 0): 0 * 0)
        }
        __syncthreads();
        if (tid == 0)
            for (int i = 0; i < n; ++i) L += sv[i];
        __syncthreads();
    }
    if (tid == 0) {
        out_max[q] = m;
        out_log_rel[q] = logf(L);
    }
}

}  // namespace

int64_t scan_nq_pad(int64_t nq) { return nq <= 64 ? 64 : (nq + 127) / 128 * 128; }
int64_t scan_tiles(int64_t ntotal) { return (ntotal + SCAN_BM - 1) / SCAN_BM; }

hipError_t launch_scan_stage(const ScanInputs& s, int64_t q_first, int64_t nq, int64_t nq_pad, hipStream_t stream) {
    const int64_t n = nq_pad * (s.dim_pad / 8);
    hipLaunchKernelGGL(scan_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, s.q_src, s.q_dtype, q_first, nq, s.dim,
                       (uint16_t*)s.q_stage, s.store_dtype, nq_pad, s.dim_pad);
    return hipGetLastError();
}

FilterExtra scan_filter_extra(const ScanInputs& s, int64_t q_first) {
    FilterExtra ex;
    if (s.q_label != nullptr) {
        ex.row_label = s.row_label;
        ex.q_label = s.q_label + (size_t)q_first * s.n_qlab;
        ex.n_qlab = s.n_qlab;
    }
    return ex;
}

hipError_t launch_log_partition(const PartitionArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = scan_nq_pad(nq);
    const int64_t n_tiles = scan_tiles(a.ntotal);
    if (a.dim_pad % 64 != 0 || a.dim_pad <= 0 || a.ntotal < 0 || a.ntotal >= (1ll << 31) - 512 || nq > (1 << 20)) return hipErrorInvalidValue;
    if (n_tiles > 0) {
        if (hipError_t e = launch_scan_stage(a, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
        const FilterExtra ex = scan_filter_extra(a, q_first);
        const hipError_t e = scan_dispatch(a.store_dtype, nq_pad, ex.row_label != nullptr, [&](auto dt, auto bn, auto wn, auto subset) {
            const int n_qtiles = (int)(nq_pad / bn.value);
            return scan_launch<bn.value, wn.value>(partition_scan_kernel<dt.value, bn.value, wn.value, subset.value>, scan_grid((int)n_tiles, n_qtiles), stream,
                                                   (const uint16_t*)a.store, (const uint16_t*)a.q_stage, (int)a.dim_pad, (int)a.ntotal, (int)n_tiles,
                                                   n_qtiles, (int)nq, a.beta, (float2*)a.part, ex);
        });
        if (e != hipSuccess) return e;
    }
    return launch_partition_finish(a, q_first, nq, stream);
}

hipError_t launch_partition_finish(const PartitionArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    hipLaunchKernelGGL(partition_finish_kernel, dim3((unsigned)nq), dim3(FIN_T), 0, stream, (const float2*)a.part, scan_tiles(a.ntotal), a.beta,
                       a.out_max + q_first, a.out_log_rel + q_first);
    return hipGetLastError();
}

}  // namespace vodhip
