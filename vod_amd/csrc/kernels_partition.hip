// The exact softmax normaliser of the retriever over the WHOLE store (vodhip_index_log_partition, include/vodhip.h H2p):
//   log Z_beta(q) = log sum_{rows z < ntotal, eligible} exp(beta <q~, x~_z>) = beta * max_score + log_rel,
//   max_score = max_z <q~, x~_z>,  log_rel = log sum_z exp(beta (<q~, x~_z> - max_score)) >= 0.
// Three kernels:
//   stage    queries -> [nq_pad][dim_pad] of the store dtype, rounded as a search rounds them (store_bits: saturating), zero padded
//   scan     the K loop of mips_filter_kernel (LDS-DMA with the source-side XOR swizzle, 3-slot ring, v_mfma_f32_32x32x16 with the
//            corpus as A and the queries as B: a lane's accumulator column is ONE query, its registers are corpus rows) over a
//            256-row corpus tile x 64 | 128 queries; the epilogue replaces the top-k filter with a max-stabilised sum of exponentials
//            and writes ONE partial (m, l) per (tile, query): m = the tile's maximum, l = sum exp(beta (s - m))
//   finish   folds a query's partials into (max_score, log_rel)
// A row counts when row < ntotal (rows past it are zero or stale, tile padding reaches past the capacity), its score is not NaN (a
// search leaves NaN out too) and the query's subset labels allow it (subset_allows, mips_common.h).
//
// ONE summation order per query, fixed by ntotal (and dim_pad, the length of the K loop) alone - not by nq, by the other queries of the
// batch, by the query tile width or by the grid:
//   score   the MFMA's own order over the dim_pad / 16 k-steps, the same for every column of the B operand;
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
#include "mips_common.h"

#include <type_traits>

namespace vodhip {

namespace {

constexpr int PT_BM = 256;     // corpus rows of a tile = rows of one partial
constexpr int PT_WM = 4;       // row waves
constexpr int PT_NSTAGE = 3;   // LDS ring depth

__global__ void __launch_bounds__(256) partition_stage_kernel(const void* __restrict__ q_src, int q_dtype, int64_t q_first, int64_t nq, int64_t dim,
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
__global__ __launch_bounds__(PT_WM* WN * 64, 1)
void partition_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles,
                           int nq, float beta, float2* __restrict__ part, FilterExtra ex) {
    constexpr int BM = PT_BM, WM = PT_WM, NSTAGE = PT_NSTAGE;
    constexpr int BK = 64;
    constexpr int NWAVES = WM * WN;
    constexpr int TM = BM / WM, TN = BN / WN;
    constexpr int MI = TM / 32, NJ = TN / 32;
    constexpr int ROW_BYTES = BK * 2;
    constexpr int RPI = 8;
    constexpr int KK = BK / 16;
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES;
    constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int NA = BM / RPI / NWAVES;
    constexpr int NB = BN / RPI / NWAVES;
    constexpr int G = NA + NB;
    static_assert(BM % (RPI * NWAVES) == 0 && BN % (RPI * NWAVES) == 0, "tile/wave mismatch");
    static_assert(MI == 2, "the eligibility mask holds 2 x 16 rows per lane");
    static_assert(2 * WM * BN * (int)sizeof(float) <= STAGE_BYTES, "the reduction arrays reuse the first ring slot");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    // XCD-aware tile order (as mips_filter_kernel): the n_qtiles workgroups that re-read one corpus tile land on one XCD back to back
    const int bid = blockIdx.x;
    const int xcd = bid & 7, jj = bid >> 3;
    const int qt = jj % n_qtiles;
    const int xt = (jj / n_qtiles) * 8 + xcd;
    if (xt >= n_xtiles) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int x0 = xt * BM;
    const int q0 = qt * BN;

    // per-lane LDS-DMA sources: lane -> (row = base + lane / 8, 16-B slot = lane % 8); slot s of row r holds chunk s ^ ((r >> 1) & 7)
    const int st_row = lane >> 3, st_slot = lane & 7;
    const char* a_src[NA];
    const char* b_src[NB];
#pragma unroll
    for (int t = 0; t < NA; ++t) {
        const int r = (wave * NA + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        a_src[t] = (const char*)X + ((size_t)(x0 + r) * dim_pad + c * 8) * 2;
    }
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int r = (wave * NB + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        b_src[t] = (const char*)Q + ((size_t)(q0 + r) * dim_pad + c * 8) * 2;
    }
    auto stage_part = [&](int ks, int p, int nparts) {
        char* sa = smem + (ks % NSTAGE) * STAGE_BYTES;
        char* sb = sa + A_BYTES;
        const int kbyte = ks * ROW_BYTES;
#pragma unroll
        for (int u = 0; u < G; ++u) {
            if ((u * nparts) / G != p) continue;
            if (u < NA)
                glds16(a_src[u] + kbyte, sa + (wave * NA + u) * RPI * ROW_BYTES);
            else
                glds16(b_src[u - NA] + kbyte, sb + (wave * NB + (u - NA)) * RPI * ROW_BYTES);
        }
    };

    const int fr = lane & 31, fh = lane >> 5;
    const int swz = (fr >> 1) & 7;
    const int a_row_off = (wm * TM + fr) * ROW_BYTES;
    const int b_row_off = A_BYTES + (wn * TN + fr) * ROW_BYTES;

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = dim_pad / BK;
#pragma unroll
    for (int s = 0; s < NSTAGE - 1; ++s)
        if (s < nk) stage_part(s, 0, 1);

    auto load_frags = [&](const char* base, int kk, u32x4(&af)[MI], u32x4(&bf)[NJ]) {
        const int slot_off = ((2 * kk + fh) ^ swz) << 4;
#pragma unroll
        for (int i = 0; i < MI; ++i) af[i] = *(const u32x4*)(base + a_row_off + i * 32 * ROW_BYTES + slot_off);
#pragma unroll
        for (int j = 0; j < NJ; ++j) bf[j] = *(const u32x4*)(base + b_row_off + j * 32 * ROW_BYTES + slot_off);
    };
    auto mfma_group = [&](u32x4(&af)[MI], u32x4(&bf)[NJ]) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = mfma32<DT>(af[i], bf[j], acc[i][j]);
    };
    auto kslice = [&](int t, auto pre_tag) {
        constexpr bool PRE = decltype(pre_tag)::value;
        const char* base = smem + (t % NSTAGE) * STAGE_BYTES;
        const int ks = t + NSTAGE - 1;
        u32x4 af0[MI], bf0[NJ], af1[MI], bf1[NJ];
        load_frags(base, 0, af0, bf0);
        if constexpr (PRE) stage_part(ks, 0, KK);
        load_frags(base, 1, af1, bf1);
        mfma_group(af0, bf0);
        if constexpr (PRE) stage_part(ks, 1, KK);
        load_frags(base, 2, af0, bf0);
        mfma_group(af1, bf1);
        if constexpr (PRE) stage_part(ks, 2, KK);
        load_frags(base, 3, af1, bf1);
        mfma_group(af0, bf0);
        if constexpr (PRE) stage_part(ks, 3, KK);
        mfma_group(af1, bf1);
    };
    int t = 0;
    for (; t + NSTAGE - 1 < nk; ++t) {
        wait_vmcnt<(NSTAGE - 2) * G>();
        __builtin_amdgcn_s_barrier();
        kslice(t, std::true_type{});
    }
    for (; t < nk; ++t) {  // tail: the ring drains
        if (nk - 1 - t >= 1) wait_vmcnt<G>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        kslice(t, std::false_type{});
    }

    // ---- epilogue.  C layout: col = lane & 31 (query), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
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
        unsigned mask = 0u;
        if (q < nq) {
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = rlane + i * 32 + (r & 3) + 8 * (r >> 2);
                    const float s = acc[i][j][r];
                    mask |= (row < ntotal && s == s) ? (1u << (i * 16 + r)) : 0u;
                }
            if constexpr (SUBSET) {  // rolled: one label test per row that is still in
                unsigned m2 = mask;
                while (m2) {
                    const int b = __builtin_ctz(m2);
                    m2 &= m2 - 1;
                    const int row = rlane + (b >> 4) * 32 + (b & 3) + 8 * ((b & 15) >> 2);
                    if (!subset_allows(ex, q, row)) mask &= ~(1u << b);
                }
            }
        }
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

template <int DT, int BN, int WN, bool SUBSET>
hipError_t launch_scan(const PartitionArgs& a, int64_t nq, int64_t nq_pad, int n_tiles, const FilterExtra& ex, hipStream_t stream) {
    const int n_qtiles = (int)(nq_pad / BN);
    const int64_t grid = (int64_t)((n_tiles + 7) / 8) * 8 * n_qtiles;
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    constexpr int threads = PT_WM * WN * 64;
    constexpr size_t lds = (size_t)PT_NSTAGE * (PT_BM + BN) * 128;
    auto kern = partition_scan_kernel<DT, BN, WN, SUBSET>;
    if (hipError_t e = allow_dynamic_lds((const void*)kern, (int)lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(threads), lds, stream, (const uint16_t*)a.store, (const uint16_t*)a.q_stage, (int)a.dim_pad,
                       (int)a.ntotal, n_tiles, n_qtiles, (int)nq, a.beta, (float2*)a.part, ex);
    return hipGetLastError();
}

template <int DT>
hipError_t launch_scan_dt(const PartitionArgs& a, int64_t nq, int64_t nq_pad, int n_tiles, const FilterExtra& ex, hipStream_t stream) {
    const bool subset = ex.row_label != nullptr;
    if (nq_pad == 64)
        return subset ? launch_scan<DT, 64, 1, true>(a, nq, nq_pad, n_tiles, ex, stream) : launch_scan<DT, 64, 1, false>(a, nq, nq_pad, n_tiles, ex, stream);
    return subset ? launch_scan<DT, 128, 2, true>(a, nq, nq_pad, n_tiles, ex, stream) : launch_scan<DT, 128, 2, false>(a, nq, nq_pad, n_tiles, ex, stream);
}

}  // namespace

int64_t log_partition_nq_pad(int64_t nq) { return nq <= 64 ? 64 : (nq + 127) / 128 * 128; }
int64_t log_partition_tiles(int64_t ntotal) { return (ntotal + PT_BM - 1) / PT_BM; }

hipError_t launch_log_partition(const PartitionArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = log_partition_nq_pad(nq);
    const int64_t n_tiles = log_partition_tiles(a.ntotal);
    if (a.dim_pad % 64 != 0 || a.dim_pad <= 0 || a.ntotal < 0 || a.ntotal >= (1ll << 31) - 512 || nq > (1 << 20)) return hipErrorInvalidValue;
    if (n_tiles > 0) {
        const int64_t n = nq_pad * (a.dim_pad / 8);
        hipLaunchKernelGGL(partition_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.q_src, a.q_dtype, q_first, nq, a.dim,
                           (uint16_t*)a.q_stage, a.store_dtype, nq_pad, a.dim_pad);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        FilterExtra ex;
        if (a.q_label != nullptr) {
            ex.row_label = a.row_label;
            ex.q_label = a.q_label + (size_t)q_first * a.n_qlab;
            ex.n_qlab = a.n_qlab;
        }
        const hipError_t e = a.store_dtype == 0 ? launch_scan_dt<0>(a, nq, nq_pad, (int)n_tiles, ex, stream)
                                                : launch_scan_dt<1>(a, nq, nq_pad, (int)n_tiles, ex, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(partition_finish_kernel, dim3((unsigned)nq), dim3(FIN_T), 0, stream, (const float2*)a.part, n_tiles, a.beta, a.out_max + q_first,
                       a.out_log_rel + q_first);
    return hipGetLastError();
}

}  // namespace vodhip
