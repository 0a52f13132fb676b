// The posterior's gradient in the STORED ROWS (vodhip_index_posterior_key_gradient, include/vodhip.h H2k):
//   out[z, d] = beta * sum_{queries q < nq, z eligible for q} p(z | q) c_qz q~[q, d],   c_qz = a_q + (u_qz - ubar_q),
//   u_qz = sum_c G[q, c] v~[z, c],   ubar_q = sum_c G[q, c] y[q, c],   p(z | q) = exp(beta <q~, x~_z> - log Z_beta(q)):
// the gradient of sum_q a_q log Z_q + sum_qc G_qc y_qc in x~, [ntotal, dim].  It is the adjoint's geometry (kernels_readout_adjoint.hip:
// a workgroup owns 64 stored rows and walks the batch) with the read-out gradient's weight (kernels_readout_grad.hip: signed, centred
// BEFORE the one rounding).  The weight depends on the row through u, so it is not of the form P^T W and no sequence of adjoint calls
// gives it; the log Z term alone (G absent) is P^T (a q~) and the adjoint would give it in ceil(dim / 256) calls.
//   maxima   the largest finite |G| and |a| over the LIVE queries (finite max_score and log_rel) of the WHOLE batch (a maximum is the
//            same in every order: atomicMax on the bit patterns).  A dead query enters no scale: behind a batch it changes no bit.
//   query    one workgroup per query of the whole batch.  k = the exponent of max |G| (of max |a| when no G is given or G is all zero):
//            ONE power of two for the batch.  A per-query scale is not possible here: the contraction of the second product runs over
//            the queries inside the MFMA, so a per-query factor could not be undone behind it; a batch-wide one can.  G^ =
//            round16(G 2^-k) (exact scale, one rounding), a' = a 2^-k in float32 (never rounded to 16 bits), ubar_q = float32(sum_c g^ y)
//            summed in double in increasing c over the columns with g^ != 0 (readout_grad_stage_kernel's), B_q = |a'_q| + sum_c |g^_qc|
//            vmax_c + |ubar_q| >= |c_qz| for every row, vmax the cached readout_grad_vmax.  Per query (a', ubar, flag): flag 1 = the zero
//            row (B_q = 0, or a dead query: it weighs +0), flag 2 = a non-finite a_q, G[q, :], used y[q, c] or B_q.  max_q B_q by atomicMax.
//   scale    R = 2^e, the power of two above max_q B_q (1 + 2^-10): every |c_qz| / R <= 1 and no fp16 weight overflows.  In fp16 a query
//            whose gradient is far below the batch's largest therefore loses RELATIVE precision (its weights sit low in the format's
//            range, scaled by 2^15 they stay normal down to 2^-29 of R) but not absolute precision: the bound carries a floor in units
//            of 2^k R.
//   stage    per slice of <= 1024 queries: launch_scan_stage stages the queries as every scan does; G^ of the slice -> g_stage
//            [nq_pad][c_pad], rows of padding and of flagged queries zero.
//   scan     one workgroup per (64 consecutive stored rows, chunk of KG_NSL 64-column slices of dim_pad), the row tiles padded to the 8
//            XCDs.  Per 256-query tile t of the slice, in increasing t:
//            1. scan_k_loop on (staged queries, the 64 rows): the scores, the same bits as every scan;
//            2. TABLE: scan_k_loop on (g_stage tile, the 64 table rows) with dim_pad = c_pad: u in the scores' accumulator layout (a
//               template parameter: the log Z-only build has no second loop, no u registers);
//            3. the adjoint's eligibility mask: rows >= ntotal, NaN scores, subset labels;
//            4. e = expf(min(0, beta (s - max_q)) - log_rel_q), W' = round16(e * ((a'_q + (u - ubar_q)) * (1 / R))), +0 by a select AFTER
//               the product (a non-finite u of an ineligible row, a dead or flagged query spread nothing), packed as the B fragments
//               (fp16: scaled by 2^15 before the rounding);
//            5. Y[d, z] += q~[q, d] W'[q, z]: the chunk's 64-column slices of the staged query tile, streamed by LDS-DMA into the
//               swizzled image and read transposed, exactly as the adjoint reads w_stage.
//            After the last tile the waves add as ((w0 + w1) + w2) + w3 and out[z, d] = ldexp(beta * Y, k + e) is stored for z < ntotal,
//            d < dim (added to what is there for a later slice, or with `accumulate`); NaN everywhere when any query carries flag 2.
// ONE order per (row, column), fixed by the queries' positions in the batch alone; no atomics in the scan, no partials, no fold.  An
// element depends on its row, the queries, their words and the batch-wide (k, e) alone.
// CHUNK WIDTH.  log Z only: 4 slices (256 AGPRs of accumulators beside the 64 score registers, as the adjoint).  With a table the u
// accumulator is live beside the scores: 3 slices, as kernels_readout_grad.hip found (`make check-key-grad`: no scratch anywhere).
// NOT BUILT: the form in which each wave owns a column range and the scores are computed once per tile - K-loop steps (K + K) per
// tile against this design's chunks * (K + slices) (K = dim_pad / 64 steps; chunks = ceil(K / slices)); it needs the weights exchanged
// through the LDS between the waves and half-tiles of queries to fit 160 KB.
// The slice-image geometry, the fp16 weight scale, acc_scale and the host dispatch are scan_contract.h's, which also records why the
// second product itself stays spelled out in this file.
#include "scan_contract.h"

#include "../../include/vodhip.h"

#include <algorithm>

namespace vodhip {

namespace {

constexpr int KG_BQ = SCAN_BM;                  // queries of a tile: the streamed operand of the K loops
constexpr int KG_BZ = 64;                       // stored rows of a workgroup: the resident operand
#ifndef VODHIP_KEY_GRAD_SLICES_LOGZ
#define VODHIP_KEY_GRAD_SLICES_LOGZ 4
#endif
#ifndef VODHIP_KEY_GRAD_SLICES_TABLE
#define VODHIP_KEY_GRAD_SLICES_TABLE 3
#endif
constexpr int KG_NSL_LOGZ = VODHIP_KEY_GRAD_SLICES_LOGZ;    // 64-column slices of a full chunk, a only
constexpr int KG_NSL_TABLE = VODHIP_KEY_GRAD_SLICES_TABLE;  // with a table term
constexpr int KG_A_BYTES = CT_SLICE_BYTES;      // one slice image
constexpr int KG_IMG = CT_IMG;                  // the slices of the second product; >= the K loop's ring
constexpr int KG_LDS = KG_IMG + KG_BQ * (int)sizeof(float4);  // + the tile's (max_score, log_rel, a', ubar) words
static_assert(KG_NSL_LOGZ == 3 || KG_NSL_LOGZ == 4, "3 or 4 slices");
static_assert(KG_NSL_TABLE == 3 || KG_NSL_TABLE == 4, "3 or 4 slices");
static_assert(KG_BZ == CT_BN, "the geometry of scan_contract.h");


// what the staging leaves per query of the batch
struct KgQuery {
    float a;     // a' = a 2^-k
    float ubar;  // sum_c g^ y
    int flag;    // 0 = scan, 1 = the zero row, 2 = the NaN row
    int pad;
};
// the batch-wide words
struct KgScales {
    unsigned int gmax, amax, bmax;  // bit patterns of the largest finite |G|, |a| and of max_q B_q (non-negative floats order as their bits)
    int nan;                        // any query with flag 2, or R beyond float32
    int k, e;                       // G^ = G 2^-k; R = 2^e
    float rinv;                     // 1 / R
    int shift;                      // k + e
};

constexpr int KGS_T = 256;
static_assert(KGS_T >= VODHIP_READOUT_MAX_COLS, "one thread per value column");

__device__ __forceinline__ bool kg_live(const float* max_score, const float* log_rel, int64_t q) {
    const float inf = __builtin_inff(), m = max_score[q], r = log_rel[q];
    return m > -inf && m < inf && r > -inf && r < inf;
}

__device__ __forceinline__ int kg_batch_k(const KgScales* sc) {
    const float gm = __uint_as_float(sc->gmax), am = __uint_as_float(sc->amax);
    return gm > 0.f ? ilogbf(gm) : (am > 0.f ? ilogbf(am) : 0);
}

// ---- the largest finite |G| and |a| of the batch
__global__ __launch_bounds__(KGS_T)
void key_grad_max_kernel(const float* __restrict__ a, const float* __restrict__ g, const float* __restrict__ max_score, const float* __restrict__ log_rel,
                         int64_t nq, int n_cols, KgScales* __restrict__ sc) {
    __shared__ float red[2][KGS_T];
    const int tid = threadIdx.x;
    const float inf = __builtin_inff();
    float mg = 0.f, ma = 0.f;
    const int64_t step = (int64_t)gridDim.x * KGS_T, first = (int64_t)blockIdx.x * KGS_T + tid;
    if (g)
        for (int64_t i = first; i < nq * n_cols; i += step) {
            const float v = fabsf(g[i]);
            if (v < inf && kg_live(max_score, log_rel, i / n_cols)) mg = fmaxf(mg, v);  // (NaN and infinity fail the comparison)
        }
    if (a)
        for (int64_t i = first; i < nq; i += step) {
            const float v = fabsf(a[i]);
            if (v < inf && kg_live(max_score, log_rel, i)) ma = fmaxf(ma, v);
        }
    red[0][tid] = mg;
    red[1][tid] = ma;
    __syncthreads();
    for (int s = KGS_T / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] = fmaxf(red[0][tid], red[0][tid + s]);
            red[1][tid] = fmaxf(red[1][tid], red[1][tid + s]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (red[0][0] > 0.f) atomicMax(&sc->gmax, __float_as_uint(red[0][0]));
        if (red[1][0] > 0.f) atomicMax(&sc->amax, __float_as_uint(red[1][0]));
    }
}

// ---- one workgroup per query of the batch: (a', ubar, flag) and the batch's max B
__global__ __launch_bounds__(KGS_T)
void key_grad_query_kernel(const float* __restrict__ a, const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ vmax,
                           const float* __restrict__ max_score, const float* __restrict__ log_rel, int n_cols, int store_dtype, KgScales* __restrict__ sc,
                           KgQuery* __restrict__ aux) {
    __shared__ float gh[KGS_T];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float inf = __builtin_inff();
    const int k = kg_batch_k(sc);
    const float v = (g && tid < n_cols) ? g[(size_t)q * n_cols + tid] : 0.f;
    const int bad_g = __syncthreads_or(!(fabsf(v) < inf));
    float r = 0.f;
    if (!bad_g) (void)store_bits(ldexpf(v, -k), store_dtype, &r);  // |g 2^-k| < 2: exact scale, one rounding
    gh[tid] = r;
    __syncthreads();
    if (tid == 0) {
        const float aq = a ? a[q] : 0.f;
        const float as = ldexpf(aq, -k);
        KgQuery w = {0.f, 0.f, 2, 0};
        if (!bad_g && fabsf(aq) < inf && !kg_live(max_score, log_rel, q)) {
            w.flag = 1;  // a dead query: finite gradients that weigh nothing and enter no scale
        } else if (!bad_g && fabsf(aq) < inf) {
            double ub = 0.0, sa = 0.0;
            if (g)
                for (int c = 0; c < n_cols; ++c) {
                    if (gh[c] != 0.f) {
                        ub += (double)gh[c] * (double)y[(size_t)q * n_cols + c];
                        sa += (double)fabsf(gh[c]) * (double)vmax[c];
                    }
                }
            const float ubar = (float)ub;
            const double B = (double)fabsf(as) + sa + fabs((double)ubar);
            float bf = (float)B;
            if ((double)bf < B) bf = nextafterf(bf, inf);  // (rounded up: the maximum stays a bound)
            if (B == 0.0) {
                w.flag = 1;  // a', every u_z and ubar are exactly 0
            } else if (bf < inf) {  // (false for a NaN: a non-finite y under a non-zero g^, or a' beyond float32)
                w.a = as;
                w.ubar = ubar;
                w.flag = 0;
                atomicMax(&sc->bmax, __float_as_uint(bf));
            }
        }
        if (w.flag == 2) atomicOr(&sc->nan, 1);
        aux[q] = w;
    }
}

// ---- R = 2^e above max_q B_q (1 + 2^-10)
__global__ void key_grad_scale_kernel(KgScales* __restrict__ sc) {
    const int k = kg_batch_k(sc);
    const double A = (double)__uint_as_float(sc->bmax) * (1.0 + 1.0 / 1024.0);
    int e = 0;
    if (A > 0.0) {
        (void)frexp(A, &e);  // A = f 2^e, 1/2 <= f < 1: R = 2^e > A
        e = max(e, -120);
        if (e > 120) {
            sc->nan = 1;
            e = 0;
        }
    }
    sc->k = k;
    sc->e = e;
    sc->rinv = ldexpf(1.f, -e);
    sc->shift = k + e;
}

// ---- G rows [q_first, q_first + nq) -> g_stage [nq_pad][c_pad]: one thread per element
__global__ __launch_bounds__(KGS_T)
void key_grad_gstage_kernel(const float* __restrict__ g, const KgQuery* __restrict__ aux, const KgScales* __restrict__ sc, int64_t nq, int64_t nq_pad, int n_cols,
                            int c_pad, int store_dtype, uint16_t* __restrict__ g_stage) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq_pad * c_pad) return;
    const int64_t q = i / c_pad;
    const int c = (int)(i % c_pad);
    uint16_t bits = 0;
    if (q < nq && c < n_cols && aux[q].flag == 0) {
        float r;
        bits = store_bits(ldexpf(g[q * n_cols + c], -sc->k), store_dtype, &r);
    }
    g_stage[i] = bits;
}

// Qs: the staged queries [n_qtiles * 256][dim_pad]; X: the store; V: the value table [>= round_up(ntotal, 256)][c_pad]; Gs: g_stage
// [n_qtiles * 256][c_pad]; aux, max_score, log_rel: the nq words of the slice; out [ntotal][dim].  The launch covers n_dchunks chunks of
// NSL slices each from column col_first on.  ex: the subset filter of the slice
template <int DT, bool SUBSET, bool TABLE, int NSL>
__global__ __launch_bounds__(scan_threads(1), 1)
void key_grad_kernel(const uint16_t* __restrict__ Qs, const uint16_t* __restrict__ X, const uint16_t* __restrict__ V, const uint16_t* __restrict__ Gs,
                     const KgQuery* __restrict__ aux, const KgScales* __restrict__ sc, const float* __restrict__ max_score, const float* __restrict__ log_rel,
                     int dim_pad, int c_pad, int dim, int ntotal, int n_rtiles, int n_qtiles, int n_dchunks, int col_first, int nq, float beta, int add,
                     float* __restrict__ out, FilterExtra ex) {
    constexpr int BM = KG_BQ, WM = SCAN_WM, BN = KG_BZ;
    constexpr int TM = BM / WM;
    constexpr int MI = TM / 32, NJ = BN / 32;
    constexpr int ROW_BYTES = SCAN_BK * 2;
    constexpr int RPI = 8;
    constexpr int A_BYTES = KG_A_BYTES;
    constexpr int NA = BM / RPI / WM;
    constexpr int NYB = 2 * NSL;      // 32-column blocks of the accumulator
    constexpr int C_W = 64 * NSL;     // columns of this launch's chunks
    constexpr int QG = TABLE ? 4 : 8;  // queries whose words a lane holds at a time: four words each with a table, three without
    static_assert(MI == 2 && NJ == 2, "a lane holds 2 x 16 queries per row column");
    static_assert(NYB * NJ * 16 * 64 * (int)sizeof(float) <= KG_IMG, "the wave reduction fits the LDS");
    static_assert(scan_threads(1) == KG_BQ, "one thread stages one query's words");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    // the words of the tile's 256 queries.  TABLE: float4 (max_score, log_rel, a', ubar), one read; else float2 (max_score, log_rel) and,
    // behind them, a' / R at the same 8-byte stride (one address serves both reads): a lane holds eight queries' words at a time, and a
    // fourth word each is a register too many at 4 slices
    float4* words4 = reinterpret_cast<float4*>(smem + KG_IMG);
    float2* words2 = reinterpret_cast<float2*>(smem + KG_IMG);
    float2* wordc = words2 + KG_BQ;

    // XCD-aware order: consecutive row tiles on the 8 XCDs, the chunks of one row tile back to back on one XCD
    const int bid = blockIdx.x;
    const int xcd = bid & 7, jj = bid >> 3;
    const int col0 = col_first + (jj % n_dchunks) * C_W;
    const int rt = (jj / n_dchunks) * 8 + xcd;
    if (rt >= n_rtiles) return;  // (uniform over the workgroup, before any barrier)
    const int z0 = rt * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave;

    // per-lane LDS-DMA sources of the query slices (tile 0, slice 0 of the chunk): formed again in every tile (kernels_readout_grad.hip)
    const int st_row = lane >> 3, st_slot = lane & 7;
    static_assert(NA % 2 == 0 && (NA * RPI) % 16 == 0, "the swizzle of a lane's rows has period 2 in u");
    auto q_off = [&](int t) {
        const int r = (wave * NA + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        return (unsigned)(r * dim_pad + c * 8) * 2u + (unsigned)col0 * 2u;
    };

    const int fr = lane & 31, fh = lane >> 5;

    // transposed reads of a slice image: posterior_scan_kernel's
    const int tq = (lane & 15) >> 2;
    const int t_row = wm * TM + 4 * fh + tq;                       // + 32 i + 16 s + 8 e
    const int t_chunk = 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1);  // + 4 mb
    const int t_sub = 8 * (lane & 1);
    const int t_swz = 2 * fh + (tq >> 1);                          // ((row >> 1) & 7) = 4 e + t_swz

    const float inf = __builtin_inff();

    f32x16 yacc[NYB][NJ];
#pragma unroll
    for (int b = 0; b < NYB; ++b)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[b][j][r] = 0.f;

    for (int qt = 0; qt < n_qtiles; ++qt) {
        const int q0 = qt * BM;
        const char* q_tile = (const char*)Qs + (size_t)q0 * dim_pad * 2;

        __syncthreads();  // the previous tile's transposed reads and word reads are done: the ring and the words may be written
        {
            const int q = q0 + tid;
            float2 w = make_float2(0.f, inf), wc = make_float2(0.f, 0.f);  // weighs +0: past nq, no finite log Z, flag 1, flag 2
            if (q < nq) {
                const float mq = max_score[q], lq = log_rel[q];
                const KgQuery x = aux[q];
                if (x.flag == 0 && mq > -inf && mq < inf && lq > -inf && lq < inf) {
                    w = make_float2(mq, lq);
                    wc = make_float2(TABLE ? x.a : x.a * sc->rinv, x.ubar);
                }
            }
            if constexpr (TABLE) {
                words4[tid] = make_float4(w.x, w.y, wc.x, wc.y);  // (visible behind the K loop's barriers)
            } else {
                words2[tid] = w;
                wordc[tid] = wc;
            }
        }
        f32x16 acc[MI][NJ];
        scan_k_loop<DT, BN, 1>(Qs + (size_t)q0 * dim_pad, X + (size_t)z0 * dim_pad, dim_pad, smem, acc);

        // (register classes, no instructions: the accumulators stay in AGPRs across the K loops, the scores arrive in VGPRs)
#pragma unroll
        for (int b = 0; b < NYB; ++b)
#pragma unroll
            for (int j = 0; j < NJ; ++j) asm volatile("" : "+a"(yacc[b][j]));
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(acc[i][j]));

        f32x16 uacc[MI][NJ];
        if constexpr (TABLE) {
            __syncthreads();  // every wave has read its last fragments: the ring is written again
            scan_k_loop<DT, BN, 1>(Gs + (size_t)q0 * c_pad, V + (size_t)z0 * c_pad, c_pad, smem, uacc);
#pragma unroll
            for (int b = 0; b < NYB; ++b)
#pragma unroll
                for (int j = 0; j < NJ; ++j) asm volatile("" : "+a"(yacc[b][j]));
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    asm volatile("" : "+v"(acc[i][j]));
                    asm volatile("" : "+v"(uacc[i][j]));
                }
        }

        __syncthreads();  // the LDS becomes the slice images
        {
            const unsigned off[2] = {q_off(0), q_off(1)};
            const unsigned q_pair = (unsigned)(2 * RPI * dim_pad) * 2u;  // between the rows of equal parity
#pragma unroll
            for (int sl = 0; sl < NSL; ++sl)
#pragma unroll
                for (int u = 0; u < NA; ++u)
                    glds16(q_tile + off[u & 1] + ((u >> 1) * q_pair + sl * ROW_BYTES), smem + sl * A_BYTES + (wave * NA + u) * RPI * ROW_BYTES);
        }

        // ---- the eligible (query, row) pairs of the lane: bit 16 i + r of column j = query register r of block i, row z0 + 32 j + fr
        const int qlane = wm * TM + 4 * fh;  // the lane's query of (block 0, register 0) in the tile: scan_lane_row gives the others
        unsigned okm[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int row = z0 + j * 32 + fr;
            unsigned mask = 0u;
            if (row < ntotal) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mask |= (acc[0][j][r] == acc[0][j][r]) ? (1u << r) : 0u;
#pragma unroll
                for (int r = 0; r < 16; ++r) mask |= (acc[1][j][r] == acc[1][j][r]) ? (1u << (16 + r)) : 0u;
            }
            if constexpr (SUBSET) {  // rolled: one label test per pair that is still in; a query past nq has no labels (and weighs +0)
                unsigned m2 = mask;
                while (m2) {
                    const int b = __builtin_ctz(m2);
                    m2 &= m2 - 1;
                    const int q = q0 + scan_lane_row(qlane, b);
                    if (q >= nq || !subset_allows(ex, q, row)) mask &= ~(1u << b);
                }
            }
            okm[j] = mask;
        }
        float rinv = 1.f;
        if constexpr (TABLE) rinv = sc->rinv;

        // ---- weights, packed as the B fragments of the second product
        u32x4 wf[MI][2][NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float w8[NJ][8];
#pragma unroll
                for (int h = 0; h < 8 / QG; ++h) {
                    float2 wd[QG];
                    float ca[QG], cb[QG];  // (a', ubar), or a' / R alone
#pragma unroll
                    for (int e = 0; e < QG; ++e) {
                        const int at = scan_lane_row(qlane, 16 * i + 8 * s + QG * h + e);
                        if constexpr (TABLE) {
                            const float4 w4 = words4[at];
                            wd[e] = make_float2(w4.x, w4.y);
                            ca[e] = w4.z;
                            cb[e] = w4.w;
                        } else {
                            wd[e] = words2[at];
                            ca[e] = wordc[at].x;
                            cb[e] = 0.f;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int e = 0; e < QG; ++e) {
                            const int r = 8 * s + QG * h + e;
                            const float ev = expf(fminf(0.f, beta * (acc[i][j][r] - wd[e].x)) - wd[e].y);
                            // the select AFTER the product.  Without a table a query that weighs +0 has e = +0 and a' / R = +0: no NaN to keep out
                            bool ok = (okm[j] & (1u << (i * 16 + r))) != 0u;
                            float cu;
                            if constexpr (TABLE) {
                                cu = (ca[e] + (uacc[i][j][r] - cb[e])) * rinv;
                                ok = ok && wd[e].y < inf;
                            } else {
                                cu = ca[e];
                            }
                            w8[j][QG * h + e] = ok ? ev * cu : 0.f;
                        }
                    // (QG queries at a time: interleaving all 64 exponentials costs registers)
                    if constexpr (QG < 8) __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    if constexpr (DT == 0) {
                        f16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (_Float16)(w8[j][e] * CT_FP16_SCALE);
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    } else {
                        bf16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (__bf16)w8[j][e];
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }

        wait_vmcnt<0>();
        __syncthreads();  // the slices have landed

        // ---- Y[d, z] += Q^T W': A = the transposed slice (rows of A = store columns d), B = the weights
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int i = 0; i < MI; ++i)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        s16x4 half[2];
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int row = t_row + 32 * i + 16 * s + 8 * e;
                            const int phys = (4 * mb + t_chunk) ^ (4 * e + t_swz);
                            const char* at = smem + sl * A_BYTES + row * ROW_BYTES + (phys << 4) + t_sub;
                            half[e] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VOD_AS3 s16x4*)at);
                        }
                        const s16x8 both = __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7);
                        const u32x4 af = __builtin_bit_cast(u32x4, both);
#pragma unroll
                        for (int j = 0; j < NJ; ++j) yacc[sl * 2 + mb][j] = mfma32<DT>(af, wf[i][s][j], yacc[sl * 2 + mb][j]);
                    }
    }

    // ---- ((w0 + w1) + w2) + w3 through the LDS (kernels_readout.hip), then the workgroup stores its [64 rows][C_W] block
    __syncthreads();
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    float* red = reinterpret_cast<float*>(smem);  // [NYB * NJ * 16][64]: element r of block (b, j) of lane l at ((b NJ + j) 16 + r) 64 + l
    if (wave == 0) {
#pragma unroll
        for (int b = 0; b < NYB; ++b)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x16 v = yacc[b][j];
                asm volatile("" : "+v"(v));  // (one block at a time through 16 vector registers)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((b * NJ + j) * 16 + r) * 64 + lane_e] = v[r];
                __builtin_amdgcn_sched_barrier(0);
            }
    }
    __syncthreads();
#pragma unroll 1
    for (int w = 1; w < WM; ++w) {
        if (wave == w) {
#pragma unroll
            for (int b = 0; b < NYB; ++b)
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    f32x16 v = yacc[b][j];
                    asm volatile("" : "+v"(v));
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int at = ((b * NJ + j) * 16 + r) * 64 + lane_e;
                        red[at] = red[at] + v[r];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        __syncthreads();
    }
    // column c of the chunk, row column `col`: block b = c / 32, lane half (c >> 2) & 1, register (c & 3) + 4 ((c & 31) >> 3) - the C
    // layout of the second product (its rows are the store columns).  The batch's power of two (and the 2^-15 of the fp16 weights) is exact
    const int shift = sc->shift - (DT == 0 ? CT_FP16_SHIFT : 0);
    const bool nan = sc->nan != 0;
    for (int idx = wave * 64 + lane_e; idx < BN * C_W; idx += scan_threads(1)) {  // (wave * 64 + lane_e = tid)
        const int col = idx / C_W, c = idx % C_W;
        const int z = z0 + col, d = col0 + c;
        if (z < ntotal && d < dim) {
            const int r = (c & 3) + 4 * ((c & 31) >> 3);
            const int l = 32 * ((c >> 2) & 1) + (col & 31);
            const float y = red[(((c >> 5) * NJ + (col >> 5)) * 16 + r) * 64 + l];
            const float v = nan ? __builtin_nanf("") : ldexpf(beta * y, shift);
            float* at = out + (size_t)z * dim + d;
            *at = add ? *at + v : v;
        }
    }
}

// the full chunks in one launch, the last narrower chunk (if any) in a second one
template <int DT, bool SUBSET, bool TABLE>
hipError_t launch_kg_scan(const KeyGradArgs& a, int64_t q_first, int64_t nq, int add, const FilterExtra& ex, hipStream_t stream) {
    constexpr int NFULL = TABLE ? KG_NSL_TABLE : KG_NSL_LOGZ;
    const int n_rtiles = (int)((a.p.ntotal + KG_BZ - 1) / KG_BZ);
    const int n_qtiles = (int)((nq + KG_BQ - 1) / KG_BQ);
    return chunks_dispatch<NFULL>((int)(a.p.dim_pad / 64), [&](auto nsl, int first_chunk, int n_dchunks) {
        return scan_launch_lds<1>(key_grad_kernel<DT, SUBSET, TABLE, nsl.value>, scan_grid(n_rtiles, n_dchunks), KG_LDS, stream, (const uint16_t*)a.p.q_stage,
                                  (const uint16_t*)a.p.store, (const uint16_t*)a.values, (const uint16_t*)a.g_stage, (const KgQuery*)a.aux + q_first,
                                  (const KgScales*)a.scales, a.p.out_max + q_first, a.p.out_log_rel + q_first, (int)a.p.dim_pad, a.c_pad, (int)a.p.dim, (int)a.p.ntotal,
                                  n_rtiles, n_qtiles, n_dchunks, first_chunk * NFULL * 64, (int)nq, a.p.beta, add, a.out, ex);
    });
}

bool key_grad_args_ok(const KeyGradArgs& a) {
    if (!scan_store_ok(a.p) || a.p.dim < 1 || a.p.dim > a.p.dim_pad) return false;
    if (!a.a && !a.g) return false;
    if (a.g) {
        if (!readout_cols_ok(a.c_pad, a.n_cols)) return false;
        if (!a.y || !a.vmax || !a.values || !a.g_stage) return false;
    }
    return a.aux && a.scales && a.out;
}

}  // namespace

size_t key_grad_aux_bytes() { return sizeof(KgQuery); }
size_t key_grad_scales_bytes() { return sizeof(KgScales); }
int64_t key_grad_nq_pad(int64_t nq) { return (nq + KG_BQ - 1) / KG_BQ * KG_BQ; }

hipError_t launch_key_grad_scales(const KeyGradArgs& a, int64_t nq, hipStream_t stream) {
    if (!key_grad_args_ok(a) || nq <= 0 || nq > 0x7fffffffll) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(a.scales, 0, sizeof(KgScales), stream); e != hipSuccess) return e;
    const int64_t n = nq * (a.g ? a.n_cols : 1);
    const unsigned grid = (unsigned)std::min<int64_t>((n + KGS_T * 8 - 1) / (KGS_T * 8), 512);
    hipLaunchKernelGGL(key_grad_max_kernel, dim3(grid), dim3(KGS_T), 0, stream, a.a, a.g, a.p.out_max, a.p.out_log_rel, nq, a.n_cols, (KgScales*)a.scales);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(key_grad_query_kernel, dim3((unsigned)nq), dim3(KGS_T), 0, stream, a.a, a.g, a.y, a.vmax, a.p.out_max, a.p.out_log_rel, a.n_cols, a.p.store_dtype,
                       (KgScales*)a.scales, (KgQuery*)a.aux);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(key_grad_scale_kernel, dim3(1), dim3(1), 0, stream, (KgScales*)a.scales);
    return hipGetLastError();
}

hipError_t launch_posterior_key_gradient(const KeyGradArgs& a, int64_t q_first, int64_t nq, int add, hipStream_t stream) {
    if (nq <= 0 || a.p.ntotal == 0) return hipSuccess;
    if (!key_grad_args_ok(a) || nq > (1 << 20)) return hipErrorInvalidValue;
    const int64_t nq_pad = key_grad_nq_pad(nq);
    if (hipError_t e = launch_scan_stage(a.p, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
    if (a.g) {
        const int64_t n = nq_pad * a.c_pad;
        hipLaunchKernelGGL(key_grad_gstage_kernel, dim3((unsigned)((n + KGS_T - 1) / KGS_T)), dim3(KGS_T), 0, stream, a.g + (size_t)q_first * a.n_cols,
                           (const KgQuery*)a.aux + q_first, (const KgScales*)a.scales, nq, nq_pad, a.n_cols, a.c_pad, a.p.store_dtype, (uint16_t*)a.g_stage);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    const FilterExtra ex = scan_filter_extra(a.p, q_first);
    return contract_dispatch(a.p.store_dtype, ex.row_label != nullptr, [&](auto dt, auto subset) {
        return a.g ? launch_kg_scan<dt.value, subset.value, true>(a, q_first, nq, add, ex, stream) : launch_kg_scan<dt.value, subset.value, false>(a, q_first, nq, add, ex, stream);
    });
}

}  // namespace vodhip
