// The adjoint of the posterior read-out, its gradient in the value table (vodhip_index_posterior_adjoint, include/vodhip.h H2a):
//   out[z, c] = sum_{queries q < nq, z eligible for q} p(z | q) W[q, c],   p(z | q) = exp(beta <q~, x~_z> - log Z_beta(q)):
// P^T W, [ntotal, n_cols].  It reduces over the QUERIES per stored row, where every other whole-store scan reduces over the rows per query.
// The forward's (max_score, log_rel) are inputs, so no partition scan runs in front and nothing is rescaled: ONE scan of the store.
//   colmax   one workgroup per weight column: k_c = the exponent of max_q |W[q, c]| over the WHOLE batch (0 for an all-zero column); a NaN
//            or an infinity in the column marks it (ADJ_K_NAN).
//   stage    W^[q, c] = round16(W[q, c] * 2^-k_c) -> w_stage [nq_pad][c_pad] of the store dtype, nq_pad a multiple of 256, rows and columns
//            of padding and marked columns zero.  The scale is exact, the largest entry of a column lands in [1, 2): a loss gradient of
//            1e-6 does not flush in fp16.  A per-column scale survives a contraction over queries, a per-query one would not.
//   scan     one workgroup per 64 consecutive stored rows, the grid padded to the 8 XCDs.  For each 256-query tile t of the slice, in
//            increasing t:
//            1. the K loop of the shared scan core (scan_k_loop, store_scan.h) with its operands exchanged: the staged queries are the
//               streamed 256-row operand, the 64 stored rows the resident column operand.  The loop is symmetric in the two - both are
//               row-major [rows][dim_pad] - and an element is still the one sum over the k-steps in the MFMA's own order.  The accumulator
//               holds stored rows in its lane columns and queries in its registers;
//            2. e = expf(min(0, beta (s - max_score[q])) - log_rel[q]) per (query register, row column); the two words of the tile's 256
//               queries sit in LDS, (0, +inf) for a query past nq or without a finite log Z, so that it weighs +0.  The weight is +0 by a
//               select when the row is >= ntotal, the score is NaN, or the query's subset labels do not allow the row: scan_eligible_mask
//               with rows and queries exchanged;
//            3. P' = round16(e) packed as the B fragments of the second product exactly as readout_scan_kernel packs them (fp16: scaled
//               by 2^15 before the rounding);
//            4. the tile's NSL slices of 64 columns of w_stage, streamed by LDS-DMA into the swizzled 128-byte-row image and read
//               transposed (ds_read_b64_tr_b16): Y[c, z] += W^[q, c] P'[q, z] in float32 - the read-out's steps with w_stage in place of
//               the value table.
//            After the last tile the waves add as ((w0 + w1) + w2) + w3 through the LDS and out[z, c] = 2^k_c Y[c, z] is stored for
//            z < ntotal, c < n_cols (added to what is there for a later slice of the batch, or with `accumulate`).
// ONE order per (row, column), fixed by the query's position in the batch alone - not by ntotal, the row's neighbours or the grid: wave w
// adds queries 256 t + 64 w .. + 63 in k-step order, tile after tile, then the waves, then the slices of 1024 queries in slice order.  A
// row has ONE owning workgroup: no atomics, no partials, no fold.  An element depends on its row, the queries and their words alone.
// The slice-image geometry, the fp16 weight scale, acc_scale and the host dispatch are scan_contract.h's, which also records why the
// second product itself stays spelled out in this file.
#include "scan_contract.h"

#include "../../include/vodhip.h"

#include <algorithm>
#include <climits>

namespace vodhip {

namespace {

constexpr int ADJ_BQ = SCAN_BM;                  // queries of a tile: the streamed operand of the K loop
constexpr int ADJ_BZ = 64;                       // stored rows of a workgroup: the resident operand
constexpr int ADJ_A_BYTES = CT_SLICE_BYTES;      // one slice image
constexpr int ADJ_IMG = CT_IMG;                  // the slices of the second product; >= the K loop's ring
constexpr int ADJ_LDS = ADJ_IMG + ADJ_BQ * (int)sizeof(float2);  // + the tile's (max_score, log_rel) words
constexpr int ADJ_K_NAN = INT_MIN;               // col_k of a column that holds a NaN or an infinity
static_assert(ADJ_BZ == CT_BN, "the geometry of scan_contract.h");


// ---- k_c per weight column over the whole batch: one workgroup per column, the queries strided over its threads (a maximum is the same
// in every order)
constexpr int ADJS_T = 256;
__global__ __launch_bounds__(ADJS_T)
void adjoint_colmax_kernel(const float* __restrict__ w, int64_t nq, int n_cols, int* __restrict__ col_k) {
    __shared__ float red[ADJS_T];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const float inf = __builtin_inff();
    float m = 0.f;
    if (c < n_cols) {
        for (int64_t q = tid; q < nq; q += ADJS_T) {
            const float a = fabsf(w[q * n_cols + c]);
            m = fmaxf(m, a < inf ? a : inf);  // (a NaN counts as an infinity)
        }
    }
    red[tid] = m;
    __syncthreads();
    for (int s = ADJS_T / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    if (tid == 0) col_k[c] = red[0] == inf ? ADJ_K_NAN : (red[0] > 0.f ? ilogbf(red[0]) : 0);
}

// ---- w rows [q_first, q_first + nq) -> w_stage [nq_pad][c_pad]: one thread per element
__global__ __launch_bounds__(ADJS_T)
void adjoint_stage_kernel(const float* __restrict__ w, int64_t nq, int64_t nq_pad, int n_cols, int c_pad, const int* __restrict__ col_k, int store_dtype,
                          uint16_t* __restrict__ w_stage) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq_pad * c_pad) return;
    const int64_t q = i / c_pad;
    const int c = (int)(i % c_pad);
    uint16_t bits = 0;
    if (q < nq && c < n_cols) {
        const int k = col_k[c];
        float r;
        if (k != ADJ_K_NAN) bits = store_bits(ldexpf(w[q * n_cols + c], -k), store_dtype, &r);  // |w 2^-k| < 2: exact scale, one rounding
    }
    w_stage[i] = bits;
}

// Qs: the staged queries [n_qtiles * 256][dim_pad]; X: the store; Ws: w_stage [n_qtiles * 256][c_pad], c_pad = 64 NSL; max_score / log_rel:
// the nq words of the slice; out [ntotal][n_cols].  ex: the subset filter of the slice (its query index is the index in the slice)
template <int DT, bool SUBSET, int NSL>
__global__ __launch_bounds__(scan_threads(1), 1)
void readout_adjoint_kernel(const uint16_t* __restrict__ Qs, const uint16_t* __restrict__ X, const uint16_t* __restrict__ Ws, const int* __restrict__ col_k,
                            const float* __restrict__ max_score, const float* __restrict__ log_rel, int dim_pad, int ntotal, int n_rtiles, int n_qtiles, int nq,
                            int n_cols, float beta, int add, float* __restrict__ out, FilterExtra ex) {
    constexpr int BM = ADJ_BQ, WM = SCAN_WM, BN = ADJ_BZ;
    constexpr int TM = BM / WM;
    constexpr int MI = TM / 32, NJ = BN / 32;
    constexpr int ROW_BYTES = SCAN_BK * 2;
    constexpr int RPI = 8;
    constexpr int A_BYTES = ADJ_A_BYTES;
    constexpr int NA = BM / RPI / WM;
    constexpr int NYB = 2 * NSL;      // 32-column blocks of the accumulator
    constexpr int C_PAD = 64 * NSL;
    static_assert(MI == 2 && NJ == 2, "a lane holds 2 x 16 queries per row column");
    static_assert(NYB * NJ * 16 * 64 * (int)sizeof(float) <= ADJ_IMG, "the wave reduction fits the LDS");
    static_assert(scan_threads(1) == ADJ_BQ, "one thread stages one query's words");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* words = reinterpret_cast<float2*>(smem + ADJ_IMG);  // [256] (max_score, log_rel) of the tile's queries

    // XCD-aware order: consecutive row tiles on the 8 XCDs; every workgroup streams the same staged queries and weights
    const int bid = blockIdx.x;
    const int rt = (bid >> 3) * 8 + (bid & 7);
    if (rt >= n_rtiles) return;  // (uniform over the workgroup, before any barrier)
    const int z0 = rt * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave;

    // per-lane LDS-DMA sources of the weight slices (tile 0): readout_scan_kernel's two offsets
    const int st_row = lane >> 3, st_slot = lane & 7;
    static_assert(NA % 2 == 0 && (NA * RPI) % 16 == 0, "the swizzle of a lane's rows has period 2 in u");
    unsigned v_off[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int r = (wave * NA + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        v_off[t] = (unsigned)(r * C_PAD + c * 8) * 2u;
    }

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
        const char* w_tile = (const char*)Ws + (size_t)q0 * C_PAD * 2;

        __syncthreads();  // the previous tile's transposed reads and word reads are done: the ring and the words may be written
        {
            const int q = q0 + tid;
            float m = 0.f, lr = inf;
            if (q < nq) {
                const float mq = max_score[q], lq = log_rel[q];
                if (mq > -inf && mq < inf && lq > -inf && lq < inf) {
                    m = mq;
                    lr = lq;
                }
            }
            words[tid] = make_float2(m, lr);  // (visible behind the K loop's barriers)
        }
        f32x16 acc[MI][NJ];
        scan_k_loop<DT, BN, 1>(Qs + (size_t)q0 * dim_pad, X + (size_t)z0 * dim_pad, dim_pad, smem, acc);

        // (register classes, no instructions: the accumulators stay in AGPRs across the K loop, the scores arrive in VGPRs)
#pragma unroll
        for (int b = 0; b < NYB; ++b)
#pragma unroll
            for (int j = 0; j < NJ; ++j) asm volatile("" : "+a"(yacc[b][j]));
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(acc[i][j]));
        __syncthreads();  // every wave has read its last fragments: the LDS becomes the slice images
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl)
#pragma unroll
            for (int u = 0; u < NA; ++u)
                glds16(w_tile + v_off[u & 1] + ((u >> 1) * 2 * RPI * C_PAD * 2 + sl * ROW_BYTES), smem + sl * A_BYTES + (wave * NA + u) * RPI * ROW_BYTES);

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

        // ---- weights, packed as the B fragments of the second product
        u32x4 wf[MI][2][NJ];
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float2 wd[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) wd[e] = words[scan_lane_row(qlane, 16 * i + 8 * s + e)];
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    float w8[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int r = 8 * s + e;
                        const float ev = expf(fminf(0.f, beta * (acc[i][j][r] - wd[e].x)) - wd[e].y);
                        w8[e] = (okm[j] & (1u << (i * 16 + r))) ? ev : 0.f;
                    }
                    if constexpr (DT == 0) {
                        f16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (_Float16)(w8[e] * CT_FP16_SCALE);
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    } else {
                        bf16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (__bf16)w8[e];
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);  // (eight queries at a time: interleaving all 64 exponentials costs registers)
            }

        wait_vmcnt<0>();
        __syncthreads();  // the slices have landed

        // ---- Y[c, z] += W^T P': A = the transposed slice (rows of A = weight columns c), B = the weights
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

    // ---- ((w0 + w1) + w2) + w3 through the LDS (kernels_readout.hip), then the workgroup stores its [64 rows][n_cols] block
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
    // column c of row column `col`: block b = c / 32, lane half (c >> 2) & 1, register (c & 3) + 4 ((c & 31) >> 3) - the C layout of the
    // second product (its rows are the weight columns).  The column's power of two (and the 2^-15 of the fp16 weights) is exact
    constexpr int unscale = DT == 0 ? CT_FP16_SHIFT : 0;
    for (int idx = wave * 64 + lane_e; idx < BN * C_PAD; idx += scan_threads(1)) {  // (wave * 64 + lane_e = tid)
        const int col = idx / C_PAD, c = idx % C_PAD;
        const int z = z0 + col;
        if (z < ntotal && c < n_cols) {
            const int r = (c & 3) + 4 * ((c & 31) >> 3);
            const int l = 32 * ((c >> 2) & 1) + (col & 31);
            const int k = col_k[c];
            const float y = red[(((c >> 5) * NJ + (col >> 5)) * 16 + r) * 64 + l];
            const float v = k == ADJ_K_NAN ? __builtin_nanf("") : ldexpf(y, k - unscale);
            float* at = out + (size_t)z * n_cols + c;
            *at = add ? *at + v : v;
        }
    }
}

bool adjoint_args_ok(const ReadoutAdjointArgs& a) { return scan_store_ok(a.p) && readout_cols_ok(a.c_pad, a.n_cols) && a.w && a.col_k && a.w_stage && a.out; }

}  // namespace

int64_t readout_adjoint_nq_pad(int64_t nq) { return (nq + ADJ_BQ - 1) / ADJ_BQ * ADJ_BQ; }

hipError_t launch_readout_adjoint_columns(const ReadoutAdjointArgs& a, int64_t nq, hipStream_t stream) {
    if (!adjoint_args_ok(a) || nq < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adjoint_colmax_kernel, dim3((unsigned)a.c_pad), dim3(ADJS_T), 0, stream, a.w, nq, a.n_cols, (int*)a.col_k);
    return hipGetLastError();
}

hipError_t launch_posterior_adjoint(const ReadoutAdjointArgs& a, int64_t q_first, int64_t nq, int add, hipStream_t stream) {
    if (nq <= 0 || a.p.ntotal == 0) return hipSuccess;
    if (!adjoint_args_ok(a) || nq > (1 << 20)) return hipErrorInvalidValue;
    const int64_t nq_pad = readout_adjoint_nq_pad(nq);
    if (hipError_t e = launch_scan_stage(a.p, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
    const int64_t n = nq_pad * a.c_pad;
    hipLaunchKernelGGL(adjoint_stage_kernel, dim3((unsigned)((n + ADJS_T - 1) / ADJS_T)), dim3(ADJS_T), 0, stream, a.w + (size_t)q_first * a.n_cols, nq, nq_pad,
                       a.n_cols, a.c_pad, (const int*)a.col_k, a.p.store_dtype, (uint16_t*)a.w_stage);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const FilterExtra ex = scan_filter_extra(a.p, q_first);
    const int n_rtiles = (int)((a.p.ntotal + ADJ_BZ - 1) / ADJ_BZ);
    const int n_qtiles = (int)(nq_pad / ADJ_BQ);
    return contract_dispatch(a.p.store_dtype, ex.row_label != nullptr, [&](auto dt, auto subset) {
        return slices_dispatch<CT_MAX_SLICES>(a.c_pad / 64, [&](auto nsl) {
            return scan_launch_lds<1>(readout_adjoint_kernel<dt.value, subset.value, nsl.value>, scan_grid(n_rtiles, 1), ADJ_LDS, stream, (const uint16_t*)a.p.q_stage,
                                      (const uint16_t*)a.p.store, (const uint16_t*)a.w_stage, (const int*)a.col_k, a.p.out_max + q_first, a.p.out_log_rel + q_first,
                                      (int)a.p.dim_pad, (int)a.p.ntotal, n_rtiles, n_qtiles, (int)nq, a.n_cols, a.p.beta, add, a.out, ex);
        });
    });
}

}  // namespace vodhip
