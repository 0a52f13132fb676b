// The posterior read-out of a per-row value table under the retriever's softmax over the WHOLE store
// (vodhip_index_posterior_expectation, include/vodhip.h H2e):
//   out[q, c] = sum_{rows z < ntotal, eligible} p(z | q) v~[z, c],   p(z | q) = exp(beta <q~, x~_z> - log Z_beta(q)),
// v~ the table of vodhip_index_set_row_values: [tiles * 256][c_pad] of the store dtype, c_pad = 64 * ceil(n_cols / 64), zero padded.
// ONE scan of the store (posterior_mean runs two: the partition scan for the group maxima, then its own), by the online-softmax
// arrangement - a running maximum with rescaling:
//   scan     one workgroup per (group of RO_GT consecutive row tiles, 64 staged queries).  Per tile, in increasing tile order:
//            1. the K loop of the shared scan core (scan_k_loop, store_scan.h: the same score bits as every other scan);
//            2. the epilogue of partition_scan_kernel, restated with its arithmetic and its order: the eligibility mask, the tile
//               maximum m_t across the four row waves, e = expf(beta (s - m_t)) per (row, query), l_t = their sum; part[q][t] =
//               (m_t, l_t), so that partition_finish_kernel gives (max_score, log_rel) with the bits of log_partition;
//            3. the running maximum M of the query column (one value per lane column, known to every row wave): m_t > M multiplies
//               the column's value accumulators by expf(beta (M - m_t)) and sets M = m_t (nothing to rescale while M is -inf);
//               otherwise gamma = expf(beta (m_t - M)) <= 1;
//            4. the weights P' = round16(e * gamma) - the e of step 2, ONE expf per (row, query) - packed as the B fragments of the
//               second product exactly as posterior_scan_kernel packs them (fp16: scaled by 2^15 before the rounding);
//            5. the tile's NSL slices of 64 value columns, streamed by LDS-DMA into the swizzled 128-byte-row image and read
//               transposed (ds_read_b64_tr_b16): Y[c, q] += V[row, c] P'[row, q] in float32.  The image offsets are
//               posterior_scan_kernel's with the table's base and c_pad in place of X and dim_pad.  Every lane is active at those reads.
//            A tile with no eligible row, a +inf score, a query past nq: the weights are +0 and M stays.  At the group's end the waves
//            add as ((w0 + w1) + w2) + w3 through the LDS and acc_g[group][q][c_pad] is stored once; M is then the maximum of the
//            group's finite tile maxima, which the finish recomputes from `part`.
//   finish   out[q, c] = sum over groups g = 0, 1, .. in increasing order of expf(beta (M_g - max_score) - log_rel) * acc_g[q, c];
//            a query with no finite log Z gets the zero row (its accumulators are not read).
// Cost: one K loop + the partition epilogue + NSL slices of the second product (a slice = the MFMAs of one K-loop step) per tile:
// DESIGN.md 4 "Posterior read-out".
//
// ONE order per (query, column), fixed by ntotal, dim_pad and c_pad alone - not by nq, the other queries, the slice of the batch or
// the grid: wave w of the 4 row waves adds its rows 64 w .. 64 w + 63 in k-step order (block i = 0, 1; step s = 0, 1; inside a step the
// MFMA's own order), tile after tile in increasing t with the rescales between them (a rescale by exactly 1 is skipped or done: the same
// bits); then the waves, then the groups.  There are no atomics.  An ineligible row has weight +0 - and 0 * NaN is NaN on the MFMA: a
// NaN / infinity in column c of the table makes column c of every query NaN; the other columns and the two scalar words are unaffected.
// The slice-image geometry, the fp16 weight scale, acc_scale and the host dispatch are scan_contract.h's, which also records why the
// second product itself stays spelled out in this file.
#include "scan_contract.h"

#include "../../include/vodhip.h"

#include <algorithm>

namespace vodhip {

namespace {

constexpr int RO_BN = 64;                                   // queries of a workgroup
constexpr int RO_GT = VODHIP_READOUT_GROUP_ROWS / SCAN_BM;  // tiles of a group
constexpr int RO_A_BYTES = CT_SLICE_BYTES;                  // one slice image
constexpr int RO_IMG = CT_IMG;                              // the slices of the second product; >= the K loop's ring
constexpr int RO_LDS = RO_IMG + 2 * SCAN_WM * RO_BN * (int)sizeof(float);  // + the two reduction arrays of the epilogue
static_assert(RO_BN == CT_BN, "the geometry of scan_contract.h");
static_assert(RO_GT * SCAN_BM == VODHIP_READOUT_GROUP_ROWS && RO_GT >= 1, "the header states the group size");


// X, Q: as partition_scan_kernel; V: the value table [>= n_xtiles * 256][c_pad]; part [nq_pad][n_xtiles] (rows below n_qtiles * 64 are
// written here); acc_out [n_groups][nq_pad][c_pad], c_pad = 64 NSL.  n_qtiles = ceil(nq / 64) <= nq_pad / 64: the staging pads a batch
// above 64 queries to a multiple of 128, and a 64-query tile without a live query is not launched
template <int DT, bool SUBSET, int NSL>
__global__ __launch_bounds__(scan_threads(1), 1)
void readout_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, const uint16_t* __restrict__ V, int dim_pad, int ntotal,
                         int n_xtiles, int n_qtiles, int nq_pad, int nq, float beta, float2* __restrict__ part, float* __restrict__ acc_out, FilterExtra ex) {
    constexpr int BM = SCAN_BM, WM = SCAN_WM, BN = RO_BN;
    constexpr int TM = BM / WM;
    constexpr int MI = TM / 32, NJ = BN / 32;
    constexpr int ROW_BYTES = SCAN_BK * 2;
    constexpr int RPI = 8;
    constexpr int A_BYTES = RO_A_BYTES;
    constexpr int NA = BM / RPI / WM;
    constexpr int NYB = 2 * NSL;      // 32-column blocks of the accumulator
    constexpr int C_PAD = 64 * NSL;
    static_assert(MI == 2 && NJ == 2, "the eligibility mask holds 2 x 16 rows per lane");
    static_assert(NYB * NJ * 16 * 64 * (int)sizeof(float) <= RO_IMG, "the wave reduction fits the LDS");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red_m = reinterpret_cast<float*>(smem + RO_IMG);  // [WM][BN]
    float* red_l = red_m + WM * BN;                          // [WM][BN]

    // XCD-aware order (scan_block_tile's, with a group for the tile): the n_qtiles workgroups that walk one group's tiles land on one
    // XCD back to back and walk them together
    const int bid = blockIdx.x;
    const int xcd = bid & 7, jj = bid >> 3;
    const int qt = jj % n_qtiles;
    const int grp = (jj / n_qtiles) * 8 + xcd;
    if (grp * RO_GT >= n_xtiles) return;  // (uniform over the workgroup, before any barrier)
    const int t_begin = grp * RO_GT;
    const int t_end = min(t_begin + RO_GT, n_xtiles);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave;
    const int q0 = qt * BN;

    // per-lane LDS-DMA sources of the slices (tile 0), in the K loop's image: lane -> (row = base + lane / 8, 16-B slot = lane % 8); slot s
    // of row r holds chunk s ^ ((r >> 1) & 7)
    const int st_row = lane >> 3, st_slot = lane & 7;
    // Row r = 8 (wave NA + u) + st_row: (r >> 1) & 7 depends on u through its parity alone, so a lane has two source offsets (u even,
    // u odd) and a compile-time stride between the rows of equal parity
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
    float run_m[NJ];  // the running maximum per query column of this lane
#pragma unroll
    for (int j = 0; j < NJ; ++j) run_m[j] = -inf;

    f32x16 yacc[NYB][NJ];
#pragma unroll
    for (int b = 0; b < NYB; ++b)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[b][j][r] = 0.f;

    for (int xt = t_begin; xt < t_end; ++xt) {
        const int x0 = xt * BM;
        const char* v_tile = (const char*)V + (size_t)x0 * C_PAD * 2;

        __syncthreads();  // the previous tile's transposed reads are done: the ring may be written
        f32x16 acc[MI][NJ];
        scan_k_loop<DT, BN, 1>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

        // (register classes, no instructions: the value accumulators stay in AGPRs across the K loop, the scores arrive in VGPRs)
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
                glds16(v_tile + v_off[u & 1] + ((u >> 1) * 2 * RPI * C_PAD * 2 + sl * ROW_BYTES), smem + sl * A_BYTES + (wave * NA + u) * RPI * ROW_BYTES);

        // ---- the epilogue of partition_scan_kernel (BN = 64, WN = 1), while the slices arrive
        const int rlane = x0 + wm * TM + 4 * fh;  // the lane's row of (block 0, register 0)
        unsigned okm[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = j * 32 + fr;
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
        bool tile_fin[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = j * 32 + fr;
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
                    const float term = (fin && (okm[j] & (1u << (i * 16 + r)))) ? e : 0.f;
                    l += term;
                    acc[i][j][r] = term;  // the score is not needed again: the register keeps the row's exponential (+0: not counted)
                }
            l += __shfl_xor(l, 32, 64);  // (h = 0) + (h = 1): the same value in both lanes
            if (fh == 0) red_l[wm * BN + col] = l;
            tile_m[j] = m;
            tile_fin[j] = fin;
        }
        __syncthreads();
        if (wm == 0 && fh == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = j * 32 + fr;
                float l = red_l[col];
#pragma unroll
                for (int w = 1; w < WM; ++w) l += red_l[w * BN + col];
                if (tile_m[j] == inf) l = inf;
                part[(size_t)(q0 + col) * n_xtiles + xt] = make_float2(tile_m[j], l);
            }
        }

        // ---- the running maximum: rescale the accumulators of a column whose maximum rose, or shrink the tile's weights
        float gamma[NJ], scale[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float m = tile_m[j], M = run_m[j];
            const bool rises = tile_fin[j] && m > M;
            const bool had = M > -inf;  // (false: the accumulators are zero, and M - m is not formed)
            scale[j] = (rises && had) ? expf(beta * (M - m)) : 1.f;
            gamma[j] = (tile_fin[j] && !rises) ? expf(beta * (m - M)) : 1.f;  // (not rising and finite: M >= m > -inf)
            run_m[j] = rises ? m : M;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (__any(scale[j] != 1.f)) {  // (uniform over the wave; a lane whose scale is 1 multiplies by exactly 1)
#pragma unroll
                for (int b = 0; b < NYB; ++b) acc_scale(yacc[b][j], scale[j]);
            }
        }

        // ---- weights, packed as the B fragments of the second product
        u32x4 wf[MI][2][NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if constexpr (DT == 0) {
                        f16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (_Float16)((acc[i][j][8 * s + e] * gamma[j]) * CT_FP16_SCALE);
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    } else {
                        bf16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (__bf16)(acc[i][j][8 * s + e] * gamma[j]);
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    }
                }

        wait_vmcnt<0>();
        __syncthreads();  // the slices have landed

        // ---- Y[c, q] += V^T P': A = the transposed slice (rows of A = value columns c), B = the weights
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

    // ---- end of the group: ((w0 + w1) + w2) + w3 through the LDS (wave 0 writes, waves 1, 2, 3 add in turn: the accumulators are only
    // read), then the whole workgroup stores the [64 queries][c_pad] block, a query's columns side by side
    __syncthreads();
    // (the lane index from the wave itself: a value of the prologue kept for this block alone would cost a register across the tile loop)
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    float* red = reinterpret_cast<float*>(smem);  // [NYB * NJ * 16][64]: element r of block (b, j) of lane l at ((b NJ + j) 16 + r) 64 + l
    if (wave == 0) {
#pragma unroll
        for (int b = 0; b < NYB; ++b)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x16 v = yacc[b][j];
                asm volatile("" : "+v"(v));  // (one block at a time through 16 vector registers, as in acc_scale)
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
    // column c of query column `col`: block b = c / 32, lane half (c >> 2) & 1, register (c & 3) + 4 ((c & 31) >> 3) - the C layout of
    // the second product (its rows are the value columns)
    const float unscale = DT == 0 ? 1.f / CT_FP16_SCALE : 1.f;
    float* dst = acc_out + ((size_t)grp * (size_t)nq_pad + (size_t)q0) * C_PAD;
    for (int idx = wave * 64 + lane_e; idx < BN * C_PAD; idx += scan_threads(1)) {  // (wave * 64 + lane_e = tid)
        const int col = idx / C_PAD, c = idx % C_PAD;
        const int r = (c & 3) + 4 * ((c & 31) >> 3);
        const int l = 32 * ((c >> 2) & 1) + (col & 31);
        dst[idx] = red[(((c >> 5) * NJ + (col >> 5)) * 16 + r) * 64 + l] * unscale;
    }
}

// One workgroup per query, one thread per value column (c_pad <= 256).  coef_g = expf(beta (M_g - max_score) - log_rel) is computed by
// all threads, RF_CHUNK groups at a time; every thread then adds its column's terms in increasing g.
constexpr int RF_T = 256, RF_CHUNK = 1024;
__global__ void __launch_bounds__(RF_T) readout_finish_kernel(const float2* __restrict__ part, int n_xtiles, int n_groups, const float* __restrict__ acc,
                                                              int64_t nq_pad, int c_pad, int n_cols, float beta, const float* __restrict__ out_max,
                                                              const float* __restrict__ out_log_rel, float* __restrict__ out_values) {
    __shared__ float coef[RF_CHUNK];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float inf = __builtin_inff();
    const float m = out_max[q], lr = out_log_rel[q];
    float sum = 0.f;
    if (m > -inf && m < inf) {  // (uniform over the workgroup); otherwise the zero row
        const float2* p = part + q * n_xtiles;
        for (int g0 = 0; g0 < n_groups; g0 += RF_CHUNK) {
            const int n = min(RF_CHUNK, n_groups - g0);
            for (int i = tid; i < n; i += RF_T) {
                const int t_begin = (g0 + i) * RO_GT, t_end = min(t_begin + RO_GT, n_xtiles);
                float mg = -inf;
                for (int t = t_begin; t < t_end; ++t) mg = fmaxf(mg, p[t].x);
                coef[i] = expf(beta * (mg - m) - lr);  // (a group with no eligible row: exp(-inf) = 0 times its zero accumulator)
            }
            __syncthreads();
            if (tid < n_cols) {
                const float* a = acc + ((size_t)g0 * nq_pad + q) * c_pad + tid;
                for (int i = 0; i < n; ++i) sum += coef[i] * a[(size_t)i * nq_pad * c_pad];
            }
            __syncthreads();
        }
    }
    if (tid < n_cols) out_values[q * n_cols + tid] = sum;
}

}  // namespace

int64_t readout_groups(int64_t ntotal) { return (scan_tiles(ntotal) + RO_GT - 1) / RO_GT; }

hipError_t launch_posterior_expectation(const ReadoutArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = scan_nq_pad(nq);
    const int64_t n_tiles = scan_tiles(a.p.ntotal);
    const int n_groups = (int)readout_groups(a.p.ntotal);
    if (!scan_store_ok(a.p) || nq > (1 << 20) || !readout_cols_ok(a.c_pad, a.n_cols)) return hipErrorInvalidValue;
    if (n_tiles > 0) {
        if (!a.values) return hipErrorInvalidValue;
        if (hipError_t e = launch_scan_stage(a.p, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
        const FilterExtra ex = scan_filter_extra(a.p, q_first);
        const int n_qtiles = (int)((nq + RO_BN - 1) / RO_BN);  // (<= nq_pad / 64: only the tiles that hold a query)
        const hipError_t e = contract_dispatch(a.p.store_dtype, ex.row_label != nullptr, [&](auto dt, auto subset) {
            return slices_dispatch<CT_MAX_SLICES>(a.c_pad / 64, [&](auto nsl) {
                return scan_launch_lds<1>(readout_scan_kernel<dt.value, subset.value, nsl.value>, scan_grid(n_groups, n_qtiles), RO_LDS, stream, (const uint16_t*)a.p.store,
                                          (const uint16_t*)a.p.q_stage, (const uint16_t*)a.values, (int)a.p.dim_pad, (int)a.p.ntotal, (int)n_tiles, n_qtiles, (int)nq_pad,
                                          (int)nq, a.p.beta, (float2*)a.p.part, a.acc, ex);
            });
        });
        if (e != hipSuccess) return e;
    }
    if (hipError_t e = launch_partition_finish(a.p, q_first, nq, stream); e != hipSuccess) return e;
    hipLaunchKernelGGL(readout_finish_kernel, dim3((unsigned)nq), dim3(RF_T), 0, stream, (const float2*)a.p.part, (int)n_tiles, n_groups, a.acc, nq_pad, a.c_pad,
                       a.n_cols, a.p.beta, a.p.out_max + q_first, a.p.out_log_rel + q_first, a.out_values + (size_t)q_first * a.n_cols);
    return hipGetLastError();
}

}  // namespace vodhip
