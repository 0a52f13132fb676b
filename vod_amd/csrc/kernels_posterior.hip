// The posterior mean of the stored rows under the retriever's softmax over the WHOLE store (vodhip_index_posterior_mean,
// include/vodhip.h H2m) = the gradient of log Z_beta(q) with respect to q, divided by beta:
//   mean[q, :] = sum_{rows z < ntotal, eligible} p(z | q) x~_z,   p(z | q) = exp(beta <q~, x~_z> - log Z_beta(q)).
// The call first runs the three launches of kernels_partition.hip unchanged (stage, scan, finish): (max_score, log_rel) are that call's
// bits, and its `part` array holds every 256-row tile's maximum.  Then two kernels of this file:
//   scan     one workgroup per (group of PM_GT consecutive row tiles, 64 queries, chunk of PM_DC = 256 columns).  Per tile it runs the
//            K loop of the shared scan core (scan_k_loop, store_scan.h: the same score bits as every other scan), turns the score accumulators
//            into weights P'[row, q] = exp(beta (s - m_ref(q))) rounded to the store dtype, m_ref(q) = the maximum of the group's tile
//            maxima (>= every score of the group, so the group's largest weight is exactly 1), and contracts them with the tile's rows
//            on the MFMA: Y[d, q] += sum_row X[row, d] P'[row, q].  The first product has the corpus as A and the queries as B, so a
//            lane's accumulator column is one query and its registers are rows: packed pairwise, registers 8 s .. 8 s + 7 of a 32-row
//            block ARE the B fragment of k-step s of the second product, with no lane movement.  Its A operand, the transpose of a
//            64-column slice of the tile's rows, is streamed by the same LDS-DMA into the same swizzled 128-byte-row image the K loop
//            uses and read column-wise with ds_read_b64_tr_b16, in the permuted k order of the packed accumulator: element j of lane
//            half h is row 16 s + 8 (j >> 2) + 4 h + (j & 3) of the block.  Every lane is active at those reads (no divergence above
//            them; the tile is padded, not masked).
//            fp16: a weight is multiplied by 2^15 before it is rounded (the largest stays below 65504), so it is a NORMAL fp16
//            number down to 2^-29 of the group's largest; the group's sum is multiplied by 2^-15 in float32 (both exact).  bf16 has
//            float32's exponent range and needs no scale.
//            The workgroup keeps its [256 columns x 64 queries] float32 accumulator in registers across the tiles of its group and
//            writes acc_g[group][q][column] once.
//   finish   mean[q, d] = sum over groups g = 0, 1, .. in increasing order of exp(beta (m_g - max_score) - log_rel) * acc_g[q, d].
// Cost: the scores are recomputed once per column chunk, so a tile costs (dim_pad / 256 rounded up) K loops + dim_pad / 64 slices of
// the second product (a slice = the MFMAs of one K-loop step) = about (ceil(dim_pad / 256) + 1) K-loop equivalents, + 1 for the
// partition scan in front: DESIGN.md 4 "Posterior mean".
//
// ONE order per (query, column), fixed by ntotal and dim_pad alone - not by nq, the other queries, the slice of the batch or the grid:
//   tile t  rows [256 t, 256 t + 256), group g = tiles [PM_GT g, PM_GT g + PM_GT).  Wave w of the 4 row waves holds rows 64 w .. 64 w + 63
//           and adds them into its own accumulator in k-step order (block i = 0, 1; step s = 0, 1; inside a step the MFMA's own order),
//           tile after tile in increasing t; at the end of the group the four waves add as ((w0 + w1) + w2) + w3.
//   finish  in increasing g, starting from 0.
// There are no atomics.  A row is eligible by the rule of the scan core (store_scan.h: row < ntotal, score not NaN, subset_allows); an
// ineligible row has weight +0 - and 0 * NaN is NaN on the MFMA: a stored NaN / infinity in column d of any scanned tile (rows past
// ntotal up to the tile's end included) makes column d of every query's mean NaN.  No eligible row or a +inf score: the mean row is 0.
// The slice-image geometry, the fp16 weight scale, acc_scale and the host dispatch are scan_contract.h's, which also records why the
// second product itself stays spelled out in this file.
#include "scan_contract.h"

#include "../../include/vodhip.h"

#include <algorithm>

namespace vodhip {

namespace {

constexpr int PM_BN = 64;      // queries of a workgroup
constexpr int PM_DC = 256;     // columns of a workgroup's accumulator
constexpr int PM_GT = 64;      // tiles of a group: VODHIP_POSTERIOR_GROUP_ROWS / 256
constexpr int PM_A_BYTES = CT_SLICE_BYTES;
constexpr int PM_LDS = CT_IMG;  // the 4 slices of the second product; >= the K loop's ring
static_assert(PM_BN == CT_BN && PM_DC == 64 * CT_MAX_SLICES, "the geometry of scan_contract.h");
static_assert(PM_GT * SCAN_BM == VODHIP_POSTERIOR_GROUP_ROWS, "the header states the group size");


// X, Q, part: as partition_scan_kernel (part [n_qtiles * 64][n_xtiles], already written); acc_out [n_groups][n_qtiles * 64][dim_pad]
template <int DT, bool SUBSET, int NSL>
__global__ __launch_bounds__(scan_threads(1), 1)
void posterior_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles,
                           int n_dchunks, int dc_first, int nq, float beta, const float2* __restrict__ part, float* __restrict__ acc_out, FilterExtra ex) {
    constexpr int BM = SCAN_BM, WM = SCAN_WM, BN = PM_BN;
    constexpr int TM = BM / WM;
    constexpr int MI = TM / 32, NJ = BN / 32;
    constexpr int ROW_BYTES = SCAN_BK * 2;
    constexpr int RPI = 8;
    constexpr int A_BYTES = PM_A_BYTES;
    constexpr int NA = BM / RPI / WM;
    constexpr int NYB = 2 * NSL;      // 32-column blocks of the accumulator (NSL = the chunk's 64-column slices)
    static_assert(MI == 2 && NJ == 2, "the eligibility mask holds 2 x 16 rows per lane");
    static_assert(NYB * NJ * 16 * 64 * (int)sizeof(float) <= PM_LDS, "the wave reduction fits the LDS");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    // XCD-aware order (scan_block_tile's, with a group for the tile and the chunk index below the query tile): the n_qtiles * n_dchunks
    // workgroups that walk one group's tiles land on one XCD back to back and walk them together, so a tile comes from HBM once and from
    // that XCD's L2 for the others
    const int bid = blockIdx.x;
    const int xcd = bid & 7, jj = bid >> 3;
    const int dc = dc_first + jj % n_dchunks;
    const int qt = (jj / n_dchunks) % n_qtiles;
    const int grp = (jj / (n_dchunks * n_qtiles)) * 8 + xcd;
    if (grp * PM_GT >= n_xtiles) return;  // (uniform over the workgroup, before any barrier)
    const int t_begin = grp * PM_GT;
    const int t_end = min(t_begin + PM_GT, n_xtiles);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave;
    const int q0 = qt * BN;

    // per-lane LDS-DMA sources of the slices (tile 0), in the K loop's image: lane -> (row = base + lane / 8, 16-B slot = lane % 8); slot s
    // of row r holds chunk s ^ ((r >> 1) & 7)
    const int st_row = lane >> 3, st_slot = lane & 7;
    const char* a_src0[NA];
#pragma unroll
    for (int t = 0; t < NA; ++t) {
        const int r = (wave * NA + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        a_src0[t] = (const char*)X + ((size_t)r * dim_pad + c * 8) * 2;
    }

    const int fr = lane & 31, fh = lane >> 5;

    // transposed reads of a slice image (T10): the 16 lanes of group gq = lane >> 4 read a block of 4 rows x 16 columns, lane 4 q + p
    // of the group supplies row q, columns 4 p .. 4 p + 3, and receives column (lane & 15) of the 4 rows.  The group's columns are
    // 32 mb + 16 (gq & 1) .., its rows 64 wm + 32 i + 16 s + 8 e + 4 fh .. (e = 0: fragment elements 0 .. 3, e = 1: elements 4 .. 7)
    const int tq = (lane & 15) >> 2;
    const int t_row = wm * TM + 4 * fh + tq;                       // + 32 i + 16 s + 8 e
    const int t_chunk = 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1);  // + 4 mb
    const int t_sub = 8 * (lane & 1);
    const int t_swz = 2 * fh + (tq >> 1);                          // ((row >> 1) & 7) = 4 e + t_swz

    const float inf = __builtin_inff();
    // the group's reference maximum per query column of this lane
    float mref[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const float2* p = part + (size_t)(q0 + j * 32 + fr) * n_xtiles;
        float m = -inf;
        for (int t = t_begin; t < t_end; ++t) m = fmaxf(m, p[t].x);
        mref[j] = m;
    }

    f32x16 yacc[NYB][NJ];
#pragma unroll
    for (int b = 0; b < NYB; ++b)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) yacc[b][j][r] = 0.f;

    for (int xt = t_begin; xt < t_end; ++xt) {
        const int x0 = xt * BM;
        const size_t tile_off = (size_t)x0 * dim_pad * 2;

        __syncthreads();  // the previous tile's transposed reads are done: the ring may be written
        f32x16 acc[MI][NJ];
        scan_k_loop<DT, BN, 1>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

        __syncthreads();  // every wave has read its last fragments: the LDS becomes the slice images
        // slice sl of the chunk is the A half of K-loop step 4 dc + sl, in the same image
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl) {
                const int kbyte = (dc * (PM_DC / 64) + sl) * ROW_BYTES;
#pragma unroll
                for (int u = 0; u < NA; ++u) glds16(a_src0[u] + tile_off + kbyte, smem + sl * A_BYTES + (wave * NA + u) * RPI * ROW_BYTES);
            }

        // ---- scores -> weights, packed as the B fragments of the second product (while the slices arrive)
        const int rlane = x0 + wm * TM + 4 * fh;  // the lane's row of (block 0, register 0)
        u32x4 wf[MI][2][NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = j * 32 + fr;
            const int q = q0 + col;
            unsigned mask = q < nq ? scan_eligible_mask<SUBSET>(acc[0][j], acc[1][j], rlane, ntotal, q, ex) : 0u;
            const float m = mref[j];
            if (!(m > -inf && m < inf)) mask = 0u;  // no eligible row in the group, or a +inf score: the finish writes the zero row
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if constexpr (DT == 0) {
                        f16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int r = 8 * s + e;
                            const float w = expf(beta * (acc[i][j][r] - m)) * CT_FP16_SCALE;
                            v[e] = (_Float16)((mask & (1u << (i * 16 + r))) ? w : 0.f);
                        }
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    } else {
                        bf16x8 v;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            const int r = 8 * s + e;
                            const float w = expf(beta * (acc[i][j][r] - m));
                            v[e] = (__bf16)((mask & (1u << (i * 16 + r))) ? w : 0.f);
                        }
                        wf[i][s][j] = __builtin_bit_cast(u32x4, v);
                    }
                }
        }

        wait_vmcnt<0>();
        __syncthreads();  // the slices have landed

        // ---- Y[d, q] += X^T P': A = the transposed slice (rows of A = columns d), B = the weights
#pragma unroll
        for (int sl = 0; sl < NSL; ++sl) {
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
    }

    // ---- end of the group: ((w0 + w1) + w2) + w3 through the LDS, then one store per (query, 4 columns)
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);  // [NYB * NJ * 16][64]
#pragma unroll 1
    for (int w = 0; w < WM; ++w) {
        if (wave == w) {
#pragma unroll
            for (int b = 0; b < NYB; ++b)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int at = ((b * NJ + j) * 16 + r) * 64 + lane;
                        float v = yacc[b][j][r];
                        if (w > 0) v = red[at] + v;
                        if (w < WM - 1) red[at] = v;
                        else yacc[b][j][r] = v;
                    }
        }
        __syncthreads();
    }
    if (wave == WM - 1) {
        const float unscale = DT == 0 ? 1.f / CT_FP16_SCALE : 1.f;
#pragma unroll
        for (int b = 0; b < NYB; ++b) {
            {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    float* dst = acc_out + ((size_t)grp * ((size_t)n_qtiles * BN) + (size_t)(q0 + j * 32 + fr)) * dim_pad + dc * PM_DC + b * 32 + 4 * fh;
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = yacc[b][j][4 * r4 + e] * unscale;
                        *(f32x4*)(dst + 8 * r4) = v;
                    }
                }
            }
        }
    }
}

// One workgroup per (query, block of PF_T * PF_PER columns).  coef_g = exp(beta (m_g - max_score) - log_rel) is computed by all threads,
// PF_CHUNK groups at a time; every thread then adds its columns' terms in increasing g.
constexpr int PF_T = 256, PF_PER = 4, PF_CHUNK = 1024;
__global__ void __launch_bounds__(PF_T) posterior_finish_kernel(const float2* __restrict__ part, int n_xtiles, int n_groups, const float* __restrict__ acc,
                                                                int64_t nq_pad, int dim_pad, int dim, float beta, const float* __restrict__ out_max,
                                                                const float* __restrict__ out_log_rel, float* __restrict__ out_mean) {
    __shared__ float coef[PF_CHUNK];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int d0 = blockIdx.y * (PF_T * PF_PER);
    const float inf = __builtin_inff();
    const float m = out_max[q], lr = out_log_rel[q];
    float sum[PF_PER];
#pragma unroll
    for (int e = 0; e < PF_PER; ++e) sum[e] = 0.f;
    if (m > -inf && m < inf) {  // (uniform over the workgroup); otherwise the zero row
        const float2* p = part + q * n_xtiles;
        for (int g0 = 0; g0 < n_groups; g0 += PF_CHUNK) {
            const int n = min(PF_CHUNK, n_groups - g0);
            for (int i = tid; i < n; i += PF_T) {
                const int t_begin = (g0 + i) * PM_GT, t_end = min(t_begin + PM_GT, n_xtiles);
                float mg = -inf;
                for (int t = t_begin; t < t_end; ++t) mg = fmaxf(mg, p[t].x);
                coef[i] = expf(beta * (mg - m) - lr);  // (a group with no eligible row: exp(-inf) = 0)
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < PF_PER; ++e) {
                const int d = d0 + e * PF_T + tid;
                if (d < dim) {
                    const float* a = acc + ((size_t)g0 * nq_pad + q) * dim_pad + d;
                    float s = sum[e];
                    for (int i = 0; i < n; ++i) s += coef[i] * a[(size_t)i * nq_pad * dim_pad];
                    sum[e] = s;
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int e = 0; e < PF_PER; ++e) {
        const int d = d0 + e * PF_T + tid;
        if (d < dim) out_mean[q * dim + d] = sum[e];
    }
}

}  // namespace

int64_t posterior_mean_groups(int64_t ntotal) { return (scan_tiles(ntotal) + PM_GT - 1) / PM_GT; }

hipError_t launch_posterior_mean(const PosteriorArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (hipError_t e = launch_log_partition(a.p, q_first, nq, stream); e != hipSuccess) return e;  // (checks the shapes)
    const int64_t nq_pad = scan_nq_pad(nq);
    const int n_tiles = (int)scan_tiles(a.p.ntotal);
    const int n_groups = (int)posterior_mean_groups(a.p.ntotal);
    if (n_tiles > 0) {
        const FilterExtra ex = scan_filter_extra(a.p, q_first);
        const int n_qtiles = (int)(nq_pad / PM_BN);
        // the full 256-column chunks in one launch, the last chunk of 64 | 128 | 192 columns (if any) in a second one
        const hipError_t e = contract_dispatch(a.p.store_dtype, ex.row_label != nullptr, [&](auto dt, auto subset) {
            return chunks_dispatch<PM_DC / 64>((int)(a.p.dim_pad / 64), [&](auto nsl, int dc_first, int n_dchunks) {
                return scan_launch_lds<1>(posterior_scan_kernel<dt.value, subset.value, nsl.value>, scan_grid(n_groups, n_qtiles * n_dchunks), PM_LDS, stream,
                                          (const uint16_t*)a.p.store, (const uint16_t*)a.p.q_stage, (int)a.p.dim_pad, (int)a.p.ntotal, n_tiles, n_qtiles, n_dchunks, dc_first,
                                          (int)nq, a.p.beta, (const float2*)a.p.part, a.acc, ex);
            });
        });
        if (e != hipSuccess) return e;
    }
    const unsigned dblocks = (unsigned)((a.p.dim + PF_T * PF_PER - 1) / (PF_T * PF_PER));
    hipLaunchKernelGGL(posterior_finish_kernel, dim3((unsigned)nq, dblocks), dim3(PF_T), 0, stream, (const float2*)a.p.part, n_tiles, n_groups, a.acc, nq_pad,
                       (int)a.p.dim_pad, (int)a.p.dim, a.p.beta, a.p.out_max + q_first, a.p.out_log_rel + q_first, a.out_mean + (size_t)q_first * a.p.dim);
    return hipGetLastError();
}

}  // namespace vodhip
