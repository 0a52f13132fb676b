// The gradient of the posterior read-out in the query (vodhip_index_posterior_expectation_backward, include/vodhip.h H2b):
//   y[q, c] = sum_z p(z | q) v~[z, c]   (kernels_readout.hip),   g[q, c] = dL / dy[q, c]
//   dL/dq[q, :] = beta * sum_{rows z < ntotal, eligible} p(z | q) (u_z - ubar_q) x~_z,   u_z = sum_c g[q, c] v~[z, c],   ubar_q = sum_c g[q, c] y[q, c]:
// a posterior mean with signed, centred per-(row, query) weights.  The centring happens INSIDE the weight: E_p[u x] - ubar E_p[x] from
// two separate means cancels catastrophically for a table column of ones.  The forward's (max_score, log_rel, y) are inputs, so no
// partition scan runs in front: ONE scan of the store.
//   stage    one workgroup per query: k_q = the exponent of max_c |g[q, c]|, g^ = round16(g * 2^-k_q) (the largest entry in [1, 2): a loss
//            gradient of 1e-6 would flush in fp16 unscaled; the scale is exact) -> g_stage [nq_pad][c_pad] of the store dtype, zero padded;
//            ubar_q = float32(sum_c g^[q, c] y[q, c]) summed in double in increasing c over the columns with g^ != 0; R_q = 2^e_q, the
//            power of two above (sum_c |g^[q, c]| vmax_c + |ubar_q|) (1 + 2^-10), vmax_c = the largest finite |v~[., c]| (readout_grad_vmax,
//            cached beside the table), so that |u_z - ubar_q| / R_q <= 1 and no fp16 weight overflows.  Per query: (ubar, 1 / R, k + e, flag);
//            flag 1 = the zero row (g^ all zero, or every |u - ubar| provably 0), flag 2 = the NaN row (a NaN / infinity in g[q, :], in a
//            y[q, c] with g^[q, c] != 0, or R beyond float32): both stage a zero g^ row.
//   scan     one workgroup per (group of RG_GT consecutive row tiles, 64 staged queries, chunk of RG_DC columns of the store): the
//            geometry of readout_scan_kernel, split over column chunks as posterior_scan_kernel is.  Per tile, in increasing order:
//            (a) scan_k_loop on (X tile, Q): the scores, the same bits as every other scan;
//            (b) scan_k_loop on (V tile, g_stage) with dim_pad = c_pad: u[row, q] in the accumulator layout of the scores - the table is
//                laid out [tiles * 256][c_pad] in the store dtype, exactly what the K loop reads;
//            (c) the read-out's eligibility mask, tile maximum m_t, e = expf(beta (s - m_t)), running maximum M with the rescale of the
//                accumulators by expf(beta (M - m_t)), gamma = expf(beta (m_t - M)): restated with their arithmetic; `part` is not written;
//            (d) W' = round16(((e * gamma) * ((u - ubar_q) * (1 / R_q)))), +0 by a select AFTER the product for a row that does not count
//                (a non-finite u in an ineligible row spreads nothing), packed as the B fragments of the second product (fp16: * 2^15);
//            (e) Y[d, q] += X[row, d] W'[row, q] on the chunk's 64-column slices of the tile's rows: LDS-DMA into the swizzled image,
//                ds_read_b64_tr_b16, exactly as posterior_scan_kernel reads them.
//            At the group's end the waves add as ((w0 + w1) + w2) + w3; acc_g[group][q][dim_pad] and the group's final M_g are stored.
//   finish   grad[q, d] = ldexp(beta * sum_g expf(beta (M_g - max_score) - log_rel) acc_g[q, d], k_q + e_q) in increasing g; a query
//            without a finite max_score or with flag 1 gets +0, one with flag 2 NaN.
// ONE order per (query, column), fixed by ntotal, dim_pad and c_pad alone (kernels_readout.hip: the same argument); no atomics.
// The slice-image geometry, the fp16 weight scale, acc_scale and the host dispatch are scan_contract.h's, which also records why the
// second product itself stays spelled out in this file.
#include "scan_contract.h"

#include "../../include/vodhip.h"

#include <algorithm>

namespace vodhip {

namespace {

constexpr int RG_BN = 64;                                   // queries of a workgroup
constexpr int RG_GT = VODHIP_READOUT_GROUP_ROWS / SCAN_BM;  // tiles of a group
// 64-column slices of a workgroup's accumulator.  The score and u accumulators (64 + 64 VGPRs) are live together beside it: with 4
// slices (256 AGPRs) no register is left to hold the scores across the second K loop and the kernel compiles with 132 - 156 bytes of
// scratch per lane; with 3 (192 AGPRs + 64 for the scores) with none (`make check-readout-grad`; DESIGN.md 4 "Read-out gradient")
#ifndef VODHIP_READOUT_GRAD_SLICES
#define VODHIP_READOUT_GRAD_SLICES 3
#endif
constexpr int RG_NSL = VODHIP_READOUT_GRAD_SLICES;
constexpr int RG_DC = 64 * RG_NSL;                          // columns of a full chunk
constexpr int RG_A_BYTES = CT_SLICE_BYTES;                  // one slice image
constexpr int RG_IMG = CT_IMG;                              // the slices of the second product; >= the K loop's ring
constexpr int RG_LDS = RG_IMG + SCAN_WM * RG_BN * (int)sizeof(float);  // + the reduction array of the tile maximum
static_assert(RG_NSL == 3 || RG_NSL == 4, "3 or 4 slices");
static_assert(RG_BN == CT_BN, "the geometry of scan_contract.h");
static_assert(RG_GT * SCAN_BM == VODHIP_READOUT_GROUP_ROWS && RG_GT >= 1, "the header states the group size");


// what the stage kernel leaves per staged query
struct RgQuery {
    float ubar;  // sum_c g^ y
    float rinv;  // 1 / R_q, a power of two
    int shift;   // k_q + e_q: the finish multiplies by 2^shift
    int flag;    // 0 = scan, 1 = the zero row, 2 = the NaN row
};

// ---- vmax_c: the largest finite |v~[z, c]| over the table's rows.  One thread per column, the rows strided over the workgroups; a
// maximum is the same in every order, so the atomic changes no bit (non-negative floats order as their bit patterns)
__global__ void readout_grad_vmax_kernel(const uint16_t* __restrict__ V, int64_t n_rows, int c_pad, int store_dtype, unsigned int* __restrict__ vmax) {
    const int c = threadIdx.x;
    float m = 0.f;
    for (int64_t z = blockIdx.x; z < n_rows; z += gridDim.x) {
        const uint16_t b = V[z * c_pad + c];
        const float v = store_dtype == 0 ? (float)__builtin_bit_cast(_Float16, b) : __uint_as_float((unsigned int)b << 16);
        const float a = fabsf(v);
        if (a < __builtin_inff()) m = fmaxf(m, a);  // (NaN and infinity fail the comparison)
    }
    if (m > 0.f) atomicMax(vmax + c, __float_as_uint(m));
}

// ---- stage: one workgroup per staged query row (rows >= nq: zeros, flag 1)
constexpr int RGS_T = 256;
static_assert(RGS_T >= VODHIP_READOUT_MAX_COLS, "one thread per value column");
__global__ __launch_bounds__(RGS_T)
void readout_grad_stage_kernel(const float* __restrict__ g, const float* __restrict__ y, const float* __restrict__ vmax, int n_cols, int c_pad, int nq,
                               int store_dtype, uint16_t* __restrict__ g_stage, RgQuery* __restrict__ aux) {
    __shared__ float red[RGS_T];
    __shared__ float gh[RGS_T];
    __shared__ int flag;
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const float inf = __builtin_inff();
    const float v = (q < nq && tid < n_cols) ? g[(size_t)q * n_cols + tid] : 0.f;
    const float a = fabsf(v);
    red[tid] = a < inf ? a : inf;  // (a NaN counts as an infinity)
    __syncthreads();
    for (int s = RGS_T / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float amax = red[0];
    const bool scan = amax > 0.f && amax < inf;
    const int k = scan ? ilogbf(amax) : 0;
    float r = 0.f;
    uint16_t bits = 0;
    if (scan) bits = store_bits(ldexpf(v, -k), store_dtype, &r);  // |g 2^-k| < 2: exact scale, one rounding
    gh[tid] = r;
    if (tid < c_pad) g_stage[(size_t)q * c_pad + tid] = bits;
    __syncthreads();
    if (tid == 0) {
        RgQuery w = {0.f, 0.f, 0, amax == 0.f ? 1 : 2};
        if (scan) {
            double ub = 0.0, sa = 0.0;
            for (int c = 0; c < n_cols; ++c) {
                if (gh[c] != 0.f) {
                    ub += (double)gh[c] * (double)y[(size_t)q * n_cols + c];
                    sa += (double)fabsf(gh[c]) * (double)vmax[c];
                }
            }
            const float ubar = (float)ub;
            const double A = (sa + fabs((double)ubar)) * (1.0 + 1.0 / 1024.0);
            int e = 0;
            if (!(A < (double)inf)) {
                w.flag = 2;  // a non-finite y under a non-zero g^
            } else if (A == 0.0) {
                w.flag = 1;  // every u_z and ubar are exactly 0
            } else {
                (void)frexp(A, &e);  // A = f 2^e, 1/2 <= f < 1: R = 2^e > A
                e = max(e, -120);
                if (e > 120) {
                    w.flag = 2;
                } else {
                    w.ubar = ubar;
                    w.rinv = ldexpf(1.f, -e);
                    w.shift = k + e;
                    w.flag = 0;
                }
            }
        }
        aux[q] = w;
        flag = w.flag;
    }
    __syncthreads();
    // a row that is not scanned stages zeros (decided by thread 0 after the bits were written)
    if (flag != 0 && tid < c_pad) g_stage[(size_t)q * c_pad + tid] = 0;
}

// X, Q: as partition_scan_kernel; V: the value table [>= n_xtiles * 256][c_pad]; G: g_stage [nq_pad][c_pad]; aux [nq_pad];
// acc_out [n_groups][nq_pad][dim_pad]; mg_out [n_groups][nq_pad].  n_qtiles = ceil(nq / 64) <= nq_pad / 64.  The launch covers the
// column chunks dc_first .. dc_first + n_dchunks - 1 of RG_DC columns each, NSL slices wide (the last chunk may be narrower)
template <int DT, bool SUBSET, int NSL>
__global__ __launch_bounds__(scan_threads(1), 1)
void readout_grad_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, const uint16_t* __restrict__ V, const uint16_t* __restrict__ G,
                              const RgQuery* __restrict__ aux, int dim_pad, int c_pad, int ntotal, int n_xtiles, int n_qtiles, int n_dchunks, int dc_first,
                              int nq_pad, int nq, float beta, float* __restrict__ acc_out, float* __restrict__ mg_out, FilterExtra ex) {
    constexpr int BM = SCAN_BM, WM = SCAN_WM, BN = RG_BN;
    constexpr int TM = BM / WM;
    constexpr int MI = TM / 32, NJ = BN / 32;
    constexpr int ROW_BYTES = SCAN_BK * 2;
    constexpr int RPI = 8;
    constexpr int A_BYTES = RG_A_BYTES;
    constexpr int NA = BM / RPI / WM;
    constexpr int NYB = 2 * NSL;      // 32-column blocks of the accumulator
    constexpr int C_W = 64 * NSL;     // columns of this launch's chunk
    static_assert(MI == 2 && NJ == 2, "the eligibility mask holds 2 x 16 rows per lane");
    static_assert(NYB * NJ * 16 * 64 * (int)sizeof(float) <= RG_IMG, "the wave reduction fits the LDS");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* red_m = reinterpret_cast<float*>(smem + RG_IMG);  // [WM][BN]

    // XCD-aware order (posterior_scan_kernel's): the workgroups that walk one group's tiles land on one XCD back to back
    const int bid = blockIdx.x;
    const int xcd = bid & 7, jj = bid >> 3;
    const int dc = dc_first + jj % n_dchunks;
    const int qt = (jj / n_dchunks) % n_qtiles;
    const int grp = (jj / (n_dchunks * n_qtiles)) * 8 + xcd;
    if (grp * RG_GT >= n_xtiles) return;  // (uniform over the workgroup, before any barrier)
    const int t_begin = grp * RG_GT;
    const int t_end = min(t_begin + RG_GT, n_xtiles);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave;
    const int q0 = qt * BN;

    // per-lane LDS-DMA sources of the row slices (tile 0, slice 0 of the chunk): kernels_readout.hip's two offsets, with dim_pad for c_pad
    const int st_row = lane >> 3, st_slot = lane & 7;
    static_assert(NA % 2 == 0 && (NA * RPI) % 16 == 0, "the swizzle of a lane's rows has period 2 in u");
    // (formed again in every tile, and the query's words loaded again: a register held across the two K loops is one too many)
    auto x_off = [&](int t) {
        const int r = (wave * NA + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        return (unsigned)(r * dim_pad + c * 8) * 2u + (unsigned)(dc * RG_DC) * 2u;
    };

    const int fr = lane & 31, fh = lane >> 5;

    // transposed reads of a slice image: posterior_scan_kernel's
    const int tq = (lane & 15) >> 2;
    const int t_row = wm * TM + 4 * fh + tq;                       // + 32 i + 16 s + 8 e
    const int t_chunk = 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1);  // + 4 mb
    const int t_sub = 8 * (lane & 1);
    const int t_swz = 2 * fh + (tq >> 1);                          // ((row >> 1) & 7) = 4 e + t_swz

    const float inf = __builtin_inff();
    float run_m[NJ];
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
        const char* x_tile = (const char*)X + (size_t)x0 * dim_pad * 2;

        __syncthreads();  // the previous tile's transposed reads are done: the ring may be written
        f32x16 acc[MI][NJ];
        scan_k_loop<DT, BN, 1>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);
#pragma unroll
        for (int b = 0; b < NYB; ++b)
#pragma unroll
            for (int j = 0; j < NJ; ++j) asm volatile("" : "+a"(yacc[b][j]));
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(acc[i][j]));

        __syncthreads();  // every wave has read its last fragments: the ring is written again
        f32x16 uacc[MI][NJ];
        scan_k_loop<DT, BN, 1>(V + (size_t)x0 * c_pad, G + (size_t)q0 * c_pad, c_pad, smem, uacc);
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

        __syncthreads();  // the LDS becomes the slice images
        {
            const unsigned off[2] = {x_off(0), x_off(1)};
            const unsigned x_pair = (unsigned)(2 * RPI * dim_pad) * 2u;  // between the rows of equal parity
#pragma unroll
            for (int sl = 0; sl < NSL; ++sl)
#pragma unroll
                for (int u = 0; u < NA; ++u)
                    glds16(x_tile + off[u & 1] + ((u >> 1) * x_pair + sl * ROW_BYTES), smem + sl * A_BYTES + (wave * NA + u) * RPI * ROW_BYTES);
        }
        float ubar[NJ], rinv[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const float2 w = *reinterpret_cast<const float2*>(aux + q0 + j * 32 + fr);  // (ubar, rinv)
            ubar[j] = w.x;
            rinv[j] = w.y;
        }

        // ---- the read-out's mask and tile maximum (BN = 64, WN = 1), while the slices arrive
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

        // ---- the running maximum: rescale the accumulators of a column whose maximum rose, or shrink the tile's weights
        float tile_m[NJ], gamma[NJ], scale[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = j * 32 + fr;
            float m = red_m[col];
#pragma unroll
            for (int w = 1; w < WM; ++w) m = fmaxf(m, red_m[w * BN + col]);
            const bool fin = m > -inf && m < inf;
            const float M = run_m[j];
            const bool rises = fin && m > M;
            const bool had = M > -inf;  // (false: the accumulators are zero, and M - m is not formed)
            scale[j] = (rises && had) ? expf(beta * (M - m)) : 1.f;
            gamma[j] = (fin && !rises) ? expf(beta * (m - M)) : 1.f;  // (not rising and finite: M >= m > -inf)
            run_m[j] = rises ? m : M;
            tile_m[j] = m;
            if (!fin) okm[j] = 0u;  // no eligible row, or a +inf score: the tile's weights are +0 and M stays
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
                    float w8[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const int r = 8 * s + e;
                        const float ev = expf(beta * (acc[i][j][r] - tile_m[j]));
                        const float cu = (uacc[i][j][r] - ubar[j]) * rinv[j];
                        const float w = (ev * gamma[j]) * cu;
                        w8[e] = (okm[j] & (1u << (i * 16 + r))) ? w : 0.f;  // the select AFTER the product
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
                    __builtin_amdgcn_sched_barrier(0);  // (eight weights at a time: interleaving all 64 exponentials costs registers)
                }

        wait_vmcnt<0>();
        __syncthreads();  // the slices have landed

        // ---- Y[d, q] += X^T W': A = the transposed slice (rows of A = columns d), B = the weights
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

    // ---- end of the group: ((w0 + w1) + w2) + w3 through the LDS (kernels_readout.hip), then the workgroup stores [64 queries][C_W]
    __syncthreads();
    const int lane_e = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    // the group's final running maximum: every chunk's workgroup holds the same words, chunk 0's stores them (the lane index from the
    // wave itself: a value of the prologue kept for this block alone would cost a register across the tile loop)
    if (dc == 0 && wave == 0 && lane_e < 32) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) mg_out[(size_t)grp * nq_pad + q0 + j * 32 + lane_e] = run_m[j];
    }
    float* red = reinterpret_cast<float*>(smem);  // [NYB * NJ * 16][64]
    if (wave == 0) {
#pragma unroll
        for (int b = 0; b < NYB; ++b)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                f32x16 v = yacc[b][j];
                asm volatile("" : "+v"(v));
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
    // column c of the chunk, query column `col`: block b = c / 32, lane half (c >> 2) & 1, register (c & 3) + 4 ((c & 31) >> 3)
    const float unscale = DT == 0 ? 1.f / CT_FP16_SCALE : 1.f;
    float* dst = acc_out + ((size_t)grp * (size_t)nq_pad + (size_t)q0) * dim_pad + (size_t)dc * RG_DC;
    for (int idx = wave * 64 + lane_e; idx < BN * C_W; idx += scan_threads(1)) {
        const int col = idx / C_W, c = idx % C_W;
        const int r = (c & 3) + 4 * ((c & 31) >> 3);
        const int l = 32 * ((c >> 2) & 1) + (col & 31);
        dst[(size_t)col * dim_pad + c] = red[(((c >> 5) * NJ + (col >> 5)) * 16 + r) * 64 + l] * unscale;
    }
}

// One workgroup per (query, block of GF_T * GF_PER columns): posterior_finish_kernel with the stored group maxima and the query's words
constexpr int GF_T = 256, GF_PER = 4, GF_CHUNK = 1024;
__global__ void __launch_bounds__(GF_T) readout_grad_finish_kernel(const float* __restrict__ mg, int n_groups, const float* __restrict__ acc, const RgQuery* __restrict__ aux,
                                                                   int64_t nq_pad, int dim_pad, int dim, float beta, const float* __restrict__ in_max,
                                                                   const float* __restrict__ in_log_rel, float* __restrict__ out_grad) {
    __shared__ float coef[GF_CHUNK];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int d0 = blockIdx.y * (GF_T * GF_PER);
    const float inf = __builtin_inff();
    const float m = in_max[q], lr = in_log_rel[q];
    const RgQuery w = aux[q];
    float sum[GF_PER];
#pragma unroll
    for (int e = 0; e < GF_PER; ++e) sum[e] = 0.f;
    const bool live = w.flag == 0 && m > -inf && m < inf;  // (uniform over the workgroup)
    if (live) {
        for (int g0 = 0; g0 < n_groups; g0 += GF_CHUNK) {
            const int n = min(GF_CHUNK, n_groups - g0);
            for (int i = tid; i < n; i += GF_T) coef[i] = expf(beta * (mg[(size_t)(g0 + i) * nq_pad + q] - m) - lr);  // (no eligible row: exp(-inf) = 0)
            __syncthreads();
#pragma unroll
            for (int e = 0; e < GF_PER; ++e) {
                const int d = d0 + e * GF_T + tid;
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
    for (int e = 0; e < GF_PER; ++e) {
        const int d = d0 + e * GF_T + tid;
        if (d < dim) out_grad[q * dim + d] = w.flag == 2 ? __builtin_nanf("") : (live ? ldexpf(beta * sum[e], w.shift) : 0.f);
    }
}

}  // namespace

size_t readout_grad_aux_bytes() { return sizeof(RgQuery); }

hipError_t launch_readout_grad_vmax(const void* values, int64_t n_rows, int c_pad, int store_dtype, float* vmax, hipStream_t stream) {
    if (!readout_cols_ok(c_pad, 1)) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(vmax, 0, (size_t)c_pad * sizeof(float), stream); e != hipSuccess) return e;
    if (n_rows <= 0) return hipSuccess;
    const unsigned grid = (unsigned)std::min<int64_t>(n_rows, 2048);
    hipLaunchKernelGGL(readout_grad_vmax_kernel, dim3(grid), dim3((unsigned)c_pad), 0, stream, (const uint16_t*)values, n_rows, c_pad, store_dtype, (unsigned int*)vmax);
    return hipGetLastError();
}

hipError_t launch_posterior_expectation_backward(const ReadoutGradArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = scan_nq_pad(nq);
    const int64_t n_tiles = scan_tiles(a.p.ntotal);
    const int n_groups = (int)readout_groups(a.p.ntotal);
    if (!scan_store_ok(a.p) || nq > (1 << 20) || !readout_cols_ok(a.c_pad, a.n_cols)) return hipErrorInvalidValue;
    if (!a.vmax || !a.g || !a.y || !a.g_stage || !a.aux) return hipErrorInvalidValue;
    hipLaunchKernelGGL(readout_grad_stage_kernel, dim3((unsigned)nq_pad), dim3(RGS_T), 0, stream, a.g + (size_t)q_first * a.n_cols, a.y + (size_t)q_first * a.n_cols,
                       a.vmax, a.n_cols, a.c_pad, (int)nq, a.p.store_dtype, (uint16_t*)a.g_stage, (RgQuery*)a.aux);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (n_tiles > 0) {
        if (!a.values) return hipErrorInvalidValue;
        if (hipError_t e = launch_scan_stage(a.p, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
        const FilterExtra ex = scan_filter_extra(a.p, q_first);
        const int n_qtiles = (int)((nq + RG_BN - 1) / RG_BN);  // (<= nq_pad / 64: only the tiles that hold a query)
        const hipError_t e = contract_dispatch(a.p.store_dtype, ex.row_label != nullptr, [&](auto dt, auto subset) {
            return chunks_dispatch<RG_NSL>((int)(a.p.dim_pad / 64), [&](auto nsl, int dc_first, int n_dchunks) {
                return scan_launch_lds<1>(readout_grad_scan_kernel<dt.value, subset.value, nsl.value>, scan_grid(n_groups, n_qtiles * n_dchunks), RG_LDS, stream,
                                          (const uint16_t*)a.p.store, (const uint16_t*)a.p.q_stage, (const uint16_t*)a.values, (const uint16_t*)a.g_stage,
                                          (const RgQuery*)a.aux, (int)a.p.dim_pad, a.c_pad, (int)a.p.ntotal, (int)n_tiles, n_qtiles, n_dchunks, dc_first, (int)nq_pad,
                                          (int)nq, a.p.beta, a.acc, a.mg, ex);
            });
        });
        if (e != hipSuccess) return e;
    }
    const unsigned dblocks = (unsigned)((a.p.dim + GF_T * GF_PER - 1) / (GF_T * GF_PER));
    hipLaunchKernelGGL(readout_grad_finish_kernel, dim3((unsigned)nq, dblocks), dim3(GF_T), 0, stream, a.mg, n_groups, a.acc, (const RgQuery*)a.aux, nq_pad,
                       (int)a.p.dim_pad, (int)a.p.dim, a.p.beta, a.p.out_max + q_first, a.p.out_log_rel + q_first, a.out_grad + (size_t)q_first * a.p.dim);
    return hipGetLastError();
}

}  // namespace vodhip
