// The core of the whole-store scans: log_partition (kernels_partition.hip), posterior_stats (kernels_stats.hip), posterior_divergence
// (kernels_divergence.hip), range_search (kernels_range.hip), sample_posterior (kernels_sample_posterior.hip), rank_ids / count_above
// (kernels_rank.hip), and the five that contract their weights with a second operand (scan_contract.h: their geometry and host side):
// posterior_mean (kernels_posterior.hip), posterior_expectation (kernels_readout.hip), its gradient in the query
// (kernels_readout_grad.hip), its adjoint in the value table (kernels_readout_adjoint.hip) and key_gradient (kernels_key_grad.hip).  Each
// of them scores a tile of 256 streamed rows against 64 | 128 resident ones with the ONE K loop below and differs from the others in its
// epilogue alone (posterior_divergence also in the row map of its staging: the two queries of a pair sit 32 columns apart, in the two
// accumulator columns of one lane).  The streamed rows are stored rows and the resident ones staged queries, except in the adjoint and
// the key gradient, which exchange the operands: the loop is symmetric in the two.
//
// THE CONTRACT.  A (query, row) pair has one score, the same bits in every scan and the bits a search returns:
//   score     scan_k_loop is the K loop of mips_filter_kernel (kernels_mips.hip): LDS-DMA with the source-side XOR swizzle, a 3-slot
//             ring, v_mfma_f32_32x32x16 with the rows as A and the staged queries as B.  An output element depends on its A row and its
//             B column alone and is summed in the MFMA's own order over the dim_pad / 16 k-steps, the same for every column of the B
//             operand, for the 64-query and the 128-query instantiation, for every grid and every split of a batch.
//   C layout  a lane's accumulator column is ONE query, col = lane & 31, and its registers are rows: register r of 32-row block i of
//             the wave's 64 rows is row 32 i + (r & 3) + 8 (r >> 2) + 4 (lane >> 5) - scan_lane_row with bit = 16 i + r.
//   eligible  row z counts for query q when z < ntotal (rows past it are zero or stale, tile padding reaches past the capacity), its
//             score is not NaN (a search leaves NaN out too) and the query's subset labels allow it (subset_allows, mips_common.h):
//             scan_eligible_mask.
//   queries   staged by launch_scan_stage (kernels_partition.hip): [nq_pad][dim_pad] of the store dtype, rounded as a search rounds
//             them (store_bits: saturating), zero padded.
#pragma once
#include "mips_common.h"

#include <type_traits>

namespace vodhip {

constexpr int SCAN_BM = 256;     // stored rows of a tile
constexpr int SCAN_WM = 4;       // row waves: a wave holds 64 rows of the tile
constexpr int SCAN_NSTAGE = 3;   // LDS ring depth
constexpr int SCAN_BK = 64;      // columns of a K-loop step: one 128-byte LDS row
constexpr int scan_threads(int wn) { return SCAN_WM * wn * 64; }
constexpr int scan_ring_bytes(int bn) { return SCAN_NSTAGE * (SCAN_BM + bn) * SCAN_BK * 2; }

// XCD-aware tile order (as mips_filter_kernel): the n_qtiles workgroups that re-read one row tile land on one XCD back to back.
// False (uniform over the workgroup): the grid's padding, no tile.
__device__ __forceinline__ bool scan_block_tile(int bid, int n_qtiles, int n_xtiles, int* qt, int* xt) {
    const int xcd = bid & 7, jj = bid >> 3;
    *qt = jj % n_qtiles;
    *xt = (jj / n_qtiles) * 8 + xcd;
    return *xt < n_xtiles;
}

// rlane: the lane's row of (block 0, register 0) = the tile's first row + 64 * (row wave) + 4 * (lane >> 5); bit = 16 i + r
__device__ __forceinline__ int scan_lane_row(int rlane, int bit) { return rlane + (bit >> 4) * 32 + (bit & 3) + 8 * ((bit & 15) >> 2); }

// X: the first of 256 rows [dim_pad]; Q: the first of BN staged queries.  On return every wave may still be reading the ring: a
// __syncthreads() precedes any reuse of `smem` (scan_ring_bytes(BN) bytes).
template <int DT, int BN, int WN>
__device__ __forceinline__ void scan_k_loop(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, char* smem,
                                            f32x16 (&acc)[2][BN / WN / 32]) {
    constexpr int BM = SCAN_BM, WM = SCAN_WM, NSTAGE = SCAN_NSTAGE, BK = SCAN_BK;
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
    static_assert(MI == 2, "a lane holds 2 x 16 rows per query column");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;

    // per-lane LDS-DMA sources: lane -> (row = base + lane / 8, 16-B slot = lane % 8); slot s of row r holds chunk s ^ ((r >> 1) & 7)
    const int st_row = lane >> 3, st_slot = lane & 7;
    const char* a_src[NA];
    const char* b_src[NB];
#pragma unroll
    for (int t = 0; t < NA; ++t) {
        const int r = (wave * NA + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        a_src[t] = (const char*)X + ((size_t)r * dim_pad + c * 8) * 2;
    }
#pragma unroll
    for (int t = 0; t < NB; ++t) {
        const int r = (wave * NB + t) * RPI + st_row;
        const int c = st_slot ^ ((r >> 1) & 7);
        b_src[t] = (const char*)Q + ((size_t)r * dim_pad + c * 8) * 2;
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
}

// The eligible rows of one query column of a lane: bit 16 i + r = register r of block i.  a0 / a1: the column's two accumulators
// (taken by reference, so that the column index stays a compile-time constant at the call site: a rolled index reads the accumulator
// through scratch).  The caller has checked q < nq.
template <bool SUBSET>
__device__ __forceinline__ unsigned scan_eligible_mask(const f32x16& a0, const f32x16& a1, int rlane, int ntotal, int q, const FilterExtra& ex) {
    unsigned mask = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) mask |= (scan_lane_row(rlane, r) < ntotal && a0[r] == a0[r]) ? (1u << r) : 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) mask |= (scan_lane_row(rlane, 16 + r) < ntotal && a1[r] == a1[r]) ? (1u << (16 + r)) : 0u;
    if constexpr (SUBSET) {  // rolled: one label test per row that is still in
        unsigned m2 = mask;
        while (m2) {
            const int b = __builtin_ctz(m2);
            m2 &= m2 - 1;
            if (!subset_allows(ex, q, scan_lane_row(rlane, b))) mask &= ~(1u << b);
        }
    }
    return mask;
}

// ---- host side: the launch of a scan kernel ------------------------------------------------------------------------------------
// f(dt, bn, wn, subset) with the four compile-time tags (std::integral_constant) of the instantiation that scans nq_pad staged queries
template <class F>
hipError_t scan_dispatch(int store_dtype, int64_t nq_pad, bool subset, F&& f) {
    auto with_subset = [&](auto dt, auto bn, auto wn) { return subset ? f(dt, bn, wn, std::true_type{}) : f(dt, bn, wn, std::false_type{}); };
    auto with_width = [&](auto dt) {
        return nq_pad == 64 ? with_subset(dt, std::integral_constant<int, 64>{}, std::integral_constant<int, 1>{})
                            : with_subset(dt, std::integral_constant<int, 128>{}, std::integral_constant<int, 2>{});
    };
    return store_dtype == 0 ? with_width(std::integral_constant<int, 0>{}) : with_width(std::integral_constant<int, 1>{});
}

// one workgroup per (row tile, query tile) in the order scan_block_tile decodes: the row tiles padded to the 8 XCDs
inline int64_t scan_grid(int n_tiles, int n_qtiles) { return (int64_t)((n_tiles + 7) / 8) * 8 * n_qtiles; }

// a kernel of WN column waves on `grid` workgroups with `lds` bytes of dynamic LDS
template <int WN, class K, class... A>
hipError_t scan_launch_lds(K kern, int64_t grid, int lds, hipStream_t stream, A... args) {
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    if (hipError_t e = allow_dynamic_lds((const void*)kern, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(scan_threads(WN)), lds, stream, args...);
    return hipGetLastError();
}
// a kernel of the (BN, WN) geometry with the ring as its dynamic LDS
template <int BN, int WN, class K, class... A>
hipError_t scan_launch(K kern, int64_t grid, hipStream_t stream, A... args) {
    return scan_launch_lds<WN>(kern, grid, scan_ring_bytes(BN), stream, args...);
}

}  // namespace vodhip
