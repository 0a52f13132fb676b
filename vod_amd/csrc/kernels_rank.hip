// Exact ranks over the WHOLE store (vodhip_index_rank_ids / vodhip_index_count_above / vodhip_index_scan_score_ids, include/vodhip.h H2r).
//
// Definitions.  Scores s(q, z) and ELIGIBLE rows are the shared scan core's (store_scan.h).  ORDER is the search's:
// key(s) = flip_f32(s) (mips_common.h), so -0.0 and +0.0 are equal, and ties go to the smaller id.  For a threshold t and a tie id r
//   C(q; t, r) = #{ eligible rows z : key(s(q, z)) > key(t)  or  (key(s(q, z)) == key(t) and id_base + z < r) }.
//   count_above   out[q, j] = C(q; thresholds[q, j], tie_ids[q, j]); without tie ids the count is strict (r = -inf); a NaN threshold: -1
//   rank_ids      score[q, j] = the scan's score of row ids[q, j] - the bits a search returns for that pair - and
//                 rank[q, j] = C(q; score[q, j], ids[q, j]): the 0-based position at which a search over the eligible rows returns the
//                 row.  PRESENT is score_ids's rule (id >= 0, id - id_base in [0, ntotal), label allowed); an absent slot is (-1, -inf),
//                 a NaN score rank -1 with the score as computed.  Duplicates are independent slots.
//
// Kernels (one slice of the batch at a time; every table below is a stream-ordered temporary of the slice):
//   stage    queries -> [nq_pad][dim_pad] of the store dtype (launch_scan_stage)
//   resolve  listed ids -> local rows (-1 = absent)
//   gather   the present listed rows of a query tile -> a MINI-STORE [BN * m rows, padded to 256][dim_pad]: row j * BN + c holds the row
//            of slot j of the tile's query column c; absent slots are zero rows
//   pick     scan_k_loop over the mini-store's tiles against that query tile only.  An MFMA output element depends on its A row
//            and its B column alone, and the K loop adds the dim_pad / 16 k-steps in the scan's order, so element (row of slot (q, j),
//            column q) is the scan's score of that pair, bit for bit; the epilogue writes those BN * m elements and drops the rest
//   prep     (score, local row) or (threshold, tie id) -> the slot table: key(t) and the LOCAL tie row r in [0, ntotal] (0 = strict),
//            laid out [query tile][slot][BN] so that a workgroup copies its part to LDS in one coalesced pass; a slot that counts nothing
//            (absent, NaN, a padding query) holds key 0xFFFFFFFF, which no eligible row exceeds; the counts are cleared
//   count    the scan core over a 256-row tile x 64 | 128 queries (XCD-aware tile order, SUBSET a template flag) with an integer
//            epilogue: a lane turns its 32 accumulators of a query column into keys (0 for an ineligible row: below
//            every threshold) and, slot by slot (rolled), counts key > te.  In every tile but the one that holds the tie row all rows lie
//            on one side of it: below r the tie test folds into the threshold (key >= t is key > t - 1 on the integer key), above it the
//            test is strict - one compare and one add per (accumulator, slot).  Only the tie row's own tile adds the per-row test
//            key == t and row < r.  The two lane halves add by a shuffle, the four row waves by LDS integer adds, and a workgroup adds
//            its nonzero per-(query, slot) totals to the table with unsigned 32-bit atomicAdd (ntotal < 2^31; integer adds have no
//            order, so a count is the same on every repeat)
//   finish   widens the counts to int64; -1 for a slot that counts nothing
// Nothing here is of size [nq, N], and there are no float atomics.
#include "store_scan.h"
#include "../../include/vodhip.h"

namespace vodhip {

namespace {

constexpr unsigned RK_NONE = 0xFFFFFFFFu;  // the key of a slot that counts nothing (flip_f32 of a NaN pattern: no eligible row has it)

// slot (q, j) of the slice -> its local row or -1 (the presence rule of score_ids: listed_row, kernels_listed.hip)
__global__ void __launch_bounds__(256) rank_resolve_kernel(const int64_t* __restrict__ ids, int64_t q_first, int64_t nq, int m, int64_t id_base,
                                                           int64_t ntotal, FilterExtra ex, int* __restrict__ slot_row, int* __restrict__ out_rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * m) return;
    const int64_t q = i / m;
    const int64_t id = ids[q_first * m + i];
    const int64_t local = id - id_base;
    bool present = id >= 0 && local >= 0 && local < ntotal;
    if (present) present = subset_allows(ex, (int)q, (int)local);
    const int row = present ? (int)local : -1;
    slot_row[i] = row;
    if (out_rows != nullptr) out_rows[q_first * m + i] = row;
}

// mini-store row R = qt * mini_rows + j * BN + c  <-  the store row of slot j of query qt * BN + c, or zeros
__global__ void __launch_bounds__(256) rank_gather_kernel(const uint16_t* __restrict__ X, const int* __restrict__ slot_row, int64_t nq, int m, int bn,
                                                          int64_t mini_rows, int64_t total_rows, int64_t dim_pad, uint16_t* __restrict__ mini) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t chunks_per_row = dim_pad / 8;
    if (i >= total_rows * chunks_per_row) return;
    const int64_t R = i / chunks_per_row;
    const int64_t c0 = (i % chunks_per_row) * 8;
    const int64_t qt = R / mini_rows, rho = R % mini_rows;
    const int64_t q = qt * bn + (rho % bn), j = rho / bn;
    int row = -1;
    if (q < nq && j < m) row = slot_row[q * m + j];
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row >= 0) v = *(const uint4*)(X + (int64_t)row * dim_pad + c0);
    *(uint4*)(mini + R * dim_pad + c0) = v;
}

// mini: [n_qtiles][mini_tiles * 256][dim_pad]; Q: the staged queries; out: the caller's scores, already offset to the slice's first slot
template <int DT, int BN, int WN>
__global__ __launch_bounds__(scan_threads(WN), 1)
void rank_pick_kernel(const uint16_t* __restrict__ mini, const uint16_t* __restrict__ Q, int dim_pad, int mini_tiles, int nq, int m,
                      const int* __restrict__ slot_row, float* __restrict__ out) {
    constexpr int TM = SCAN_BM / SCAN_WM, TN = BN / WN, NJ = TN / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int xt = blockIdx.x % mini_tiles, qt = blockIdx.x / mini_tiles;
    const int q0 = qt * BN;
    f32x16 acc[2][NJ];
    scan_k_loop<DT, BN, WN>(mini + ((size_t)qt * mini_tiles + xt) * SCAN_BM * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 31, fh = lane >> 5;
    const int rlane = xt * SCAN_BM + wm * TM + 4 * fh;  // the lane's mini-store row of (block 0, register 0)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        const int q = q0 + col;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rho = scan_lane_row(rlane, i * 16 + r);
                const int slot = rho / BN;
                if ((rho & (BN - 1)) == col && slot < m && q < nq) {
                    const size_t at = (size_t)q * m + slot;
                    out[at] = slot_row[at] >= 0 ? acc[i][j][r] : -__builtin_inff();
                }
            }
    }
}

// slot (q, j) of the slice -> table entry (q / bn * m + j) * bn + q % bn: key, local tie row, count = 0
__global__ void __launch_bounds__(256) rank_prep_kernel(const float* __restrict__ values, const int* __restrict__ slot_row, const int64_t* __restrict__ tie_ids,
                                                        int64_t q_first, int64_t nq, int64_t nq_pad, int m, int bn, int64_t id_base, int64_t ntotal,
                                                        unsigned* __restrict__ tab_key, int* __restrict__ tab_row, unsigned* __restrict__ tab_cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq_pad * m) return;
    const int64_t q = i / m, j = i % m;
    unsigned key = RK_NONE;
    int row = 0;
    if (q < nq) {
        const float t = values[q_first * m + i];
        if (slot_row != nullptr) {  // rank_ids: the slot's own score and row
            const int r = slot_row[i];
            if (r >= 0 && t == t) {
                key = flip_f32(t);
                row = r;
            }
        } else if (t == t) {        // count_above: the caller's threshold; no tie ids = strict
            key = flip_f32(t);
            if (tie_ids != nullptr) {
                const int64_t id = tie_ids[q_first * m + i];
                row = id <= id_base ? 0 : (id - id_base >= ntotal ? (int)ntotal : (int)(id - id_base));
            }
        }
    }
    const int64_t at = ((q / bn) * m + j) * bn + (q % bn);
    tab_key[at] = key;
    tab_row[at] = row;
    tab_cnt[at] = 0u;
}

// X: the store [>= n_xtiles * 256 rows][dim_pad]; Q: the staged queries [n_qtiles * BN][dim_pad]; the slot table [n_qtiles][m][BN]
template <int DT, int BN, int WN, bool SUBSET>
__global__ __launch_bounds__(scan_threads(WN), 1)
void rank_count_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles, int nq,
                       int m, const unsigned* __restrict__ tab_key, const int* __restrict__ tab_row, unsigned* __restrict__ tab_cnt, FilterExtra ex) {
    constexpr int BM = SCAN_BM;
    constexpr int NT = scan_threads(WN);
    constexpr int TM = BM / SCAN_WM, TN = BN / WN, NJ = TN / 32;
    static_assert(3 * VODHIP_RANK_MAX_LISTED * BN * 4 <= scan_ring_bytes(BN), "the slot table reuses the ring");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int qt, xt;
    if (!scan_block_tile(blockIdx.x, n_qtiles, n_xtiles, &qt, &xt)) return;
    const int x0 = xt * BM;
    const int q0 = qt * BN;

    f32x16 acc[2][NJ];
    scan_k_loop<DT, BN, WN>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 31, fh = lane >> 5;

    __syncthreads();  // every wave has read its last fragments: the ring becomes the workgroup's part of the slot table
    unsigned* s_key = reinterpret_cast<unsigned*>(smem);          // [m][BN]
    int* s_row = reinterpret_cast<int*>(s_key + m * BN);          // [m][BN]
    unsigned* s_cnt = reinterpret_cast<unsigned*>(s_row + m * BN);  // [m][BN]
    const size_t tb = (size_t)qt * m * BN;
    for (int i = tid; i < m * BN; i += NT) {
        s_key[i] = tab_key[tb + i];
        s_row[i] = tab_row[tb + i];
        s_cnt[i] = 0u;
    }

    // the lane's keys: 0 for a row that does not count (below every threshold: a counting slot's key is >= key(-inf) - 1 > 0)
    const int rlane = x0 + wm * TM + 4 * fh;  // the lane's row of (block 0, register 0)
    unsigned key[NJ][32];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = q0 + wn * TN + j * 32 + fr;
        // (scan_eligible_mask, spelled out: through the helper this kernel's register allocation differs and every shape of
        // tools/bench_rank_ids.py measured 0.1 - 0.5 % slower than before, profiles/store_scan_refactor.md)
        unsigned mask = 0u;
        if (q < nq) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s = acc[i][j][r];
                    mask |= (scan_lane_row(rlane, i * 16 + r) < ntotal && s == s) ? (1u << (i * 16 + r)) : 0u;
                }
            if constexpr (SUBSET) {  // rolled: one label test per row that is still in
                unsigned m2 = mask;
                while (m2) {
                    const int b = __builtin_ctz(m2);
                    m2 &= m2 - 1;
                    if (!subset_allows(ex, q, scan_lane_row(rlane, b))) mask &= ~(1u << b);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) key[j][i * 16 + r] = (mask & (1u << (i * 16 + r))) ? flip_f32(acc[i][j][r]) : 0u;
    }
    __syncthreads();

#pragma unroll 1
    for (int sl = 0; sl < m; ++sl) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int col = wn * TN + j * 32 + fr;
            const unsigned t = s_key[sl * BN + col];
            const int tr = s_row[sl * BN + col];
            const unsigned te = tr >= x0 + BM ? t - 1u : t;  // the whole tile is below the tie row: key >= t
            unsigned c = 0u;
#pragma unroll
            for (int e = 0; e < 32; ++e) c += key[j][e] > te ? 1u : 0u;
            if (tr > x0 && tr < x0 + BM) {  // the tie row's own tile (te = t): the rows below it that tie
#pragma unroll
                for (int e = 0; e < 32; ++e) {
                    c += (key[j][e] == t && scan_lane_row(rlane, e) < tr) ? 1u : 0u;
                }
            }
            c += __shfl_xor(c, 32, 64);
            if (fh == 0 && c != 0u) atomicAdd(&s_cnt[sl * BN + col], c);
        }
    }
    __syncthreads();
    for (int i = tid; i < m * BN; i += NT) {
        const unsigned c = s_cnt[i];
        if (c != 0u) atomicAdd(&tab_cnt[tb + i], c);
    }
}

__global__ void __launch_bounds__(256) rank_finish_kernel(const unsigned* __restrict__ tab_key, const unsigned* __restrict__ tab_cnt, int64_t q_first,
                                                          int64_t nq, int m, int bn, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq * m) return;
    const int64_t q = i / m, j = i % m;
    const int64_t at = ((q / bn) * m + j) * bn + (q % bn);
    out[q_first * m + i] = tab_key[at] == RK_NONE ? -1ll : (int64_t)tab_cnt[at];
}

template <int DT, int BN, int WN>
hipError_t launch_pick(const RankArgs& a, int64_t q_first, int64_t nq, int64_t nq_pad, hipStream_t stream) {
    const int m = (int)a.m;
    const int n_qtiles = (int)(nq_pad / BN);
    const int mini_tiles = (BN * m + SCAN_BM - 1) / SCAN_BM;
    const int64_t mini_rows = (int64_t)mini_tiles * SCAN_BM, total_rows = mini_rows * n_qtiles;
    const int64_t n = total_rows * (a.dim_pad / 8);
    hipLaunchKernelGGL(rank_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const uint16_t*)a.store, (const int*)a.slot_row, nq, m,
                       BN, mini_rows, total_rows, a.dim_pad, (uint16_t*)a.mini);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return scan_launch<BN, WN>(rank_pick_kernel<DT, BN, WN>, (int64_t)mini_tiles * n_qtiles, stream, (const uint16_t*)a.mini, (const uint16_t*)a.q_stage,
                               (int)a.dim_pad, mini_tiles, (int)nq, m, (const int*)a.slot_row, a.out_score + q_first * a.m);
}

template <int DT, int BN, int WN, bool SUBSET>
hipError_t launch_count(const RankArgs& a, int64_t nq, int64_t nq_pad, int n_tiles, const FilterExtra& ex, hipStream_t stream) {
    const int n_qtiles = (int)(nq_pad / BN);
    const size_t slots = (size_t)nq_pad * (size_t)a.m;
    return scan_launch<BN, WN>(rank_count_kernel<DT, BN, WN, SUBSET>, scan_grid(n_tiles, n_qtiles), stream, (const uint16_t*)a.store,
                               (const uint16_t*)a.q_stage, (int)a.dim_pad, (int)a.ntotal, n_tiles, n_qtiles, (int)nq, (int)a.m, (const unsigned*)a.table,
                               (const int*)(a.table + slots), a.table + 2 * slots, ex);
}

}  // namespace

int64_t rank_mini_rows(int64_t nq_pad, int64_t m) {
    const int64_t bn = nq_pad == 64 ? 64 : 128;
    return (nq_pad / bn) * ((bn * m + SCAN_BM - 1) / SCAN_BM * SCAN_BM);
}

hipError_t launch_rank(const RankArgs& a, int mode, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = scan_nq_pad(nq);
    const int bn = nq_pad == 64 ? 64 : 128;
    const int64_t n_tiles = scan_tiles(a.ntotal);
    if (a.dim_pad % 64 != 0 || a.dim_pad <= 0 || a.ntotal < 0 || a.ntotal >= (1ll << 31) - 512 || nq > (1 << 20) || a.m < 1 ||
        a.m > VODHIP_RANK_MAX_LISTED)
        return hipErrorInvalidValue;
    const int m = (int)a.m;
    const FilterExtra ex = scan_filter_extra(a, q_first);
    if (hipError_t e = launch_scan_stage(a, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
    const bool pick = mode != RANK_MODE_THRESHOLDS;
    if (pick) {
        hipLaunchKernelGGL(rank_resolve_kernel, dim3((unsigned)((nq * m + 255) / 256)), dim3(256), 0, stream, a.ids, q_first, nq, m, a.id_base, a.ntotal,
                           ex, a.slot_row, a.out_rows);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        const hipError_t e = scan_dispatch(a.store_dtype, nq_pad, false, [&](auto dt, auto qn, auto wn, auto) {
            return launch_pick<dt.value, qn.value, wn.value>(a, q_first, nq, nq_pad, stream);
        });
        if (e != hipSuccess) return e;
        if (mode == RANK_MODE_PICK) return hipSuccess;
    }
    const size_t slots = (size_t)nq_pad * (size_t)m;
    hipLaunchKernelGGL(rank_prep_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, pick ? (const float*)a.out_score : a.thresholds,
                       pick ? (const int*)a.slot_row : (const int*)nullptr, pick ? (const int64_t*)nullptr : a.tie_ids, q_first, nq, nq_pad, m, bn,
                       a.id_base, a.ntotal, a.table, (int*)(a.table + slots), a.table + 2 * slots);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (n_tiles > 0) {
        const hipError_t e = scan_dispatch(a.store_dtype, nq_pad, ex.row_label != nullptr, [&](auto dt, auto qn, auto wn, auto subset) {
            return launch_count<dt.value, qn.value, wn.value, subset.value>(a, nq, nq_pad, (int)n_tiles, ex, stream);
        });
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((nq * m + 255) / 256)), dim3(256), 0, stream, (const unsigned*)a.table,
                       (const unsigned*)(a.table + 2 * slots), q_first, nq, m, bn, a.out_count);
    return hipGetLastError();
}

}  // namespace vodhip
