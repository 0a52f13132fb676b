// Range scan over the WHOLE store (vodhip_index_range_search, include/vodhip.h H2g): WHICH rows score above a per-query threshold.
//
// Definitions.  Scores, ELIGIBLE rows and ORDER are the rank calls' (kernels_rank.hip): key(s) = flip_f32(s), ties go to the smaller id.
// For a threshold t and a tie id r the result of query q is the set
//   R(q) = { eligible rows z : key(s(q, z)) > key(t)  or  (key(s(q, z)) == key(t) and id_base + z < r) }
// - the set count_above counts - as a CSR list: lims [nq + 1], and per hit the scan's score and the global id, ids ASCENDING within a
// query.  A NaN threshold gives an empty list.
//
// Kernels (one slice of the batch at a time; the tables are stream-ordered temporaries of the slice):
//   stage    queries -> [nq_pad][dim_pad] of the store dtype (launch_scan_stage)
//   prep     (threshold, tie id) -> the threshold and the LOCAL tie row in [0, ntotal] (0 = strict) per query, as rank_prep_kernel maps it;
//            a query that selects nothing (a NaN threshold, padding) holds NaN
//   scan     ONE instantiation per (DT, BN, WN, SUBSET), launched twice with a mode word, so that both passes evaluate the predicate
//            with the same instructions.  After the K loop a lane forms, per query column, the 32-bit mask of its rows in R(q).  The
//            predicate is rank_count_kernel's, on the floats: for scores and thresholds that are not NaN, key(s) > key(t) is s > t and
//            key(s) == key(t) is s == t (both zeros equal), so the rank scan's folding of the tie rule into the threshold (key > t - 1,
//            i.e. key >= t, in a tile wholly below the tie row, key > t above it) is s >= t or s > t, chosen per lane, and only the tie
//            row's own tile adds the per-row test s == t and row < r.  A NaN score or threshold fails every compare, which is the
//            eligibility rule and the empty list; rows past ntotal are cleared in the last tile, subset labels are tested on the rows that
//            are in so far.  Three vector instructions per accumulator: the epilogue is not hidden - one workgroup per CU.
//            The two lanes of a column exchange masks by one shuffle and interleave them
//            into the wave's 64-bit mask in ROW ORDER: by scan_lane_row the row within a 32-row block is (r & 3) + 4 h + 8 (r >> 2), so
//            nibble n of the ordered block mask is nibble n >> 1 of lane half n & 1 (range_row_order).
//     count  the four row waves put their popcounts into LDS; the workgroup stores ONE int32 per (query, tile) into the table
//            [nq_pad][n_tiles].  Nothing else leaves the workgroup; there are no atomics.
//     emit   a workgroup none of whose queries has a hit in its tile leaves before its K loop (a uniform test).  Otherwise it recomputes
//            the masks; a row's position is lims[q] + the tile's offset + the hits of lower row waves + the popcount of the lower bits
//            of the 64-bit mask.  (score, id_base + row) go there with plain stores; a position at or past the capacity is not
//            written.  A status word counts (query, tile) pairs whose emit count differs from the stored one (expected: never).
//   prefix   one workgroup per query: the exclusive scan over its tiles, in place (a tile's count stays readable as the difference to
//            the next offset, the last tile's to the query's total)
//   lims     one workgroup: the scan of the slice's totals into lims, carrying lims[first query of the slice] of the slice before
// The whole result is a function of the store and the query alone: the same in any batch, any slice and on every repeat.
#include "store_scan.h"
#include "../../include/vodhip.h"

namespace vodhip {

namespace {

struct RangeScan {
    int emit;                  // 0 = count pass, 1 = emit pass
    const float* thr;          // [nq_pad] the threshold; NaN = the query selects nothing
    const int* tie_row;        // [nq_pad] the local tie row in [0, ntotal]
    int* table;                // [nq_pad][n_tiles]: count pass: the counts (written); emit pass: the exclusive offsets
    const unsigned* total;     // emit: [nq_pad] hits per query
    const int64_t* lims;       // emit: the caller's lims, offset to the slice's first query
    float* out_scores;         // emit
    int64_t* out_ids;
    int64_t capacity;
    int64_t id_base;
    unsigned* status;          // emit: RGS_* words
};

// 16-bit abcd -> 32-bit 0a0b0c0d (nibbles)
__device__ __forceinline__ unsigned range_spread_nibbles(unsigned x) {
    x = (x | (x << 8)) & 0x00FF00FFu;
    return (x | (x << 4)) & 0x0F0F0F0Fu;
}

// h0 / h1: the 32-bit masks (bit 16 i + r) of the column's lane halves 0 / 1 -> bit 32 i + w = row 32 i + w of the wave's 64 rows
__device__ __forceinline__ unsigned long long range_row_order(unsigned h0, unsigned h1) {
    const unsigned lo = range_spread_nibbles(h0 & 0xFFFFu) | (range_spread_nibbles(h1 & 0xFFFFu) << 4);
    const unsigned hi = range_spread_nibbles(h0 >> 16) | (range_spread_nibbles(h1 >> 16) << 4);
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

// the stored hits of (query, tile) behind the prefix kernel
__device__ __forceinline__ int range_tile_count(const RangeScan& rs, int q, int xt, int n_xtiles) {
    const int* p = rs.table + (size_t)q * n_xtiles;
    return (xt + 1 < n_xtiles ? p[xt + 1] : (int)rs.total[q]) - p[xt];
}

__global__ void __launch_bounds__(256) range_prep_kernel(const float* __restrict__ thresholds, const int64_t* __restrict__ tie_ids, int64_t q_first, int64_t nq,
                                                         int64_t nq_pad, int64_t id_base, int64_t ntotal, float* __restrict__ thr, int* __restrict__ tie_row) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq_pad) return;
    float k = __builtin_nanf("");
    int row = 0;
    if (q < nq) {
        const float t = thresholds[q_first + q];
        if (t == t) {
            k = t;
            if (tie_ids != nullptr) {
                const int64_t id = tie_ids[q_first + q];
                row = id <= id_base ? 0 : (id - id_base >= ntotal ? (int)ntotal : (int)(id - id_base));
            }
        }
    }
    thr[q] = k;
    tie_row[q] = row;
}

// X: the store [>= n_xtiles * 256 rows][dim_pad]; Q: the staged queries [n_qtiles * BN][dim_pad]
template <int DT, int BN, int WN, bool SUBSET>
__global__ __launch_bounds__(scan_threads(WN), 1)
void range_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles, int nq,
                       RangeScan rs, FilterExtra ex) {
    constexpr int BM = SCAN_BM, WM = SCAN_WM;
    constexpr int TM = BM / WM, TN = BN / WN, NJ = TN / 32;
    static_assert(WM * BN * (int)sizeof(int) <= scan_ring_bytes(BN) / SCAN_NSTAGE, "the wave counts reuse the first ring slot");
    static_assert(BN <= scan_threads(WN), "one thread per query column");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int qt, xt;
    if (!scan_block_tile(blockIdx.x, n_qtiles, n_xtiles, &qt, &xt)) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 31, fh = lane >> 5;
    const int x0 = xt * BM;
    const int q0 = qt * BN;

    if (rs.emit) {  // a tile that holds no query's hits: out before the K loop (uniform over the workgroup)
        const bool hit = tid < BN && range_tile_count(rs, q0 + tid, xt, n_xtiles) != 0;
        if (!__syncthreads_or(hit)) {
            if (tid == 0) atomicAdd(&rs.status[RGS_SKIPPED], 1u);
            return;
        }
    }

    // the lane's thresholds, read ahead of the K loop: one workgroup per CU, so a load behind the loop would wait with nothing to hide it
    float thr[NJ];
    int trow[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        thr[j] = rs.thr[q0 + wn * TN + j * 32 + fr];
        trow[j] = rs.tie_row[q0 + wn * TN + j * 32 + fr];
    }

    f32x16 acc[2][NJ];
    scan_k_loop<DT, BN, WN>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

    __syncthreads();  // every wave has read its last fragments: the first ring slot becomes the wave counts
    int* s_cnt = reinterpret_cast<int*>(smem);  // [WM][BN]
    const int rlane = x0 + wm * TM + 4 * fh;    // the lane's row of (block 0, register 0)
    unsigned mine[NJ];
    unsigned long long ordered[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        const int q = q0 + col;
        unsigned mask = 0u;
        if (q < nq) {
            const float t = thr[j];
            const int tr = trow[j];
            const bool below = tr >= x0 + BM;  // the whole tile is below the tie row: ties count (key >= key(t), the rank scan's t - 1)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float s = acc[i][j][r];
                    mask |= (below ? s >= t : s > t) ? (1u << (i * 16 + r)) : 0u;
                }
            if (tr > x0 && tr < x0 + BM) {  // the tie row's own tile: the rows below it that tie
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        mask |= (acc[i][j][r] == t && scan_lane_row(rlane, i * 16 + r) < tr) ? (1u << (i * 16 + r)) : 0u;
            }
            if (x0 + BM > ntotal) {  // the last tile (uniform): rows past ntotal are zero or stale
#pragma unroll
                for (int b = 0; b < 32; ++b) mask &= scan_lane_row(rlane, b) < ntotal ? ~0u : ~(1u << b);
            }
            if constexpr (SUBSET) {  // rolled: one label test per row that is in so far
                unsigned m2 = mask;
                while (m2) {
                    const int b = __builtin_ctz(m2);
                    m2 &= m2 - 1;
                    if (!subset_allows(ex, q, scan_lane_row(rlane, b))) mask &= ~(1u << b);
                }
            }
        }
        const unsigned other = __shfl_xor(mask, 32, 64);
        mine[j] = mask;
        ordered[j] = range_row_order(fh ? other : mask, fh ? mask : other);
        if (fh == 0) s_cnt[wm * BN + col] = __popcll(ordered[j]);
    }
    __syncthreads();

    int sum = 0;  // (threads below BN: the tile's hits of query column tid)
    if (tid < BN) {
#pragma unroll
        for (int w = 0; w < WM; ++w) sum += s_cnt[w * BN + tid];
    }
    if (!rs.emit) {
        if (tid < BN) rs.table[(size_t)(q0 + tid) * n_xtiles + xt] = sum;
        return;
    }
    if (tid < BN && sum != range_tile_count(rs, q0 + tid, xt, n_xtiles)) atomicAdd(&rs.status[RGS_SELFCHECK], 1u);

#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        const int q = q0 + col;
        if (mine[j] == 0u) continue;  // (nothing for a query past nq: its mask is 0)
        int64_t base = rs.lims[q] + (int64_t)rs.table[(size_t)q * n_xtiles + xt];
        for (int w = 0; w < wm; ++w) base += s_cnt[w * BN + col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if ((mine[j] >> (i * 16 + r)) & 1u) {
                    const int p = 32 * i + 8 * (r >> 2) + 4 * fh + (r & 3);  // the row within the wave's 64
                    const int64_t pos = base + __popcll(ordered[j] & ((1ull << p) - 1ull));
                    if (pos < rs.capacity) {
                        rs.out_scores[pos] = acc[i][j][r];
                        rs.out_ids[pos] = rs.id_base + (int64_t)scan_lane_row(rlane, i * 16 + r);
                    }
                }
            }
    }
}

// One workgroup per staged query: table[q][0 .. n_tiles) counts -> exclusive offsets in place; total[q] = their sum (< 2^31: ntotal is)
constexpr int PF_T = 256;
__global__ void __launch_bounds__(PF_T) range_prefix_kernel(int* __restrict__ table, int n_tiles, unsigned* __restrict__ total) {
    constexpr int NW = PF_T / 64;
    __shared__ int s_wave[2][NW];  // the waves' sums of a chunk; two copies, so that one barrier per chunk is enough
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int* p = table + (size_t)blockIdx.x * n_tiles;
    int carry = 0;
    int v = tid < n_tiles ? p[tid] : 0;
    int it = 0;
    for (int b = 0; b < n_tiles; b += PF_T, it ^= 1) {  // (uniform)
        const int t = b + tid;
        const int next = t + PF_T < n_tiles ? p[t + PF_T] : 0;  // the next chunk's count: in flight during this chunk's scan
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int x = __shfl_up(incl, d, 64);
            if (lane >= d) incl += x;
        }
        if (lane == 63) s_wave[it][wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int x = s_wave[it][k];
            all += x;
            before += k < wave ? x : 0;
        }
        if (t < n_tiles) p[t] = carry + before + incl - v;
        carry += all;
        v = next;
    }
    if (tid == 0) total[blockIdx.x] = (unsigned)carry;
}

// One workgroup: lims[i + 1] = lims[0] + total[0] + .. + total[i] for the slice's nq <= 1024 queries; the first slice sets lims[0] = 0
constexpr int LM_T = 1024;
__global__ void __launch_bounds__(LM_T) range_lims_kernel(const unsigned* __restrict__ total, int nq, int first, int64_t* __restrict__ lims) {
    __shared__ int64_t s[LM_T];
    const int tid = threadIdx.x;
    s[tid] = tid < nq ? (int64_t)total[tid] : 0;
    __syncthreads();
    for (int d = 1; d < LM_T; d <<= 1) {
        const int64_t x = tid >= d ? s[tid - d] : 0;
        __syncthreads();
        s[tid] += x;
        __syncthreads();
    }
    const int64_t base = first ? 0 : lims[0];  // (lims[0] is written by the first slice alone, where nobody reads it)
    if (tid < nq) lims[tid + 1] = base + s[tid];
    if (first && tid == 0) lims[0] = 0;
}

}  // namespace

hipError_t launch_range(const RangeArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = scan_nq_pad(nq);
    const int64_t n_tiles = scan_tiles(a.ntotal);
    if (a.dim_pad % 64 != 0 || a.dim_pad <= 0 || a.ntotal < 0 || a.ntotal >= (1ll << 31) - 512 || nq > LM_T) return hipErrorInvalidValue;
    const FilterExtra ex = scan_filter_extra(a, q_first);
    if (hipError_t e = launch_scan_stage(a, q_first, nq, nq_pad, stream); e != hipSuccess) return e;
    float* thr = (float*)a.words;
    int* tie_row = (int*)(a.words + nq_pad);
    unsigned* total = a.words + 2 * nq_pad;
    hipLaunchKernelGGL(range_prep_kernel, dim3((unsigned)((nq_pad + 255) / 256)), dim3(256), 0, stream, a.thresholds, a.tie_ids, q_first, nq, nq_pad, a.id_base,
                       a.ntotal, thr, tie_row);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    RangeScan rs;
    rs.emit = 0;
    rs.thr = thr;
    rs.tie_row = tie_row;
    rs.table = a.table;
    rs.total = total;
    rs.lims = a.lims + q_first;
    rs.out_scores = a.out_scores;
    rs.out_ids = a.out_ids;
    rs.capacity = a.capacity;
    rs.id_base = a.id_base;
    rs.status = a.status;
    auto scan = [&]() {
        return scan_dispatch(a.store_dtype, nq_pad, ex.row_label != nullptr, [&](auto dt, auto bn, auto wn, auto subset) {
            const int n_qtiles = (int)(nq_pad / bn.value);
            return scan_launch<bn.value, wn.value>(range_scan_kernel<dt.value, bn.value, wn.value, subset.value>, scan_grid((int)n_tiles, n_qtiles), stream,
                                                   (const uint16_t*)a.store, (const uint16_t*)a.q_stage, (int)a.dim_pad, (int)a.ntotal, (int)n_tiles, n_qtiles,
                                                   (int)nq, rs, ex);
        });
    };
    if (n_tiles > 0)
        if (hipError_t e = scan(); e != hipSuccess) return e;
    hipLaunchKernelGGL(range_prefix_kernel, dim3((unsigned)nq_pad), dim3(PF_T), 0, stream, a.table, (int)n_tiles, total);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(range_lims_kernel, dim3(1), dim3(LM_T), 0, stream, (const unsigned*)total, (int)nq, q_first == 0 ? 1 : 0, a.lims + q_first);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (a.out_scores != nullptr && n_tiles > 0) {
        rs.emit = 1;
        if (hipError_t e = scan(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace vodhip
