// Exact ranks over the WHOLE store (vodhip_index_rank_ids / vodhip_index_count_above / vodhip_index_scan_score_ids, include/vodhip.h H2r).
//
// Definitions.  A row z is ELIGIBLE for query q when z < ntotal, its scan score s(q, z) is not NaN and the query's subset labels allow it
// (subset_allows, mips_common.h): the rule of the log-partition scan (kernels_partition.hip).  ORDER is the search's:
// key(s) = flip_f32(s) (mips_common.h), so -0.0 and +0.0 are equal, and ties go to the smaller id.  For a threshold t and a tie id r
//   C(q; t, r) = #{ eligible rows z : key(s(q, z)) > key(t)  or  (key(s(q, z)) == key(t) and id_base + z < r) }.
//   count_above   out[q, j] = C(q; thresholds[q, j], tie_ids[q, j]); without tie ids the count is strict (r = -inf); a NaN threshold: -1
//   rank_ids      score[q, j] = the scan's score of row ids[q, j] - the bits a search returns for that pair - and
//                 rank[q, j] = C(q; score[q, j], ids[q, j]): the 0-based position at which a search over the eligible rows returns the
//                 row.  PRESENT is score_ids's rule (id >= 0, id - id_base in [0, ntotal), label allowed); an absent slot is (-1, -inf),
//                 a NaN score rank -1 with the score as computed.  Duplicates are independent slots.
//
// Kernels (one slice of the batch at a time; every table below is a stream-ordered temporary of the slice):
//   stage    queries -> [nq_pad][dim_pad] of the store dtype, rounded as a search rounds them (store_bits: saturating), zero padded
//   resolve  listed ids -> local rows (-1 = absent)
//   gather   the present listed rows of a query tile -> a MINI-STORE [BN * m rows, padded to 256][dim_pad]: row j * BN + c holds the row
//            of slot j of the tile's query column c; absent slots are zero rows
//   pick     the K loop below over the mini-store's tiles against that query tile only.  An MFMA output element depends on its A row
//            and its B column alone, and the K loop adds the dim_pad / 16 k-steps in the scan's order, so element (row of slot (q, j),
//            column q) is the scan's score of that pair, bit for bit; the epilogue writes those BN * m elements and drops the rest
//   prep     (score, local row) or (threshold, tie id) -> the slot table: key(t) and the LOCAL tie row r in [0, ntotal] (0 = strict),
//            laid out [query tile][slot][BN] so that a workgroup copies its part to LDS in one coalesced pass; a slot that counts nothing
//            (absent, NaN, a padding query) holds key 0xFFFFFFFF, which no eligible row exceeds; the counts are cleared
//   count    the log-partition scan's geometry (256-row tile x 64 | 128 queries, LDS-DMA ring, XCD-aware tile order, SUBSET a template
//            flag) with an integer epilogue: a lane turns its 32 accumulators of a query column into keys (0 for an ineligible row: below
//            every threshold) and, slot by slot (rolled), counts key > te.  In every tile but the one that holds the tie row all rows lie
//            on one side of it: below r the tie test folds into the threshold (key >= t is key > t - 1 on the integer key), above it the
//            test is strict - one compare and one add per (accumulator, slot).  Only the tie row's own tile adds the per-row test
//            key == t and row < r.  The two lane halves add by a shuffle, the four row waves by LDS integer adds, and a workgroup adds
//            its nonzero per-(query, slot) totals to the table with unsigned 32-bit atomicAdd (ntotal < 2^31; integer adds have no
//            order, so a count is the same on every repeat)
//   finish   widens the counts to int64; -1 for a slot that counts nothing
// Nothing here is of size [nq, N], and there are no float atomics.
#include "mips_common.h"
#include "../../include/vodhip.h"

#include <type_traits>

namespace vodhip {

namespace {

constexpr int RK_BM = 256;     // corpus rows of a tile
constexpr int RK_WM = 4;       // row waves
constexpr int RK_NSTAGE = 3;   // LDS ring depth
constexpr unsigned RK_NONE = 0xFFFFFFFFu;  // the key of a slot that counts nothing (flip_f32 of a NaN pattern: no eligible row has it)

__global__ void __launch_bounds__(256) rank_stage_kernel(const void* __restrict__ q_src, int q_dtype, int64_t q_first, int64_t nq, int64_t dim,
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

// The K loop of partition_scan_kernel (kernels_partition.hip), instruction for instruction: LDS-DMA with the source-side XOR swizzle,
// 3-slot ring, v_mfma_f32_32x32x16 with the rows as A and the queries as B.  X: the first of 256 rows [dim_pad]; Q: the first of BN
// staged queries.  On return every wave may still be reading the ring: a __syncthreads() precedes any reuse of `smem`.
// C layout: col = lane & 31 (query), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
template <int DT, int BN, int WN>
__device__ __forceinline__ void rank_k_loop(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, char* smem,
                                            f32x16 (&acc)[2][BN / WN / 32]) {
    constexpr int BM = RK_BM, WM = RK_WM, NSTAGE = RK_NSTAGE;
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

// mini: [n_qtiles][mini_tiles * 256][dim_pad]; Q: the staged queries; out: the caller's scores, already offset to the slice's first slot
template <int DT, int BN, int WN>
__global__ __launch_bounds__(RK_WM* WN * 64, 1)
void rank_pick_kernel(const uint16_t* __restrict__ mini, const uint16_t* __restrict__ Q, int dim_pad, int mini_tiles, int nq, int m,
                      const int* __restrict__ slot_row, float* __restrict__ out) {
    constexpr int TM = RK_BM / RK_WM, TN = BN / WN, NJ = TN / 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int xt = blockIdx.x % mini_tiles, qt = blockIdx.x / mini_tiles;
    const int q0 = qt * BN;
    f32x16 acc[2][NJ];
    rank_k_loop<DT, BN, WN>(mini + ((size_t)qt * mini_tiles + xt) * RK_BM * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 31, fh = lane >> 5;
    const int rlane = xt * RK_BM + wm * TM + 4 * fh;  // the lane's mini-store row of (block 0, register 0)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = wn * TN + j * 32 + fr;
        const int q = q0 + col;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rho = rlane + i * 32 + (r & 3) + 8 * (r >> 2);
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
__global__ __launch_bounds__(RK_WM* WN * 64, 1)
void rank_count_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles, int nq,
                       int m, const unsigned* __restrict__ tab_key, const int* __restrict__ tab_row, unsigned* __restrict__ tab_cnt, FilterExtra ex) {
    constexpr int BM = RK_BM, WM = RK_WM;
    constexpr int NT = WM * WN * 64;
    constexpr int TM = BM / WM, TN = BN / WN, NJ = TN / 32;
    static_assert(3 * VODHIP_RANK_MAX_LISTED * BN * 4 <= RK_NSTAGE * (BM + BN) * 128, "the slot table reuses the ring");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // XCD-aware tile order (as partition_scan_kernel): the n_qtiles workgroups that re-read one corpus tile land on one XCD back to back
    const int bid = blockIdx.x;
    const int xcd = bid & 7, jj = bid >> 3;
    const int qt = jj % n_qtiles;
    const int xt = (jj / n_qtiles) * 8 + xcd;
    if (xt >= n_xtiles) return;
    const int x0 = xt * BM;
    const int q0 = qt * BN;

    f32x16 acc[2][NJ];
    rank_k_loop<DT, BN, WN>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

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
        unsigned mask = 0u;
        if (q < nq) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
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
                    const int row = rlane + (e >> 4) * 32 + (e & 3) + 8 * ((e & 15) >> 2);
                    c += (key[j][e] == t && row < tr) ? 1u : 0u;
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
    const int mini_tiles = (BN * m + RK_BM - 1) / RK_BM;
    const int64_t mini_rows = (int64_t)mini_tiles * RK_BM, total_rows = mini_rows * n_qtiles;
    const int64_t n = total_rows * (a.dim_pad / 8);
    hipLaunchKernelGGL(rank_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const uint16_t*)a.store, (const int*)a.slot_row, nq, m,
                       BN, mini_rows, total_rows, a.dim_pad, (uint16_t*)a.mini);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    constexpr int threads = RK_WM * WN * 64;
    constexpr size_t lds = (size_t)RK_NSTAGE * (RK_BM + BN) * 128;
    auto kern = rank_pick_kernel<DT, BN, WN>;
    if (hipError_t e = allow_dynamic_lds((const void*)kern, (int)lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(mini_tiles * n_qtiles)), dim3(threads), lds, stream, (const uint16_t*)a.mini, (const uint16_t*)a.q_stage,
                       (int)a.dim_pad, mini_tiles, (int)nq, m, (const int*)a.slot_row, a.out_score + q_first * a.m);
    return hipGetLastError();
}

template <int DT, int BN, int WN, bool SUBSET>
hipError_t launch_count(const RankArgs& a, int64_t nq, int64_t nq_pad, int n_tiles, const FilterExtra& ex, hipStream_t stream) {
    const int n_qtiles = (int)(nq_pad / BN);
    const int64_t grid = (int64_t)((n_tiles + 7) / 8) * 8 * n_qtiles;
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    constexpr int threads = RK_WM * WN * 64;
    constexpr size_t lds = (size_t)RK_NSTAGE * (RK_BM + BN) * 128;
    auto kern = rank_count_kernel<DT, BN, WN, SUBSET>;
    if (hipError_t e = allow_dynamic_lds((const void*)kern, (int)lds); e != hipSuccess) return e;
    const size_t slots = (size_t)nq_pad * (size_t)a.m;
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(threads), lds, stream, (const uint16_t*)a.store, (const uint16_t*)a.q_stage, (int)a.dim_pad,
                       (int)a.ntotal, n_tiles, n_qtiles, (int)nq, (int)a.m, (const unsigned*)a.table, (const int*)(a.table + slots),
                       a.table + 2 * slots, ex);
    return hipGetLastError();
}

template <int DT>
hipError_t launch_pick_dt(const RankArgs& a, int64_t q_first, int64_t nq, int64_t nq_pad, hipStream_t stream) {
    return nq_pad == 64 ? launch_pick<DT, 64, 1>(a, q_first, nq, nq_pad, stream) : launch_pick<DT, 128, 2>(a, q_first, nq, nq_pad, stream);
}

template <int DT>
hipError_t launch_count_dt(const RankArgs& a, int64_t nq, int64_t nq_pad, int n_tiles, const FilterExtra& ex, hipStream_t stream) {
    const bool subset = ex.row_label != nullptr;
    if (nq_pad == 64)
        return subset ? launch_count<DT, 64, 1, true>(a, nq, nq_pad, n_tiles, ex, stream) : launch_count<DT, 64, 1, false>(a, nq, nq_pad, n_tiles, ex, stream);
    return subset ? launch_count<DT, 128, 2, true>(a, nq, nq_pad, n_tiles, ex, stream) : launch_count<DT, 128, 2, false>(a, nq, nq_pad, n_tiles, ex, stream);
}

}  // namespace

int64_t rank_nq_pad(int64_t nq) { return nq <= 64 ? 64 : (nq + 127) / 128 * 128; }
int64_t rank_mini_rows(int64_t nq_pad, int64_t m) {
    const int64_t bn = nq_pad == 64 ? 64 : 128;
    return (nq_pad / bn) * ((bn * m + RK_BM - 1) / RK_BM * RK_BM);
}

hipError_t launch_rank(const RankArgs& a, int mode, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    const int64_t nq_pad = rank_nq_pad(nq);
    const int bn = nq_pad == 64 ? 64 : 128;
    const int64_t n_tiles = (a.ntotal + RK_BM - 1) / RK_BM;
    if (a.dim_pad % 64 != 0 || a.dim_pad <= 0 || a.ntotal < 0 || a.ntotal >= (1ll << 31) - 512 || nq > (1 << 20) || a.m < 1 ||
        a.m > VODHIP_RANK_MAX_LISTED)
        return hipErrorInvalidValue;
    const int m = (int)a.m;
    FilterExtra ex;
    if (a.q_label != nullptr) {
        ex.row_label = a.row_label;
        ex.q_label = a.q_label + (size_t)q_first * a.n_qlab;
        ex.n_qlab = a.n_qlab;
    }
    {
        const int64_t n = nq_pad * (a.dim_pad / 8);
        hipLaunchKernelGGL(rank_stage_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.q_src, a.q_dtype, q_first, nq, a.dim,
                           (uint16_t*)a.q_stage, a.store_dtype, nq_pad, a.dim_pad);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    const bool pick = mode != RANK_MODE_THRESHOLDS;
    if (pick) {
        hipLaunchKernelGGL(rank_resolve_kernel, dim3((unsigned)((nq * m + 255) / 256)), dim3(256), 0, stream, a.ids, q_first, nq, m, a.id_base, a.ntotal,
                           ex, a.slot_row, a.out_rows);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        const hipError_t e = a.store_dtype == 0 ? launch_pick_dt<0>(a, q_first, nq, nq_pad, stream) : launch_pick_dt<1>(a, q_first, nq, nq_pad, stream);
        if (e != hipSuccess) return e;
        if (mode == RANK_MODE_PICK) return hipSuccess;
    }
    const size_t slots = (size_t)nq_pad * (size_t)m;
    hipLaunchKernelGGL(rank_prep_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, stream, pick ? (const float*)a.out_score : a.thresholds,
                       pick ? (const int*)a.slot_row : (const int*)nullptr, pick ? (const int64_t*)nullptr : a.tie_ids, q_first, nq, nq_pad, m, bn,
                       a.id_base, a.ntotal, a.table, (int*)(a.table + slots), a.table + 2 * slots);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (n_tiles > 0) {
        const hipError_t e = a.store_dtype == 0 ? launch_count_dt<0>(a, nq, nq_pad, (int)n_tiles, ex, stream)
                                                : launch_count_dt<1>(a, nq, nq_pad, (int)n_tiles, ex, stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)((nq * m + 255) / 256)), dim3(256), 0, stream, (const unsigned*)a.table,
                       (const unsigned*)(a.table + 2 * slots), q_first, nq, m, bn, a.out_count);
    return hipGetLastError();
}

}  // namespace vodhip
