// libvodhip -- the FILTER stage on the guide's "256^2 8-phase" K loop (round 5).  Tile 14 = the production kernel of batches with two or
// more query tiles (C3: -2.4 %, C4 shard: -4.0 % against tile 8, profiles/r05_ab_8phase.txt); KEEPB0 = false is the guide's read
// schedule (B0 fragments re-read in phase 4), experiment builds only.
//
// Same tile, wave layout (8 waves = 2 x 4 of 128 x 64), fragment maps (v_mfma_f32_16x16x32), epilogue, survivor lists and stage
// order as the persistent kernel of kernels_mips.hip; the K loop is rebuilt after /opt/skills/guides/cdna_hip_programming.md
// ("The 256^2 8-phase template", lines 376-437):
//   * LDS operands: 8 half-tile buffers of 16 KB (2 K-tiles x [A0 | B1 | A1 | B0]; a half-tile = 128 rows x 64 k) = 128 KB.
//     A-half h = the rows {wm*128 + h*64 .. +63} of both wave rows, B-half h = the queries {wn*64 + h*32 .. +31} of all four wave
//     columns, so that a phase's register sub-tile is one quadrant (64 rows x 32 queries) of EVERY wave's 128 x 64 output;
//   * one K-tile (64 deep) = 4 phases, one C quadrant x K = 64 = 16 MFMAs per wave each:
//       qd 0: (m0, n0)  ds_read A0 (8) + B0 (4)      qd 1: (m0, n1)  B1 (4)      qd 2: (m1, n1)  A1 (8)      qd 3: (m1, n0)  B0 (4) again
//     every phase = [ds_read the sub-tile | 2 x global_load_lds of ONE half-tile, 7 half-tiles ahead | lgkmcnt(0)] s_barrier
//     [s_setprio 1 | 16 MFMA | s_setprio 0] s_barrier;
//   * the two wave rows run staggered by one barrier (wm = 1 takes an extra s_barrier up front): on every SIMD the read section of
//     one wave runs beside the MFMA section of the other;
//   * `s_waitcnt vmcnt(6)` once per K-tile, in phase qd 3 (never 0 in the steady state): with a lead of 7 half-tiles everything but
//     the three youngest half-tiles has landed, i.e. the whole NEXT K-tile; it is read from the next phase on (one barrier later for
//     the wave row that runs ahead, two for the other);
//   * WAR: the half-tile staged in phase g overwrites the buffer last read in phase g - 1; those reads are retired (lgkmcnt(0)) BEFORE
//     that phase's first barrier, and the stage is issued after the phase's second barrier of the wave row that runs ahead - i.e. after
//     the first barrier of the other row, which has retired its reads as well.
// The half-tile stream continues across corpus tiles (the first half-tiles of the next tile are in flight during a tile's last
// K-tile and its epilogue).  A flush of the survivor lists (global loads / atomics / stores, rare) drains vmcnt afterwards, so the
// counted waits only ever count LDS-DMA pieces.  Results are bit-identical to tile 8: same products, same summation order.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mips_common.h"

namespace vodhip {

namespace {
constexpr int P8_HALF = 128 * 128;         // one half-tile: 128 rows x 128 B
constexpr int P8_OPERANDS = 8 * P8_HALF;   // 128 KB
constexpr int P8_WL_CAP = 256;             // records per wave list
constexpr int P8_WL_FLUSH = 176;
constexpr int P8_TRANSPOSE_MAX_LANES = 2;  // query blocks in the loop with at most this many lanes holding survivors take the transpose path
constexpr int P8_XPOSE = 8 * 2 * 32 * 4;   // survivor transpose: per wave 2 slots of a lane's 32 sums of one query (2 KB)
constexpr int P8_DRAIN_RECORDS = 112;      // the ring's drain: records per LDS-DMA copy (14 KB + 448 B of metadata of a wave's 16 KB)
constexpr int P8_SC1 = 16;                 // cache-policy immediate `sc1` (device scope): the load misses the CU's L1
static_assert(P8_DRAIN_RECORDS % 8 == 0 && P8_DRAIN_RECORDS * 132 + 256 <= P8_OPERANDS / 8, "drain staging");
constexpr int P8_LDS = P8_OPERANDS + 8 * P8_WL_CAP * 12 + P8_XPOSE;
static_assert(P8_LDS <= 160 * 1024, "LDS budget");
}  // namespace

// KEEPB0 (tile 14): the B0 fragments stay in registers from phase qd 0 to qd 3 (16 more VGPRs, 4 fewer ds_read_b128 per K-tile)
// LEAD = half-tiles the LDS-DMA stream runs ahead of the phase that issues it (7 = the guide's; 6 / 5: experiment builds)
template <int DT, bool SUBSET, bool KEEPB0, int LEAD = 7>
__global__ __launch_bounds__(512, 2) void mips_filter8ph_kernel(
    const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int row_begin, int row_end, int n_xtiles,
    int n_qtiles, int nq, const float* __restrict__ thr_s, const key_t64* __restrict__ thr_key, key_t64* __restrict__ cand,
    unsigned int* __restrict__ cnt, int cap, unsigned int* __restrict__ overflow, FilterExtra ex, float* __restrict__ ring, int ring_cap) {
    constexpr int BM = 256, BN = 256, WN = 4, NWAVES = 8, TM = 128, TN = 64, MB = TM / 16, NB16 = TN / 16, ROW_BYTES = 128;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bid = blockIdx.x;
    const int xcd = bid & 7, jj = bid >> 3;
    const int qt = jj % n_qtiles;
    const int xt0 = (jj / n_qtiles) * 8 + xcd;
    const int xt_step = (int)gridDim.x / n_qtiles;  // gridDim.x is a multiple of 8 * n_qtiles
    if (xt0 >= n_xtiles) return;
    const int n_my = (n_xtiles - 1 - xt0) / xt_step + 1;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int q0 = qt * BN;
    const int nk = dim_pad / 64;  // K-tiles per corpus tile
    const size_t row_stride = (size_t)dim_pad * 2;

    // ---- LDS-DMA sources.  Wave w stages LDS rows [16 w, 16 w + 16) of every half-tile: two wave-instructions of 8 rows x 128 B.
    // LDS row lr of A-half h is tile row (lr >> 6) * 128 + h * 64 + (lr & 63); of B-half h query (lr >> 5) * 64 + h * 32 + (lr & 31).
    // 16-byte chunk c of LDS row lr sits at slot c ^ ((lr >> 1) & 7) (applied on the source address; fragment reads conflict-free).
    const int st_row = lane >> 3, st_slot = lane & 7;
    int super_cur = ex.perm_mod > 0 ? filter_tile_row0(ex, row_begin, xt0, BM) / BM : 0;
    int super_epi = super_cur;
    const int perm_inc = ex.perm_mod > 0 ? (int)(((unsigned long long)xt_step * (unsigned long long)ex.perm_mul) % (unsigned long long)ex.perm_mod) : 0;
    const char* a_src[2];
    const char* b_src[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int sw = (u * 4 + (st_row >> 1)) & 7;
        const int arow = (wave >> 2) * 128 + (wave & 3) * 16 + u * 8 + st_row;  // + h * 64
        const int brow = (wave >> 1) * 64 + (wave & 1) * 16 + u * 8 + st_row;   // + h * 32
        a_src[u] = (const char*)X + ((size_t)filter_tile_row0(ex, row_begin, xt0, BM) + arow) * row_stride + ((st_slot ^ sw) << 4);
#ifdef VODHIP_ABLATION  // diagnostic builds, kflags bit 128: every q-tile stages the rows of q-tile 0 (an XCD's query working set shrinks to 256 rows; bytes / timing only)
        const int q0_stage = (ex.flags & (128 << 8)) ? 0 : q0;
#else
        const int q0_stage = q0;
#endif
        b_src[u] = (const char*)Q + (size_t)(q0_stage + brow) * row_stride + ((st_slot ^ sw) << 4);
    }
    const size_t a_half_step = 64 * row_stride, b_half_step = 32 * row_stride;
    const size_t tile_step_bytes = (size_t)xt_step * BM * row_stride;

    // the issue stream: half-tile n = 4 * (stream K-tile) + kind, kinds in staging order [A0, B1, A1, B0]; LDS buffer = n & 7.
    // The kind is a COMPILE-TIME argument (phase qd stages kind (qd + 3) & 3): the four source pointers stay in registers (indexed
    // by a run-time kind the compiler keeps them in scratch and puts a vmcnt(0) in front of every LDS-DMA).
    const bool corpus_nt = (ex.flags & FILTER_FLAG_CORPUS_NT) != 0;
    int s_t = 0, s_it = 0, s_par = 0;  // stream K-tile: index inside its corpus tile, corpus tile, buffer parity
    int issued = 0;                     // half-tiles staged so far
    bool s_active = n_my > 0;
    auto stage = [&](auto kind_tag) {
        constexpr int KIND = decltype(kind_tag)::value;
        if (s_active) {
            char* dst = smem + (s_par * 4 + KIND) * P8_HALF + wave * 16 * ROW_BYTES;
            const int kbyte = s_t * ROW_BYTES;
            if constexpr (KIND == 0 || KIND == 2) {
                const size_t off = (KIND == 2 ? a_half_step : 0) + kbyte;
                if (corpus_nt) {  // ONE query tile: every corpus line is read once, by one workgroup (as in the two-slot kernel)
                    glds16_aux<2>(a_src[0] + off, dst);
                    glds16_aux<2>(a_src[1] + off, dst + 8 * ROW_BYTES);
                } else {
                    glds16(a_src[0] + off, dst);
                    glds16(a_src[1] + off, dst + 8 * ROW_BYTES);
                }
            } else if constexpr (KIND == 1) {
                glds16(b_src[0] + b_half_step + kbyte, dst);
                glds16(b_src[1] + b_half_step + kbyte, dst + 8 * ROW_BYTES);
            } else {
                glds16(b_src[0] + kbyte, dst);
                glds16(b_src[1] + kbyte, dst + 8 * ROW_BYTES);
            }
            ++issued;
            if constexpr (KIND == 3) {  // the stream's K-tile is complete
                s_par ^= 1;
                if (++s_t == nk) {  // ... and moves on to this workgroup's next corpus tile
                    s_t = 0;
                    ++s_it;
                    if (s_it < n_my) {
                        long long step = (long long)tile_step_bytes;
                        if (ex.perm_mod > 0) {
                            int nxt = super_cur + perm_inc;
                            if (nxt >= ex.perm_mod) nxt -= ex.perm_mod;
                            step = (long long)(nxt - super_cur) * (long long)BM * (long long)row_stride;
                            super_cur = nxt;
                        }
                        a_src[0] += step;
                        a_src[1] += step;
                    } else {
                        s_active = false;
                    }
                }
            }
        }
    };
    using K0 = std::integral_constant<int, 0>;
    using K1 = std::integral_constant<int, 1>;
    using K2 = std::integral_constant<int, 2>;
    using K3 = std::integral_constant<int, 3>;

    const int fr = lane & 15, fq = lane >> 4;
    const int swz = (fr >> 1) & 7;

    // thresholds first, and retired: a later compiler-inserted vmcnt wait for them would also drain the LDS-DMAs in flight
    float thr[NB16];
#pragma unroll
    for (int j = 0; j < NB16; ++j) {
        const int q = q0 + wn * TN + j * 16 + fr;
        thr[j] = q < nq ? thr_s[q] : __builtin_inff();
    }
#pragma unroll
    for (int j = 0; j < NB16; ++j) asm volatile("" : "+v"(thr[j]));
    wait_vmcnt<0>();

    // ---- per-wave survivor list (mips_common.h, as in the persistent kernel of kernels_mips.hip).  After a flush or a direct emit:
    // wait_vmcnt<0>(), the counted waits of the K loop must only ever see LDS-DMA pieces (loads and stores retire independently).
    WaveSurvivorList<P8_WL_CAP, SUBSET> wl(smem + P8_OPERANDS, NWAVES, wave);
    const SurvivorOut out{thr_key, cand, cnt, cap, overflow, ex};
    auto wl_append = [&](bool p, key_t64 key, int q) { if (wl.append(p, key, q, out)) wait_vmcnt<0>(); };
    auto wl_flush = [&]() { wl.flush(out); wait_vmcnt<0>(); };
    float* const xpose = (float*)(smem + P8_OPERANDS + NWAVES * P8_WL_CAP * 12) + wave * 64;
    // ---- per-wave survivor ring: the 32 sums of a (hit lane, query block) + one metadata word (corpus tile row | block << 6 | lane) per
    // record, written during the K loop and turned into list entries after the last tile (the drain below).  ring_n: wave-uniform.
    const size_t ring_wave = (size_t)bid * NWAVES + wave;
    float* const ring_w = ring + ring_wave * ring_cap * 32;
    unsigned* const ring_meta = (unsigned*)(ring + (size_t)gridDim.x * NWAVES * ring_cap * 32) + ring_wave * ring_cap;
    int ring_n = 0;
    int ring_fallbacks = 0;  // query blocks with survivors that took the in-loop path (wave-uniform; flag word [3] of `overflow`)

    f32x4 acc[MB][NB16];
    u32x4 fa[4], fb[2], fa1[4], fb1[2];  // the quadrant's fragments: k-step 0 (fa, fb) and k-step 1 (fa1, fb1)
    u32x4 fc[2], fc1[2];                 // KEEPB0: the B1 fragments get registers of their own
    // timing knobs.  Compile-time (-DP8_KNOBS: read from "kflags"): as run-time branches around s_setprio / the stagger barrier they
    // changed the compiler's schedule of the whole loop - the SAME kernel went from -1.2 % to +2.3 % against tile 8 on C3
    // (profiles/r05_ab_8phase.txt).  Measured with the knobs: no stagger +10 %, no s_setprio +2 %.
#ifdef P8_KNOBS
    const bool knob_no_stagger = (ex.flags & (1 << 8)) != 0, knob_no_prio = (ex.flags & (2 << 8)) != 0;
#else
    constexpr bool knob_no_stagger = false, knob_no_prio = false;
#endif

    // fragment reads of one half-tile buffer: A quadrant rows wm*64 + i'*16 + fr, B quadrant rows wn*32 + j'*16 + fr
    auto read_a = [&](const char* half) {
        const char* base = half + (wm * 64 + fr) * ROW_BYTES;
        const int s0 = ((0 + fq) ^ swz) << 4, s1 = ((4 + fq) ^ swz) << 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fa[i] = *(const u32x4*)(base + i * 16 * ROW_BYTES + s0);
            fa1[i] = *(const u32x4*)(base + i * 16 * ROW_BYTES + s1);
        }
    };
    auto read_b = [&](const char* half) {
        const char* base = half + (wn * 32 + fr) * ROW_BYTES;
        const int s0 = ((0 + fq) ^ swz) << 4, s1 = ((4 + fq) ^ swz) << 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            fb[j] = *(const u32x4*)(base + j * 16 * ROW_BYTES + s0);
            fb1[j] = *(const u32x4*)(base + j * 16 * ROW_BYTES + s1);
        }
    };
    auto read_b1 = [&](const char* half) {  // B1 into fc / fc1 (KEEPB0) or over B0 (fb / fb1)
        const char* base = half + (wn * 32 + fr) * ROW_BYTES;
        const int s0 = ((0 + fq) ^ swz) << 4, s1 = ((4 + fq) ^ swz) << 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if constexpr (KEEPB0) {
                fc[j] = *(const u32x4*)(base + j * 16 * ROW_BYTES + s0);
                fc1[j] = *(const u32x4*)(base + j * 16 * ROW_BYTES + s1);
            } else {
                fb[j] = *(const u32x4*)(base + j * 16 * ROW_BYTES + s0);
                fb1[j] = *(const u32x4*)(base + j * 16 * ROW_BYTES + s1);
            }
        }
    };
    auto mma_quadrant = [&](int mh, int nh, bool zero_c) {
        if (!knob_no_prio) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int mhh = 0; mhh < 2; ++mhh)
#pragma unroll
                    for (int nhh = 0; nhh < 2; ++nhh)
                        if (mhh == mh && nhh == nh) {
                            f32x4& c = acc[mhh * 4 + i][nhh * 2 + j];
                            c = mfma16<DT>(fa[i], (KEEPB0 && nhh == 1) ? fc[j] : fb[j], zero_c ? f32x4{0.f, 0.f, 0.f, 0.f} : c);
                        }
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
#pragma unroll
                for (int mhh = 0; mhh < 2; ++mhh)
#pragma unroll
                    for (int nhh = 0; nhh < 2; ++nhh)
                        if (mhh == mh && nhh == nh) {
                            f32x4& c = acc[mhh * 4 + i][nhh * 2 + j];
                            c = mfma16<DT>(fa1[i], (KEEPB0 && nhh == 1) ? fc1[j] : fb1[j], c);
                        }
            }
        if (!knob_no_prio) __builtin_amdgcn_s_setprio(0);
    };

    // ---- epilogue of one tile (the persistent kernel's, FILTER mode) ------------------------------
    // What it costs (round 6: compile-time part removal, experiments/tools/build_p8_parts.sh with -DP8_ABL_NO_EPILOGUE / -DP8_ABL_NO_EMIT;
    // profiles/r06_ab_epilogue.txt): on C3 the block maxima + compares 0.24 ms of a 13.2 ms batch, the SURVIVOR path below 0.85-1.28 ms
    // (11 % of C2, 12 % of a 1.25 M-row shard).  It is not a cold path: a stage lets ~k * growth rows per query pass, 1.4-2.4 per wave
    // tile, so ~45 % of the (wave, 16-query block) pairs take it, and the 8 waves meet at the next barrier - every tile pays its slowest
    // wave.  Hence the planner's small stage growth (vodhip_api.hip); moving the maxima into the K loop's phases and narrowing the hit mask
    // by fragment were built and measured: slower / equal (same profile).
    auto epilogue = [&](int x0) {
#ifdef P8_ABL_NO_EPILOGUE  // timing only (experiments/tools/build_p8_parts.sh): the accumulators stay live, nothing is filtered
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NB16; ++j) asm volatile("" ::"v"(acc[i][j]));
        (void)x0;
        return;
#else
        // the block maxima of this lane, all four query blocks first: four independent v_max3 chains (16 deep each) the scheduler can
        // interleave - behind the branches of the survivor path they would run one after the other.  (v_max3, not fmaxf: hipcc quiets
        // every operand of fmaxf first, two more v_max per value; a quiet NaN operand of v_max3 is ignored, which is what the per-value
        // compares below do with it too.)
        float mj[NB16];
#pragma unroll
        for (int j = 0; j < NB16; ++j) {
            mj[j] = vmax3(acc[0][j][0], acc[0][j][1], acc[0][j][2]);
            mj[j] = fmaxf_raw(mj[j], acc[0][j][3]);
        }
#pragma unroll
        for (int i = 1; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NB16; ++j) {
                mj[j] = vmax3(mj[j], acc[i][j][0], acc[i][j][1]);
                mj[j] = vmax3(mj[j], acc[i][j][2], acc[i][j][3]);
            }
#ifdef P8_ABL_NO_EMIT  // timing only: the tests run, their survivors are dropped
#pragma unroll
        for (int j = 0; j < NB16; ++j) {
            const unsigned long long any_hit = __ballot(mj[j] >= thr[j]);
            asm volatile("" ::"s"(any_hit));
        }
        (void)x0;
        return;
#else
        // ... and the four tests: most tiles of a search's late stages hold no survivor for any of the wave's 64 queries - one branch, not four
        unsigned long long hl[NB16];
#pragma unroll
        for (int j = 0; j < NB16; ++j) hl[j] = __ballot(mj[j] >= thr[j]);  // (false for NaN and for padded queries: thr = +inf)
        if ((hl[0] | hl[1] | hl[2] | hl[3]) == 0ull) {
            if (wl.n >= P8_WL_FLUSH) wl_flush();
            return;
        }
        static_assert(NB16 == 4, "the early-out above");
#pragma unroll
        for (int j = 0; j < NB16; ++j) {
            const float m = mj[j];
            const bool hit = m >= thr[j];  // false for NaN and for padded queries (thr = +inf)
            // The survivor path, two forms (the same records either way, in a different order: the select kernel's result does not
            // depend on it):
            //  * RING (the common case): every hit lane stores its 32 sums (8 x 16 B) and one metadata word to the next free record of the
            //    wave's ring - no compare, no key, no list, no branch per lane; the drain after the last tile does the rest, out of the
            //    barrier-synchronous loop.  In the loop a query block that holds any survivor cost the tile ~1.2 us in its slowest wave
            //    (the other seven wait at the next barrier), ~5 % of a C3 batch (profiles/r07_survivor_ring.txt).  The stores retire in
            //    vmcnt like the LDS-DMA pieces: the counted waits stay safe (loads still retire in order among themselves).
            //  * IN THE LOOP (a block that does not fit into the rest of the ring; the path of the previous rounds, unchanged):
            //    - TRANSPOSE (<= P8_TRANSPOSE_MAX_LANES lanes hold survivors): a lane that holds a survivor writes its 32 sums of this query
            //      to LDS (8 ds_write_b128) and lane t of a 32-lane half reads sum t back: one compare, one key and one append per half
            //      handle all 32 in parallel, with row offsets that depend on the lane number alone.  Two source lanes per pass; the source
            //      lane's threshold and coordinates travel as scalars (v_readlane, s_ff1).
            //    - MASK (more lanes): every lane compares its 32 sums into a hit mask and appends its own survivors, all lanes at once; the
            //      score of a single survivor is the lane's maximum; lanes with several go through the transpose.  Dense overflowing
            //      blocks (large k, tiny rings) need it: transpose-only was +1.4 % at k 1000 on C3, +7.6 % with a 1-record ring on a shard.
            const unsigned long long hit_lanes = hl[j];
            if (hit_lanes != 0ull && ring_n + __builtin_popcountll(hit_lanes) <= ring_cap) {
                if (hit) {
                    const int slot = ring_n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hit_lanes >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hit_lanes, 0u));
                    f32x4* const rec = (f32x4*)(ring_w + (size_t)slot * 32);
#pragma unroll
                    for (int i = 0; i < MB; ++i) rec[i] = acc[i][j];
                    int x0_o = x0, lane_o = lane;  // (opaque: see below)
                    asm volatile("" : "+s"(x0_o));
                    asm volatile("" : "+v"(lane_o));
                    ring_meta[slot] = (unsigned)x0_o | (unsigned)(j << 6) | (unsigned)lane_o;  // (x0: a multiple of 256)
                }
                ring_n += __builtin_popcountll(hit_lanes);
            } else if (hit_lanes != 0ull) {
                ++ring_fallbacks;
                // (opaque: or hipcc computes the lane-dependent offsets of all four query blocks once, outside the K loop, and holds them in
                // vector registers the loop does not have - it spilled 18)
                int x0_o = x0, row_end_o = row_end, lane_o = lane;
                asm volatile("" : "+s"(x0_o), "+s"(row_end_o));
                asm volatile("" : "+v"(lane_o));
                // (`src_lanes`: the lanes whose sums travel; `mine`: this lane is one of them)
                auto transpose_emit = [&](unsigned long long src_lanes, bool mine) __attribute__((always_inline)) {
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(src_lanes >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)src_lanes, 0u));
                    const int half = lane_o >> 5, t = lane_o & 31;
                    unsigned long long rest = src_lanes;
                    int done = 0;  // source lanes handled by earlier passes
                    do {
                        const int slot = rank - done;
                        if (mine && (unsigned)slot < 2u) {
                            float* dst = xpose + slot * 32;
#pragma unroll
                            for (int i = 0; i < MB; ++i) *(f32x4*)(dst + 4 * i) = acc[i][j];
                        }
                        wave_lds_exchange();
                        const int l0 = __builtin_ctzll(rest);
                        rest &= rest - 1ull;
                        const bool two = rest != 0ull;
                        const int l1 = two ? __builtin_ctzll(rest) : l0;
                        rest &= rest - 1ull;  // (0 stays 0)
                        const float t0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, thr[j]), l0));
                        const float t1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, thr[j]), l1));
                        const float sc = xpose[lane_o];
                        const int src = half ? l1 : l0;
                        const float thr_src = half ? t1 : t0;
                        const int q_src = q0 + wn * TN + j * 16 + (src & 15);
                        const int rw = x0_o + wm * TM + 4 * (src >> 4) + (t >> 2) * 16 + (t & 3);
                        wl_append((half == 0 || two) && sc >= thr_src && rw < row_end_o, make_key(sc, (unsigned)rw), q_src);
                        done += 2;
                        wave_lds_exchange();  // (this pass's loads before the next pass's stores)
                    } while (rest != 0ull);
                };
                if (__builtin_popcountll(hit_lanes) <= P8_TRANSPOSE_MAX_LANES) {
                    transpose_emit(hit_lanes, hit);
                } else {
                    // many lanes: every lane compares its 32 sums into a hit mask; a lane with ONE survivor appends it from its maximum, all
                    // such lanes at once; the lanes with several (few) send theirs through the transpose
                    unsigned mask = 0;
                    if (hit) {
#pragma unroll
                        for (int v = 0; v < MB * 4; ++v) mask |= (acc[v >> 2][j][v & 3] >= thr[j]) ? (1u << v) : 0u;
                    }
                    const bool several = (mask & (mask - 1u)) != 0u;
                    const int q = q0 + wn * TN + j * 16 + (lane_o & 15);
                    const int b = hit ? __builtin_ctz(mask) : 0;
                    const int rw = x0_o + wm * TM + 4 * (lane_o >> 4) + (b >> 2) * 16 + (b & 3);
                    wl_append(hit && !several && rw < row_end_o, make_key(m, (unsigned)rw), q);
                    const unsigned long long several_lanes = __ballot(several);
                    if (several_lanes != 0ull) transpose_emit(several_lanes, several);
                }
            }
        }
        if (wl.n >= P8_WL_FLUSH) wl_flush();
#endif  // P8_ABL_NO_EMIT
#endif  // P8_ABL_NO_EPILOGUE
    };

    // ---- prologue: 7 half-tiles in flight, the first K-tile landed and visible -----------------------
    stage(K0{}); stage(K1{}); stage(K2{}); stage(K3{});
    stage(K0{});
    if constexpr (LEAD >= 6) stage(K1{});
    if constexpr (LEAD >= 7) stage(K2{});
    using S0 = std::integral_constant<int, (0 + LEAD) & 3>;  // the kind phase qd stages: (qd + LEAD) & 3
    using S1 = std::integral_constant<int, (1 + LEAD) & 3>;
    using S2 = std::integral_constant<int, (2 + LEAD) & 3>;
    using S3 = std::integral_constant<int, (3 + LEAD) & 3>;
    auto wait_next_ktile = [&](int done_ktiles) {
        // everything but the half-tiles staged beyond K-tile `done_ktiles` (0-based: that one must be complete) may stay in flight
        const int ahead = issued - 4 * (done_ktiles + 1);
        if (ahead >= 3) wait_vmcnt<6>();
        else if (ahead == 2) wait_vmcnt<4>();
        else if (ahead == 1) wait_vmcnt<2>();
        else wait_vmcnt<0>();
    };
    wait_next_ktile(0);
    __builtin_amdgcn_s_barrier();
    if (wm == 1 && !knob_no_stagger) __builtin_amdgcn_s_barrier();  // the second wave row runs one barrier behind

    int kt = 0;  // global K-tile counter of this workgroup: operand buffers (kt & 1) * 4 ..
    for (int it = 0; it < n_my; ++it) {
        const int x0 = ex.perm_mod > 0 ? super_epi * BM : row_begin + (xt0 + it * xt_step) * BM;
        for (int t = 0; t < nk; ++t, ++kt) {
            const char* kb = smem + (kt & 1) * 4 * P8_HALF;  // [A0 | B1 | A1 | B0] of this K-tile
            const bool first = t == 0;
            // qd 0: (m0, n0)
            read_a(kb + 0 * P8_HALF);
            read_b(kb + 3 * P8_HALF);
            stage(S0{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (first) mma_quadrant(0, 0, true); else mma_quadrant(0, 0, false);
            __builtin_amdgcn_s_barrier();
            // qd 1: (m0, n1)
            read_b1(kb + 1 * P8_HALF);
            stage(S1{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (first) mma_quadrant(0, 1, true); else mma_quadrant(0, 1, false);
            __builtin_amdgcn_s_barrier();
            // qd 2: (m1, n1)
            read_a(kb + 2 * P8_HALF);
            stage(S2{});
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (first) mma_quadrant(1, 1, true); else mma_quadrant(1, 1, false);
            __builtin_amdgcn_s_barrier();
            // qd 3: (m1, n0); the next K-tile's half-tiles must have landed before this phase's first barrier
            if constexpr (!KEEPB0) read_b(kb + 3 * P8_HALF);
            stage(S3{});
            wait_next_ktile(kt + 1);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (first) mma_quadrant(1, 0, true); else mma_quadrant(1, 0, false);
            __builtin_amdgcn_s_barrier();
        }
        epilogue(x0);
        // the super-tile of the next corpus tile: the issue stream reached it (at the latest) two K-tiles ago, track it separately
        if (ex.perm_mod > 0) {
            int nxt = super_epi + perm_inc;
            if (nxt >= ex.perm_mod) nxt -= ex.perm_mod;
            super_epi = nxt;
        }
    }
    if (wm == 0 && !knob_no_stagger) __builtin_amdgcn_s_barrier();  // balances the stagger

    // ---- the drain: the ring's records -> the wave's list, as the transpose path does it (lane t of half h takes sum t of record
    // 2 p + h).  The operand buffers are idle now (every wave is past its last fragment read: the barrier above): the wave copies
    // P8_DRAIN_RECORDS records at a time into its 16 KB of them with LDS-DMA (one round trip per copy, device-scope `sc1` loads that miss
    // the CU's L1, whatever it holds of these lines) and reads them from there.
#ifndef P8_ABL_NO_DRAIN  // (timing only: the records are dropped)
    if (ring_n > 0) {
        wait_vmcnt<0>();  // the records have landed
        if (fq == 0) {
#pragma unroll
            for (int j = 0; j < NB16; ++j) xpose[j * 16 + fr] = thr[j];  // the thresholds by (block, query), for any lane to read
        }
        wave_lds_exchange();
        char* const stage_w = smem + wave * (P8_OPERANDS / NWAVES);
        const float* const sums = (const float*)stage_w;
        const unsigned* const meta = (const unsigned*)(stage_w + P8_DRAIN_RECORDS * 128);
        const int half = lane >> 5, t = lane & 31;
        for (int r0 = 0; r0 < ring_n; r0 += P8_DRAIN_RECORDS) {
            // (sources clamped to the wave's last record: every address stays inside its ring)
#pragma unroll
            for (int i = 0; i < P8_DRAIN_RECORDS / 8; ++i) {  // 8 records of 128 B per instruction
                const int r = min(r0 + i * 8 + (lane >> 3), ring_n - 1);
                __builtin_amdgcn_global_load_lds((const VOD_AS1 void*)(ring_w + (size_t)r * 32 + (lane & 7) * 4),
                                                 (VOD_AS3 void*)(stage_w + i * 1024), 16, 0, P8_SC1);
            }
#pragma unroll
            for (int i = 0; i < (P8_DRAIN_RECORDS + 63) / 64; ++i) {
                const int r = min(r0 + i * 64 + lane, ring_n - 1);
                __builtin_amdgcn_global_load_lds((const VOD_AS1 void*)(ring_meta + r), (VOD_AS3 void*)(stage_w + P8_DRAIN_RECORDS * 128 + i * 256),
                                                 4, 0, P8_SC1);
            }
            wait_vmcnt<0>();
            const int nr = min(ring_n - r0, P8_DRAIN_RECORDS);
            // two passes per step and one flush check: a pass appends <= 64 entries, so <= 128 before the step keeps the list in bounds
            for (int r4 = 0; r4 < nr; r4 += 4) {
                if (wl.n > P8_WL_CAP - 128) wl_flush();
                const int r = r4 + half;
#pragma unroll
                for (int u = 0; u < 4; u += 2) {
                    const float v = sums[(r + u) * 32 + t];  // (r + u < P8_DRAIN_RECORDS + 3: inside the wave's 16 KB; past nr read, not used)
                    const unsigned m = meta[r + u];
                    const int src = (int)(m & 63u), jb = (int)((m >> 6) & 3u), x0 = (int)(m & ~255u);
                    const int q_src = q0 + wn * TN + jb * 16 + (src & 15);
                    const int rw = x0 + wm * TM + 4 * (src >> 4) + (t >> 2) * 16 + (t & 3);
                    wl_append(r + u < nr && v >= xpose[jb * 16 + (src & 15)] && rw < row_end, make_key(v, (unsigned)rw), q_src);
                }
            }
        }
    }
#endif
    wl_flush();
    if (ring_fallbacks > 0 && lane == 0) atomicAdd(overflow + 3, (unsigned)ring_fallbacks);
}

template <bool KEEPB0, int LEAD = 7>
static hipError_t launch_8phase(int store_dtype, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin, int64_t row_end, int n_xtiles,
                                   int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream) {
    const bool subset = ws.extra.row_label != nullptr;
    const int n_qtiles = (int)(nq_pad / 256);
    const int n_cu = ws.n_cu > 0 ? ws.n_cu : 256;
    const int unit = 8 * n_qtiles;
    const int total = ((n_xtiles + 7) / 8) * unit;
    int grid = (n_cu / unit) * unit;
    if (grid < unit) grid = unit;
    if (grid > total) grid = total;
    // the survivor rings: ws.ring_cap records per wave, fewer if the allocation is short of this grid's waves (none: in-loop path only)
    const int ring_cap = ws.ring ? (int)std::min<int64_t>(ws.ring_cap, ws.ring_floats / ((int64_t)grid * 8 * 33)) : 0;
    auto launch = [&](auto kern) -> hipError_t {
        if (hipError_t e = allow_dynamic_lds((const void*)kern, P8_LDS); e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), P8_LDS, stream, (const uint16_t*)store, (const uint16_t*)q_pad, (int)dim_pad,
                           (int)row_begin, (int)row_end, n_xtiles, n_qtiles, (int)nq, ws.thr_s, ws.thr_key, ws.cand, ws.cnt, (int)ws.cap,
                           ws.overflow, ws.extra, ws.ring, ring_cap);
        return hipGetLastError();
    };
    if constexpr (LEAD != 7)  // (experiment builds: no subset instantiation)
        return store_dtype == 0 ? launch(mips_filter8ph_kernel<0, false, KEEPB0, LEAD>) : launch(mips_filter8ph_kernel<1, false, KEEPB0, LEAD>);
    else if (subset) return store_dtype == 0 ? launch(mips_filter8ph_kernel<0, true, KEEPB0>) : launch(mips_filter8ph_kernel<1, true, KEEPB0>);
    else return store_dtype == 0 ? launch(mips_filter8ph_kernel<0, false, KEEPB0>) : launch(mips_filter8ph_kernel<1, false, KEEPB0>);
}

hipError_t launch_filter_8phase(int store_dtype, int lead, bool keep_b0, const void* store, const void* q_pad, int64_t dim_pad, int64_t row_begin,
                                int64_t row_end, int64_t nq, int64_t nq_pad, const SearchWorkspace& ws, hipStream_t stream) {
    constexpr FilterGeometry G = geometry(FilterKernel::EightPhase);
    static_assert(G.rows == 256 && G.cols == 256 && G.persistent, "the planner's geometry of mips_filter8ph_kernel");
    int n_xtiles = (int)((row_end - row_begin + 255) / 256);
    if (ws.extra.perm_mod > 0) row_end = ws.extra.row_bound;  // permuted stage order: whole positions, rows masked at ntotal
#ifdef VODHIP_EXPERIMENTS
    if (lead == 6) return launch_8phase<true, 6>(store_dtype, store, q_pad, dim_pad, row_begin, row_end, n_xtiles, nq, nq_pad, ws, stream);
    if (lead == 5) return launch_8phase<true, 5>(store_dtype, store, q_pad, dim_pad, row_begin, row_end, n_xtiles, nq, nq_pad, ws, stream);
    if (!keep_b0) return launch_8phase<false>(store_dtype, store, q_pad, dim_pad, row_begin, row_end, n_xtiles, nq, nq_pad, ws, stream);
#endif
    (void)lead;
    (void)keep_b0;
    return launch_8phase<true>(store_dtype, store, q_pad, dim_pad, row_begin, row_end, n_xtiles, nq, nq_pad, ws, stream);
}

}  // namespace vodhip
