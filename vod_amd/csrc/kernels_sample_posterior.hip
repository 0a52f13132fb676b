// k rows drawn WITHOUT replacement from the retriever's posterior over the WHOLE store, with their priority-sampling weights
// (vodhip_index_sample_posterior, include/vodhip.h H2s): Gumbel-top-k = priority sampling with the keys
//   key(q, z) = beta * s(q, z) - log E(seed, qs, g),   E ~ Exp(1) from a counter-based generator,
// s the float32 score of the log-partition scan, g = id_base + row the global row id, qs = query_offset + q the query's stream index.
// The result is the k eligible rows with the largest keys by (key desc, id asc); log_tau = the (k+1)-th largest key - log Z.
// The call first runs the three launches of kernels_partition.hip unchanged (stage, scan, finish): (max_score, log_rel) are that call's
// bits.  Then four launches of this file:
//   key-max   the shared scan core (store_scan.h: the K loop, hence the score bits, and the eligibility rule of every whole-store scan)
//             over a 256-row tile x 64 | 128 queries; the epilogue writes the tile's MAXIMUM finite key per query, keymax[q][tile]
//             (-inf: none).  A maximum has no order: no atomics.
//   threshold one workgroup per query: theta[q] = the (k+1)-th largest of the query's tile maxima by a radix select over the
//             order-preserving image of the float (4 passes of 8 bits; the histogram counts do not depend on the order of the LDS
//             atomics); fewer than k + 1 tiles with a finite maximum: -inf.  k + 1 DISTINCT rows have keys >= theta, so theta is a lower
//             bound of the true (k+1)-th key: nothing is ever missed and there is no recovery pass.
//   emit      the SAME kernel (one binary per dtype / width / subset, a launch argument picks the epilogue's tail: the key of a row
//             is computed by the same instructions in both launches, so a tile's own maximum can never fall below theta).
//             A workgroup none of whose queries has keymax[q][tile] >= theta[q] returns BEFORE its K loop; of the others, a lane
//             looks only at its columns that are hit.  Every eligible row with a finite key >= theta[q] is appended to the query's
//             candidate list as (key | row, score) behind one returning vector atomicAdd; the list is unordered.  At most 256 t
//             candidates, t = tiles with keymax >= theta = k + 1 unless tile maxima tie exactly at theta; the list stride is
//             256 (k + 1 + SP_SLACK_TILES) (at most the padded store): a slot past it is not written, the query is counted in the
//             status words and the call fails.
//   select    one workgroup per query: the k + 1 largest candidates by (key desc, row asc) with wg_sort_regs over chunks of 1792
//             behind the running best 256; a second pass over the list finds each winner's score by binary search of its key; ids,
//             scores, keys (unnormalised, stored - never recomputed), and in double from the float32 inputs
//             log_p = beta (s - max_score) - log_rel, log_tau = (key_{k+1} - beta max_score) - log_rel,
//             log_weight = log_p - log(-expm1(-exp(log_p - log_tau)))  (log_tau = -inf: log_weight = log_p).
// NOISE.  Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (low word of g >> 2, g >> 34, qs, j): output word g & 3 of the
// call with j = 0 is the HIGH word w_hi of row g, with j = 1 its LOW word w_lo.  v = float32((w_hi 2^32 + w_lo + 1/2) 2^-64) (through
// double: the sum is exact below 2^52 and rounds once above, then once to float32), clamped to 1 - 2^-24; E = -log1pf(-v);
// key = fl(fl(beta * s) - logf(E)) with the library logf / log1pf and contraction off (sample_key).  The four rows (r & 3) of an
// accumulator register group are consecutive and start at a multiple of 4, so with id_base % 4 == 0 one generator call serves four
// registers; otherwise a second call serves the rows behind the counter boundary.
// THE HIGH-WORD SHORT-CUT.  The epilogue first bounds every row's key from above with w_hi alone (key_upper: one generator call per
// four rows, a native log2), then computes exact keys only for rows whose bound can still matter - in the key-max launch in decreasing
// order of the bound until no bound exceeds the best exact key (typically one row per lane and column), in the emit launch for bounds
// >= theta.  A key that is USED - a tile maximum, a candidate - is always the bits of sample_key; a row that is skipped has a key
// strictly below what it would be compared with.
// A query whose log Z is not finite (no eligible row, a +inf score) is all pads; a -inf score has a -inf key and is never drawn.
#include "store_scan.h"
#include "wg_sort.h"

#include "../../include/vodhip.h"

#include <algorithm>

namespace vodhip {

namespace {

constexpr int SP_SLACK_TILES = VODHIP_SAMPLE_SLACK_TILES;
constexpr int SP_SORT = 2048, SP_KEEP = 256;  // select: keys per sort, of which the running best

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// THE key: one function, explicit roundings, no contraction.
__device__ __forceinline__ float sample_key(float beta, float s, unsigned w_hi, unsigned w_lo) {
#pragma clang fp contract(off)
    const double vd = ((double)(((unsigned long long)w_hi << 32) | (unsigned long long)w_lo) + 0.5) * 0x1p-64;
    const float v = fminf((float)vd, 0x1.fffffep-1f);
    const float e = -log1pf(-v);
    return __fsub_rn(__fmul_rn(beta, s), logf(e));
}

// An upper bound of sample_key(beta, s, w_hi, any w_lo) from the high word alone, with native arithmetic.  With hm = w_hi without its
// low 8 bits (exact as a float32) and vl = hm 2^-32: vl <= v_dev (rounding is monotone, the clamp is not below any vl), so
//   E_dev = -log1pf(-v_dev) >= -log(1 - vl) (1 - 2^-22) >= vl (1 + vl / 2) (1 - 2^-22),   log(1 + x) >= x - x^2 / 2,
//   -logf(E_dev) <= -log(vl) - (x - x^2 / 2) + 2^-21 + 45 * 2^-23,   x = vl / 2   (|log E| <= 45; logf is 1 ulp).
// The native log2 is within 2^-22 relative of a value of at most 32, the roundings of this function and of the key's own subtraction
// are within 2^-23 of |beta s| + 32 each: the slack 2e-4 + (|beta s| + 32) 2^-21 covers all of it several times.  hm == 0: +inf.
__device__ __forceinline__ float key_upper(float beta, float s, unsigned w_hi) {
    const unsigned hm = w_hi & 0xFFFFFF00u;
    if (hm == 0u) return __builtin_inff();
    const float t1 = __fmul_rn(beta, s);
    const float vl = (float)hm * 0x1p-32f;
    const float x = 0.5f * vl;
    const float nl = -0.69314718f * __log2f(vl) - (x - 0.5f * x * x);
    return t1 + nl + ((fabsf(t1) + 32.f) * 0x1p-21f + 2e-4f);
}

struct SampleScan {
    float* keymax;              // [n_qtiles * BN][n_xtiles]
    const float* theta;         // [..] emit: the query's threshold
    key_t64* cand_key;          // [..][stride] emit: flip(key) << 32 | ~row
    float* cand_score;          // [..][stride]
    unsigned int* cnt;          // [.. * CNT_STRIDE]
    unsigned int* status;       // SPS_* words
    int stride;
    int emit;                   // 0: key-max launch, 1: emit launch
    unsigned seed_lo, seed_hi;
    unsigned qs0;               // stream index of query 0 of this launch
    unsigned long long id_base;
};
enum : int { SPS_OVERFLOW = 0, SPS_SELF = 1, SPS_MAX_CAND = 2, SPS_SKIPPED = 3, SPS_TOTAL_LO = 4, SPS_TOTAL_HI = 5, SPS_WORDS = 8 };

// X: the store [>= n_xtiles * 256 rows][dim_pad]; Q: the staged queries [n_qtiles * BN][dim_pad]
template <int DT, int BN, int WN, bool SUBSET>
__global__ __launch_bounds__(scan_threads(WN), 1)
void sample_scan_kernel(const uint16_t* __restrict__ X, const uint16_t* __restrict__ Q, int dim_pad, int ntotal, int n_xtiles, int n_qtiles,
                        int nq, float beta, SampleScan sp, FilterExtra ex) {
    constexpr int WM = SCAN_WM;
    constexpr int TM = SCAN_BM / WM, TN = BN / WN;
    constexpr int MI = TM / 32, NJ = TN / 32;
    static_assert(WM * BN * (int)sizeof(float) <= scan_ring_bytes(BN) / SCAN_NSTAGE, "the reduction array reuses the first ring slot");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    int qt, xt;
    if (!scan_block_tile(blockIdx.x, n_qtiles, n_xtiles, &qt, &xt)) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int fr = lane & 31, fh = lane >> 5;
    const int x0 = xt * SCAN_BM;
    const int q0 = qt * BN;
    const float inf = __builtin_inff();

    if (sp.emit) {  // a tile that holds no query's candidates: out before the K loop (uniform over the workgroup)
        bool hit = false;
        if (tid < BN && q0 + tid < nq) {
            const float km = sp.keymax[(size_t)(q0 + tid) * n_xtiles + xt];
            hit = km > -inf && km >= sp.theta[q0 + tid];
        }
        if (!__syncthreads_or(hit)) {
            if (tid == 0) atomicAdd(&sp.status[SPS_SKIPPED], 1u);
            return;
        }
    }

    f32x16 acc[MI][NJ];
    scan_k_loop<DT, BN, WN>(X + (size_t)x0 * dim_pad, Q + (size_t)q0 * dim_pad, dim_pad, smem, acc);

    // ---- epilogue
    __syncthreads();  // every wave has read its last fragments: the first ring slot becomes the reduction array
    float* red_m = reinterpret_cast<float*>(smem);  // [WM][BN]
    const int rlane = x0 + wm * TM + 4 * fh;        // the lane's row of (block 0, register 0): a multiple of 4
    const int sh = (int)(sp.id_base & 3ull);        // (uniform over the launch)
    static_assert(NJ == 2, "the two query columns of a lane are spelled out below");
    // (a generic lambda per column, not a loop over j: the compiler does not unroll a loop whose body holds the rolled loops below, and
    // a rolled j indexes the accumulator dynamically - through scratch)
    auto column = [&](auto j_tag) {
        constexpr int j = decltype(j_tag)::value;
        const int col = wn * TN + j * 32 + fr;
        const int q = q0 + col;
        bool act = q < nq;
        float th = -inf;
        if (sp.emit && act) {
            const float km = sp.keymax[(size_t)q * n_xtiles + xt];
            th = sp.theta[q];
            act = km > -inf && km >= th;
        }
        const unsigned mask = act ? scan_eligible_mask<SUBSET>(acc[0][j], acc[1][j], rlane, ntotal, q, ex) : 0u;
        // Pass 1, every eligible row: an UPPER bound of its key from the high word alone (key_upper) - one generator call per four rows
        // and no library logarithm.  -inf: not eligible.
        float ub[MI * 16];
        const unsigned qs = sp.qs0 + (unsigned)q;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const unsigned bits = (mask >> (i * 16 + 4 * a)) & 15u;
#pragma unroll
                for (int e = 0; e < 4; ++e) ub[i * 16 + 4 * a + e] = -inf;
                if (bits) {
                    const unsigned long long g0 = sp.id_base + (unsigned long long)(rlane + i * 32 + 8 * a);
                    const unsigned long long c0 = g0 >> 2;
                    const uint4 h0 = philox4x32_10(make_uint4((unsigned)c0, (unsigned)(c0 >> 32), qs, 0u), sp.seed_lo, sp.seed_hi);
                    uint4 h1 = h0;
                    if (sh) {  // the group straddles a counter boundary
                        const unsigned long long c1 = c0 + 1;
                        h1 = philox4x32_10(make_uint4((unsigned)c1, (unsigned)(c1 >> 32), qs, 0u), sp.seed_lo, sp.seed_hi);
                    }
                    const unsigned wh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned w_hi = sh == 0 ? wh[e] : (sh == 1 ? wh[e + 1] : (sh == 2 ? wh[e + 2] : wh[e + 3]));
                        const float up = key_upper(beta, acc[i][j][4 * a + e], w_hi);
                        ub[i * 16 + 4 * a + e] = ((bits >> e) & 1u) ? up : -inf;
                    }
                }
            }
        // Pass 2: the exact key (sample_key: both words, the library logarithms) of the row with the largest bound among those
        // that can still matter - key-max launch: a bound above the best exact key so far (a row whose bound is not above it cannot be
        // the maximum); emit launch: a bound >= theta.  One row per lane and round, the same instructions in both launches; the wave
        // leaves when no lane has a row left.  Typically one round in the key-max launch, none in most columns of the emit launch.
        float best = -inf;
        while (true) {
            float um = -inf, ssel = 0.f;
            int rsel = 0;
#pragma unroll
            for (int r = 0; r < MI * 16; ++r) {
                const bool c = ub[r] > um;
                um = c ? ub[r] : um;
                ssel = c ? acc[r >> 4][j][r & 15] : ssel;
                rsel = c ? r : rsel;
            }
            const bool go = um > -inf && (sp.emit ? um >= th : um > best);
            if (!__any(go)) break;
            if (go) {
#pragma unroll
                for (int r = 0; r < MI * 16; ++r) ub[r] = r == rsel ? -inf : ub[r];
                const int row = scan_lane_row(rlane, rsel);
                const unsigned long long g = sp.id_base + (unsigned long long)row;
                const unsigned long long c = g >> 2;
                const uint4 h = philox4x32_10(make_uint4((unsigned)c, (unsigned)(c >> 32), qs, 0u), sp.seed_lo, sp.seed_hi);
                const uint4 l = philox4x32_10(make_uint4((unsigned)c, (unsigned)(c >> 32), qs, 1u), sp.seed_lo, sp.seed_hi);
                const int w = (int)(g & 3ull);
                const unsigned w_hi = w == 0 ? h.x : (w == 1 ? h.y : (w == 2 ? h.z : h.w));
                const unsigned w_lo = w == 0 ? l.x : (w == 1 ? l.y : (w == 2 ? l.z : l.w));
                const float key = sample_key(beta, ssel, w_hi, w_lo);
                if (key > -inf && key < inf) {
                    if (!sp.emit) {
                        best = fmaxf(best, key);
                    } else if (key >= th) {
                        const unsigned slot = atomicAdd(&sp.cnt[(size_t)q * CNT_STRIDE], 1u);
                        if (slot < (unsigned)sp.stride) {  // (past the stride: not written; the select kernel reports the query)
                            sp.cand_key[(size_t)q * sp.stride + slot] = make_key(key, (unsigned)row);
                            sp.cand_score[(size_t)q * sp.stride + slot] = ssel;
                        }
                    }
                }
            }
        }
        if (!sp.emit) {
            best = fmaxf(best, __shfl_xor(best, 32, 64));
            if (fh == 0) red_m[wm * BN + col] = best;
        }
    };
    column(std::integral_constant<int, 0>{});
    column(std::integral_constant<int, 1>{});
    if (!sp.emit) {  // (uniform over the launch)
        __syncthreads();
        if (wm == 0 && fh == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int col = wn * TN + j * 32 + fr;
                float m = red_m[col];
#pragma unroll
                for (int w = 1; w < WM; ++w) m = fmaxf(m, red_m[w * BN + col]);
                sp.keymax[(size_t)(q0 + col) * n_xtiles + xt] = m;
            }
        }
    }
}

// One workgroup per query: theta = the (k+1)-th largest of keymax[q][0 .. n_tiles) (finite or -inf each), -inf when fewer than k + 1
// are finite; n_hit = the tiles with a finite maximum >= theta.
constexpr int TH_T = 256;
__global__ void __launch_bounds__(TH_T) sample_threshold_kernel(const float* __restrict__ keymax, int n_tiles, int k, float* __restrict__ theta,
                                                                unsigned int* __restrict__ n_hit) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sel_prefix, sel_want;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float* p = keymax + q * (int64_t)n_tiles;
    unsigned prefix = 0u, pmask = 0u, want = (unsigned)k + 1u;  // the want-th largest among the values that match the prefix
    float th = -__builtin_inff();
    if (n_tiles >= k + 1) {  // (uniform)
        for (int pass = 3; pass >= 0; --pass) {
            const int shift = 8 * pass;
            hist[tid] = 0u;
            __syncthreads();
            for (int t = tid; t < n_tiles; t += TH_T) {
                const unsigned u = flip_f32(p[t]);
                if ((u & pmask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0u;
                int b = 255;
                for (; b > 0; --b) {
                    if (cum + hist[b] >= want) break;
                    cum += hist[b];
                }
                sel_prefix = prefix | ((unsigned)b << shift);
                sel_want = want - cum;
            }
            __syncthreads();
            prefix = sel_prefix;
            want = sel_want;
            pmask |= 255u << shift;
            __syncthreads();
        }
        th = unflip_f32(prefix);  // (the image of -inf is the smallest that occurs: fewer than k + 1 finite maxima select it)
    }
    unsigned c = 0u;
    for (int t = tid; t < n_tiles; t += TH_T) {
        const float v = p[t];
        c += (v > -__builtin_inff() && v >= th) ? 1u : 0u;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
    __syncthreads();
    if ((tid & 63) == 0) hist[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        theta[q] = th;
        n_hit[q] = hist[0] + hist[1] + hist[2] + hist[3];
    }
}

struct SampleSelect {
    const key_t64* cand_key;
    const float* cand_score;
    const unsigned int* cnt;
    const unsigned int* n_hit;
    unsigned int* status;
    int stride, k;
    float beta;
    long long id_base;
    const float* out_max;       // (already offset to the launch's first query, as every output below)
    const float* out_log_rel;
    int64_t* out_ids;
    float* out_scores;
    float* out_log_p;
    float* out_log_weight;
    float* out_keys;
};

// One workgroup per query.
__global__ void __launch_bounds__(256) sample_select_kernel(SampleSelect a) {
    __shared__ key_t64 buf[SP_SORT];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int k = a.k;
    const float inf = __builtin_inff();
    const unsigned have = a.cnt[(size_t)q * CNT_STRIDE];
    const float m = a.out_max[q], lr = a.out_log_rel[q];
    const bool finite = m > -inf && m < inf && lr > -inf && lr < inf;
    const int n = finite ? (int)min(have, (unsigned)a.stride) : 0;
    if (tid == 0) {
        if (have > (unsigned)a.stride) atomicAdd(&a.status[SPS_OVERFLOW], 1u);
        if (have < a.n_hit[q]) atomicAdd(&a.status[SPS_SELF], 1u);  // every hit tile holds at least its own maximum
        atomicMax(&a.status[SPS_MAX_CAND], have);
        atomicAdd((unsigned long long*)&a.status[SPS_TOTAL_LO], (unsigned long long)have);
    }
    const key_t64* ck = a.cand_key + (size_t)q * a.stride;
    const float* cs = a.cand_score + (size_t)q * a.stride;
    for (int i = tid; i < SP_KEEP; i += 256) buf[i] = 0ull;
    for (int base = 0; base == 0 || base < n; base += SP_SORT - SP_KEEP) {
        for (int i = tid; i < SP_SORT - SP_KEEP; i += 256) buf[SP_KEEP + i] = base + i < n ? ck[base + i] : 0ull;
        __syncthreads();
        wg_sort_regs<256, SP_SORT / 256, true, key_t64>(buf, tid);  // descending: the best SP_KEEP stay in front
    }
    // buf[0 .. k]: the k + 1 best keys (0: none)
    const key_t64 ktau = buf[k];
    const double ltau = ktau ? ((double)unflip_f32((unsigned)(ktau >> 32)) - (double)a.beta * (double)m) - (double)lr : -(double)inf;
    for (int p = tid; p <= k; p += 256) {
        const key_t64 c = buf[p];
        a.out_keys[q * (k + 1) + p] = c ? unflip_f32((unsigned)(c >> 32)) : -inf;
        if (p < k && !c) {
            a.out_ids[q * k + p] = -1;
            a.out_scores[q * k + p] = -inf;
            a.out_log_p[q * k + p] = -inf;
            a.out_log_weight[q * k + p] = -inf;
        }
    }
    const key_t64 kth = buf[k - 1];
    for (int i = tid; i < n; i += 256) {
        const key_t64 c = ck[i];
        if (c < kth || !c) continue;
        int lo = 0, hi = k - 1;  // buf[0 .. k) is strictly descending where non-zero and holds c
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (buf[mid] > c) lo = mid + 1;
            else hi = mid;
        }
        const float s = cs[i];
        const double lp = (double)a.beta * ((double)s - (double)m) - (double)lr;
        const double lw = lp - log(-expm1(-exp(lp - ltau)));
        a.out_ids[q * k + lo] = a.id_base + (long long)(0xFFFFFFFFu - (unsigned)c);
        a.out_scores[q * k + lo] = s;
        a.out_log_p[q * k + lo] = (float)lp;
        a.out_log_weight[q * k + lo] = (float)lw;
    }
}

hipError_t launch_sp_scan(const PosteriorSampleArgs& a, const SampleScan& sp, int64_t nq, int64_t nq_pad, int n_tiles, const FilterExtra& ex, hipStream_t stream) {
    return scan_dispatch(a.p.store_dtype, nq_pad, ex.row_label != nullptr, [&](auto dt, auto bn, auto wn, auto subset) {
        const int n_qtiles = (int)(nq_pad / bn.value);
        return scan_launch<bn.value, wn.value>(sample_scan_kernel<dt.value, bn.value, wn.value, subset.value>, scan_grid(n_tiles, n_qtiles), stream,
                                               (const uint16_t*)a.p.store, (const uint16_t*)a.p.q_stage, (int)a.p.dim_pad, (int)a.p.ntotal, n_tiles, n_qtiles,
                                               (int)nq, a.p.beta, sp, ex);
    });
}

}  // namespace

int64_t sample_posterior_stride(int64_t ntotal, int k) {
    const int64_t tiles = scan_tiles(ntotal);
    return SCAN_BM * std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)k + 1 + SP_SLACK_TILES));
}
int64_t sample_posterior_ctl_words(int64_t nq_pad) { return nq_pad * CNT_STRIDE + 2 * nq_pad; }

hipError_t launch_sample_posterior(const PosteriorSampleArgs& a, int64_t q_first, int64_t nq, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (a.k < 1 || a.k > 255 || a.stride < SCAN_BM || a.stride > (1ll << 30)) return hipErrorInvalidValue;
    if (hipError_t e = launch_log_partition(a.p, q_first, nq, stream); e != hipSuccess) return e;  // (checks the shapes)
    if (a.ev && hipEventRecord(a.ev[1], stream) != hipSuccess) return hipErrorUnknown;
    const int64_t nq_pad = scan_nq_pad(nq);
    const int n_tiles = (int)scan_tiles(a.p.ntotal);
    unsigned int* cnt = a.ctl;                                   // [nq_pad * CNT_STRIDE]
    unsigned int* n_hit = a.ctl + nq_pad * CNT_STRIDE;           // [nq_pad]
    float* theta = (float*)(a.ctl + nq_pad * CNT_STRIDE + nq_pad);  // [nq_pad]
    if (hipError_t e = hipMemsetAsync(a.ctl, 0, (size_t)sample_posterior_ctl_words(nq_pad) * 4, stream); e != hipSuccess) return e;
    SampleScan sp;
    sp.keymax = a.keymax;
    sp.theta = theta;
    sp.cand_key = (key_t64*)a.cand_key;
    sp.cand_score = a.cand_score;
    sp.cnt = cnt;
    sp.status = a.status;
    sp.stride = (int)a.stride;
    sp.emit = 0;
    sp.seed_lo = (unsigned)(a.seed & 0xffffffffull);
    sp.seed_hi = (unsigned)(a.seed >> 32);
    sp.qs0 = (unsigned)((unsigned long long)a.query_offset + (unsigned long long)q_first);
    sp.id_base = (unsigned long long)a.id_base;
    if (n_tiles > 0) {
        const FilterExtra ex = scan_filter_extra(a.p, q_first);
        if (hipError_t e = launch_sp_scan(a, sp, nq, nq_pad, n_tiles, ex, stream); e != hipSuccess) return e;
        if (a.ev && hipEventRecord(a.ev[2], stream) != hipSuccess) return hipErrorUnknown;
        hipLaunchKernelGGL(sample_threshold_kernel, dim3((unsigned)nq), dim3(TH_T), 0, stream, (const float*)a.keymax, n_tiles, a.k, theta, n_hit);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (a.ev && hipEventRecord(a.ev[3], stream) != hipSuccess) return hipErrorUnknown;
        sp.emit = 1;
        if (hipError_t e = launch_sp_scan(a, sp, nq, nq_pad, n_tiles, ex, stream); e != hipSuccess) return e;
        if (a.ev && hipEventRecord(a.ev[4], stream) != hipSuccess) return hipErrorUnknown;
    } else if (a.ev) {
        for (int i = 2; i <= 4; ++i)
            if (hipEventRecord(a.ev[i], stream) != hipSuccess) return hipErrorUnknown;
    }
    SampleSelect s;
    s.cand_key = (const key_t64*)a.cand_key;
    s.cand_score = a.cand_score;
    s.cnt = cnt;
    s.n_hit = n_hit;
    s.status = a.status;
    s.stride = (int)a.stride;
    s.k = a.k;
    s.beta = a.p.beta;
    s.id_base = (long long)a.id_base;
    s.out_max = a.p.out_max + q_first;
    s.out_log_rel = a.p.out_log_rel + q_first;
    s.out_ids = a.out_ids + (size_t)q_first * a.k;
    s.out_scores = a.out_scores + (size_t)q_first * a.k;
    s.out_log_p = a.out_log_p + (size_t)q_first * a.k;
    s.out_log_weight = a.out_log_weight + (size_t)q_first * a.k;
    s.out_keys = a.out_keys + (size_t)q_first * (a.k + 1);
    hipLaunchKernelGGL(sample_select_kernel, dim3((unsigned)nq), dim3(256), 0, stream, s);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (a.ev && hipEventRecord(a.ev[5], stream) != hipSuccess) return hipErrorUnknown;
    return hipSuccess;
}

}  // namespace vodhip
