// Retrieval metrics of the training / validation monitor on gfx950: one 256-thread workgroup per row ranks the row ONCE and
// evaluates every requested (metric, topk) from the ranked list; a second launch folds the per-row values into the running
// (total, count) state of every metric in a fixed order.  Two launches per update, no host synchronisation.
//
// Replaces (paths relative to the reference's src/vod_models/monitoring):
//   prepare_for_metric_computation / _mask_rank_inputs   functional.py:15-25,164-178   (argsort + two gathers)
//   _compute_mrr / hitrate / precision / recall           functional.py:41-80
//   _compute_kldiv / min / max / entropy / ndcg           functional.py:83-161
//   RetrievalMonitor.update                               monitor.py:83-105
//   MeanAggregator.update                                 aggregator.py:43-50          (a boolean-index host sync per metric)
//
// Reference semantics kept, quirks included:
//   * n_positives counts `relevance > 0` BEFORE the masking (:172); a NaN or +inf score becomes -inf with relevance 0 (:18-20);
//     -inf is padding: ranked last, NOT masked (a -inf entry keeps its relevance).
//   * ndcg takes the ideal order over the CUT list itself (:158), not over the whole row.
//   * kldiv recounts the positives on the cut list (:91) and is NaN without one.
//   * entropy (:131-139) sums `-(exp(score) * log_softmax(score))`: exp of the raw SCORE, not of the log-probability, so it is
//     the entropy of the distribution only for scores that already are normalised log-probabilities.  Kept as it is.
//   * precision divides by the number of FINITE scores in the cut, recall by n_positives: 0 / 0 is NaN, and NaN rows do not
//     enter the aggregate (aggregator.py:46).
// Deliberate, documented choices:
//   * the reference ranks with an unstable argsort; ties go to the smaller column here (-0.0 ranks as +0.0), which is the order
//     of a stable sort;
//   * mrr / hitrate / precision / recall / min / max are one correctly rounded float32 operation or a selection: bit-exact;
//   * ndcg / kldiv / entropy are evaluated in float64 (tree sums) and rounded to float32 once: the reference's own float32
//     evaluation differs from the float64 value of its formula by more than this kernel does;
//   * the aggregate is float64, reduced in a fixed order (per-row values, then one workgroup per metric): bit-reproducible.
// Latency-bound (a few KB per row): no MFMA.
#include "../../include/vodhip.h"
#include "vodhip_internal.h"
#include "wg_sort.h"

namespace vodhip {

constexpr int MT_THREADS = 256;
typedef unsigned long long u64;

struct MtSum {
    static __device__ __forceinline__ double op(double a, double b) { return a + b; }
};
struct MtMax {
    static __device__ __forceinline__ double op(double a, double b) { return fmax(a, b); }
};

// Workgroup reduction of N doubles in a fixed order (wave butterfly, then the four wave results left to right).  All threads call it;
// `red` holds 4 * N doubles.  Counts and float32 values travel as doubles: exact.
template <typename Op, int N>
__device__ __forceinline__ void mt_block_reduce(double (&v)[N], double* red) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] = Op::op(v[k], __shfl_xor(v[k], o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) red[(threadIdx.x >> 6) * N + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = Op::op(Op::op(red[k], red[N + k]), Op::op(red[2 * N + k], red[3 * N + k]));
}

// order-preserving image of a non-NaN float (-0.0 -> +0.0) and its inverse
__device__ __forceinline__ unsigned mt_ord32(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float mt_unord32(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ __forceinline__ bool mt_finite(float v) { return fabsf(v) < __builtin_inff(); }  // false for NaN

__global__ __launch_bounds__(MT_THREADS) void retrieval_metrics_kernel(const float* __restrict__ scores,
                                                                       const int64_t* __restrict__ relevances, int64_t B, int width,
                                                                       int P, MetricSpecs specs, float* __restrict__ values) {
    extern __shared__ __attribute__((aligned(16))) char mt_smem[];
    u64* keys = (u64*)mt_smem;            // [P] sort buffer: the row's ranking keys, later the cut relevances of ndcg
    float* rs = (float*)(keys + P);       // [P] ranked scores (masked)
    float* rr = rs + P;                   // [P] ranked relevances as float32 (masked), the reference's `.to(ranked_scores)`
    double* red = (double*)(rr + P);      // [12]
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const float* sc = scores + row * width;
    const int64_t* rl = relevances + row * width;
    const float ninf = -__builtin_inff();

    // ---- mask + rank (functional.py:15-25): key = (monotone(score) << 32) | (0xFFFFFFFF - column); the padding key 0 sorts last ----
    int c_pos = 0;
    for (int i = tid; i < P; i += MT_THREADS) {
        u64 k = 0ull;
        if (i < width) {
            float s = sc[i];
            c_pos += rl[i] > 0;  // before the masking (:172)
            if (s != s || s == __builtin_inff()) s = ninf;
            k = ((u64)mt_ord32(s) << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
        }
        keys[i] = k;
    }
    __syncthreads();
    (void)wg_sort_lds_256<true, u64>(keys, P, tid);
    for (int j = tid; j < width; j += MT_THREADS) {
        const unsigned col = 0xFFFFFFFFu - (unsigned)(keys[j] & 0xFFFFFFFFull);
        const float s = sc[col];
        const bool masked = s != s || s == __builtin_inff();
        rs[j] = masked ? ninf : s;
        rr[j] = masked ? 0.f : (float)rl[col];
    }
    double np_[1] = {(double)c_pos};
    mt_block_reduce<MtSum>(np_, red);  // (its barriers also publish rs / rr)
    const float n_positives = (float)np_[0];

    for (int sp = 0; sp < specs.n; ++sp) {
        const int metric = specs.metric[sp];
        const int topk = specs.topk[sp];
        const int n = (topk > 0 && topk < width) ? topk : width;  // the cut (:174-176)
        float out = 0.f;
        switch (metric) {
            case VODHIP_METRIC_MRR:
            case VODHIP_METRIC_HITRATE:
            case VODHIP_METRIC_PRECISION:
            case VODHIP_METRIC_RECALL: {
                double cnt[2] = {0.0, 0.0};   // relevant entries, finite scores
                double first[1] = {-(double)width};  // -(index of the first relevant entry)
                for (int j = tid; j < n; j += MT_THREADS) {
                    if (rr[j] > 0.f) {
                        cnt[0] += 1.0;
                        first[0] = fmax(first[0], -(double)j);
                    }
                    cnt[1] += mt_finite(rs[j]) ? 1.0 : 0.0;
                }
                mt_block_reduce<MtSum>(cnt, red);
                mt_block_reduce<MtMax>(first, red);
                const float n_rel = (float)cnt[0];
                if (metric == VODHIP_METRIC_MRR) out = n_rel > 0.f ? __fdiv_rn(1.0f, (float)(1.0 - first[0])) : 0.f;
                else if (metric == VODHIP_METRIC_HITRATE) out = n_rel > 0.f ? 1.f : 0.f;
                else if (metric == VODHIP_METRIC_PRECISION) out = __fdiv_rn(n_rel, (float)cnt[1]);
                else out = __fdiv_rn(n_rel, n_positives);
                break;
            }
            case VODHIP_METRIC_NDCG: {
                // the ideal order of the CUT list (:158): a second descending sort, of the n cut relevances
                int P2 = 256;
                while (P2 < n) P2 <<= 1;
                for (int j = tid; j < P2; j += MT_THREADS) keys[j] = j < n ? (((u64)mt_ord32(rr[j]) << 32) | 1ull) : 0ull;
                __syncthreads();
                (void)wg_sort_lds_256<true, u64>(keys, P2, tid);
                double g[2] = {0.0, 0.0};  // dcg, idcg
                for (int j = tid; j < n; j += MT_THREADS) {
                    const double lg = log2((double)(j + 2));
                    g[0] += (double)rr[j] / lg;
                    g[1] += (double)mt_unord32((unsigned)(keys[j] >> 32)) / lg;
                }
                mt_block_reduce<MtSum>(g, red);
                out = g[1] > 0.0 ? (float)(g[0] / g[1]) : 0.f;
                break;
            }
            case VODHIP_METRIC_KLDIV: {
                // data: log-softmax over the graded relevances of the cut's positives; model: log-softmax over its finite scores
                double mx[2] = {-__builtin_inf(), -__builtin_inf()};
                double cnt[1] = {0.0};
                for (int j = tid; j < n; j += MT_THREADS) {
                    if (rr[j] > 0.f) {
                        mx[0] = fmax(mx[0], (double)rr[j]);
                        cnt[0] += 1.0;
                    }
                    if (mt_finite(rs[j])) mx[1] = fmax(mx[1], (double)rs[j]);
                }
                mt_block_reduce<MtMax>(mx, red);
                mt_block_reduce<MtSum>(cnt, red);
                double se[2] = {0.0, 0.0};
                for (int j = tid; j < n; j += MT_THREADS) {
                    if (rr[j] > 0.f) se[0] += exp((double)rr[j] - mx[0]);
                    if (mt_finite(rs[j])) se[1] += exp((double)rs[j] - mx[1]);
                }
                mt_block_reduce<MtSum>(se, red);
                const double lse_d = log(se[0]), lse_m = log(se[1]);
                double kl[1] = {0.0};
                for (int j = tid; j < n; j += MT_THREADS) {
                    if (rr[j] > 0.f && mt_finite(rs[j])) {  // both log-probabilities finite (:101-105)
                        const double dl = ((double)rr[j] - mx[0]) - lse_d;
                        const double ml = ((double)rs[j] - mx[1]) - lse_m;
                        kl[0] += exp(dl) * (dl - ml);
                    }
                }
                mt_block_reduce<MtSum>(kl, red);
                out = cnt[0] > 0.0 ? (float)kl[0] : __builtin_nanf("");
                break;
            }
            case VODHIP_METRIC_MIN:
            case VODHIP_METRIC_MAX: {
                const double sgn = metric == VODHIP_METRIC_MIN ? -1.0 : 1.0;
                double m[1] = {-__builtin_inf()};
                for (int j = tid; j < n; j += MT_THREADS)
                    if (mt_finite(rs[j])) m[0] = fmax(m[0], sgn * (double)rs[j]);
                mt_block_reduce<MtMax>(m, red);
                out = (float)(sgn * m[0]);
                break;
            }
            default: {  // VODHIP_METRIC_ENTROPY
                double m[1] = {-__builtin_inf()};
                for (int j = tid; j < n; j += MT_THREADS) m[0] = fmax(m[0], (double)rs[j]);
                mt_block_reduce<MtMax>(m, red);
                double se[1] = {0.0};
                for (int j = tid; j < n; j += MT_THREADS)
                    if (mt_finite(rs[j])) se[0] += exp((double)rs[j] - m[0]);
                mt_block_reduce<MtSum>(se, red);
                const double lse = log(se[0]);
                double h[1] = {0.0};
                for (int j = tid; j < n; j += MT_THREADS)
                    if (mt_finite(rs[j])) h[0] += -(exp((double)rs[j]) * (((double)rs[j] - m[0]) - lse));  // exp(SCORE): the quirk
                mt_block_reduce<MtSum>(h, red);
                out = (float)h[0];
                break;
            }
        }
        if (tid == 0) values[(int64_t)sp * B + row] = out;
    }
}

// MeanAggregator.update (aggregator.py:43-50) of every metric: one workgroup per metric adds the float64 sum and the number of its
// non-NaN row values to state[metric] = (total, count), in a fixed order.
__global__ __launch_bounds__(MT_THREADS) void metrics_aggregate_kernel(const float* __restrict__ values, int64_t B,
                                                                       double* __restrict__ state) {
    __shared__ double red[8];
    const int m = blockIdx.x, tid = threadIdx.x;
    double v[2] = {0.0, 0.0};
    for (int64_t i = tid; i < B; i += MT_THREADS) {
        const float x = values[(int64_t)m * B + i];
        if (x == x) {
            v[0] += (double)x;
            v[1] += 1.0;
        }
    }
    mt_block_reduce<MtSum>(v, red);
    if (tid == 0) {
        state[2 * m] += v[0];
        state[2 * m + 1] += v[1];
    }
}

hipError_t launch_retrieval_metrics(const float* scores, const int64_t* relevances, int64_t B, int width, const MetricSpecs& specs,
                                    float* values, double* state, hipStream_t stream) {
    int P = 256;
    while (P < width) P <<= 1;
    const size_t lds = (size_t)P * 16 + 12 * sizeof(double);
    if (lds > 64 * 1024) {
        hipError_t e = allow_dynamic_lds((const void*)retrieval_metrics_kernel, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(retrieval_metrics_kernel, dim3((unsigned)B), dim3(MT_THREADS), lds, stream, scores, relevances, B, width, P,
                       specs, values);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !state) return e;
    hipLaunchKernelGGL(metrics_aggregate_kernel, dim3((unsigned)specs.n), dim3(MT_THREADS), 0, stream, values, B, state);
    return hipGetLastError();
}

}  // namespace vodhip
