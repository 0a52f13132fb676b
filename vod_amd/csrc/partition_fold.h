// Host-side pieces of the log-partition call (kernels_partition.hip): the argument checks shared by the flat and the node entry
// point, and the fold of per-shard (max, log_rel) pairs of a node index.  Plain C++ (no HIP): tests/sanitize/partition_fold_check.cpp
// compiles this header alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace vodhip {

// the refusals that need no index state; the message of the first one that applies, or nullptr
inline const char* log_partition_args_error(const void* queries, int q_dtype, int64_t nq, float beta, const void* q_labels,
                                            int n_per_query, const void* out_max, const void* out_log_rel) {
    if (nq < 0 || (nq > 0 && (!queries || !out_max || !out_log_rel))) return "invalid query / output pointers";
    if (q_dtype < 0 || q_dtype > 2) return "invalid q_dtype";
    if (!(beta > 0.f) || !std::isfinite(beta)) return "beta must be finite and > 0";
    if (q_labels && (n_per_query < 1 || n_per_query > 64)) return "n_per_query must be in [1, 64]";
    return nullptr;
}

// Folds the pairs of `n_shards` shards, shard g's at max_g[g * stride + q] / log_rel_g[g * stride + q], in increasing shard order:
//   max = max_g max_g,  log_rel = log sum_g exp(beta (max_g - max) + log_rel_g).
// A shard with no eligible row holds (-inf, -inf) and contributes nothing; all shards empty -> (-inf, -inf); a +inf maximum ->
// (+inf, +inf).  The sum runs in double: its rounding is far below the float32 spacing of the result.
inline void fold_log_partition(const float* max_g, const float* log_rel_g, int n_shards, int64_t stride, int64_t nq, float beta,
                               float* out_max, float* out_log_rel) {
    const float inf = std::numeric_limits<float>::infinity();
    for (int64_t q = 0; q < nq; ++q) {
        float m = -inf;
        for (int g = 0; g < n_shards; ++g) {
            const float v = max_g[(int64_t)g * stride + q];
            if (v > m) m = v;
        }
        if (m == inf || m == -inf) {
            out_max[q] = m;
            out_log_rel[q] = m;
            continue;
        }
        double sum = 0.0;
        for (int g = 0; g < n_shards; ++g) {
            const float mg = max_g[(int64_t)g * stride + q], lg = log_rel_g[(int64_t)g * stride + q];
            if (mg == -inf || lg == -inf) continue;
            sum += std::exp((double)beta * ((double)mg - (double)m) + (double)lg);
        }
        out_max[q] = m;
        out_log_rel[q] = (float)std::log(sum);
    }
}

// The posterior means of `n_shards` shards (kernels_posterior.hip), shard g's row of query q at mean_g[g * mean_stride + q * dim], with
// the shard pairs as above and the FOLDED pair (out_max, out_log_rel) of fold_log_partition: in increasing shard order, in double,
//   mean[q, :] = sum_g w_g mean_g[q, :],  w_g = exp(beta (max_g - max) + log_rel_g - log_rel).
// A shard with no eligible row carries weight 0 and its row is not read; a query whose folded maximum is not finite gets the zero row.
inline void fold_posterior_mean(const float* max_g, const float* log_rel_g, const float* mean_g, int n_shards, int64_t stride,
                                int64_t mean_stride, int64_t nq, int64_t dim, float beta, const float* out_max, const float* out_log_rel,
                                float* out_mean) {
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<double> sum((size_t)(dim > 0 ? dim : 0));
    for (int64_t q = 0; q < nq; ++q) {
        float* row = out_mean + q * dim;
        const float m = out_max[q], lr = out_log_rel[q];
        if (m == inf || m == -inf || !(m == m)) {
            for (int64_t d = 0; d < dim; ++d) row[d] = 0.f;
            continue;
        }
        std::fill(sum.begin(), sum.end(), 0.0);
        for (int g = 0; g < n_shards; ++g) {
            const float mg = max_g[(int64_t)g * stride + q], lg = log_rel_g[(int64_t)g * stride + q];
            if (mg == -inf || lg == -inf) continue;
            const double w = std::exp((double)beta * ((double)mg - (double)m) + (double)lg - (double)lr);
            const float* src = mean_g + (int64_t)g * mean_stride + q * dim;
            for (int64_t d = 0; d < dim; ++d) sum[(size_t)d] += w * (double)src[d];
        }
        for (int64_t d = 0; d < dim; ++d) row[d] = (float)sum[(size_t)d];
    }
}

}  // namespace vodhip
