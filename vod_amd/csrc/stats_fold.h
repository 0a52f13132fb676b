// Host-side pieces of the posterior-statistics call (kernels_stats.hip): the argument checks shared by the flat and the node entry
// point, and the fold of the per-shard (max, log_rel, mean_rel, var) words of a node index.  Plain C++ (no HIP):
// tests/sanitize/stats_fold_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include "partition_fold.h"

namespace vodhip {

// the refusals that need no index state behind those of log_partition_args_error; the message of the first one that applies, or nullptr
inline const char* posterior_stats_args_error(const void* queries, int q_dtype, int64_t nq, float beta, const void* q_labels, int n_per_query,
                                              const void* out_max, const void* out_log_rel, const void* out_mean_rel, const void* out_var) {
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, out_max, out_log_rel)) return msg;
    if (nq > 0 && (!out_mean_rel || !out_var)) return "invalid query / output pointers";
    return nullptr;
}

// One query's fold in double; shard g's words at {max_g, log_rel_g, mean_rel_g, var_g}[g * stride], T = float (the shards' words) or
// double (tests/sanitize/stats_fold_check.cpp folds folds).  A shard is a mixture component: relative to the folded maximum M it has
//   weight  w_g = exp(beta (max_g - M) + log_rel_g - log_rel),   log_rel = log sum_g exp(beta (max_g - M) + log_rel_g)  (unrounded),
//   mean    u_g = mean_rel_g + max_g - M,
//   mean_rel = sum_g w_g u_g,   var = max(0, sum_g w_g (var_g + u_g^2) - mean_rel^2),
// summed in increasing shard order.  A shard with no eligible row holds (-inf, -inf, NaN, NaN), carries weight 0 and its statistics are
// not read.  A folded maximum that is not finite (all shards empty: -inf; a +inf score: +inf) -> (M, M, NaN, NaN).
template <class T>
inline void fold_posterior_stats_query(const T* max_g, const T* log_rel_g, const T* mean_rel_g, const T* var_g, int n_shards, int64_t stride,
                                       double beta, double out[4]) {
    const double inf = std::numeric_limits<double>::infinity();
    double m = -inf;
    for (int g = 0; g < n_shards; ++g) {
        const double v = (double)max_g[(int64_t)g * stride];
        if (v > m) m = v;
    }
    if (m == inf || m == -inf) {
        out[0] = out[1] = m;
        out[2] = out[3] = std::numeric_limits<double>::quiet_NaN();
        return;
    }
    double sum = 0.0, first = 0.0, second = 0.0;
    for (int g = 0; g < n_shards; ++g) {
        const int64_t at = (int64_t)g * stride;
        const double mg = (double)max_g[at], lg = (double)log_rel_g[at];
        if (mg == -inf || lg == -inf) continue;
        const double w = std::exp(beta * (mg - m) + lg);  // (before the division by the sum)
        const double u = (double)mean_rel_g[at] + (mg - m);
        sum += w;
        first += w * u;
        second += w * ((double)var_g[at] + u * u);
    }
    const double mean = first / sum;
    const double var = second / sum - mean * mean;
    out[0] = m;
    out[1] = std::log(sum);
    out[2] = mean;
    out[3] = var > 0.0 ? var : 0.0;
}

// Every query of a node call: shard g's words of query q at [g * stride + q].  (out_max, out_log_rel) are fold_log_partition's - the
// words vodhip_node_index_log_partition returns -, the two statistics the fold above rounded to float32 once.
inline void fold_posterior_stats(const float* max_g, const float* log_rel_g, const float* mean_rel_g, const float* var_g, int n_shards,
                                 int64_t stride, int64_t nq, float beta, float* out_max, float* out_log_rel, float* out_mean_rel,
                                 float* out_var) {
    fold_log_partition(max_g, log_rel_g, n_shards, stride, nq, beta, out_max, out_log_rel);
    for (int64_t q = 0; q < nq; ++q) {
        double w[4];
        fold_posterior_stats_query(max_g + q, log_rel_g + q, mean_rel_g + q, var_g + q, n_shards, stride, (double)beta, w);
        out_mean_rel[q] = (float)w[2];
        out_var[q] = (float)w[3];
    }
}

}  // namespace vodhip
