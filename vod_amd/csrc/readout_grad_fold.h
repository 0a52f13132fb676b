// Host-side pieces of the read-out's gradient in the query (kernels_readout_grad.hip, include/vodhip.h H2b): the argument checks shared
// by the flat and the node entry points and the fold of the per-shard results.  Plain C++ (no HIP):
// tests/sanitize/readout_grad_fold_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include "readout_fold.h"

namespace vodhip {

// the backward call: H2e's refusals (the forward's two words are inputs here and checked like its outputs), then the NULL inputs
inline const char* posterior_expectation_backward_args_error(const void* queries, int q_dtype, int64_t nq, float beta, const void* q_labels, int n_per_query,
                                                             const void* max_score, const void* log_rel, const void* values, const void* grad_values,
                                                             const void* out_grad_queries) {
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, max_score, log_rel)) return msg;
    if (nq > 0 && !values) return "values is NULL";
    if (nq > 0 && !grad_values) return "grad_values is NULL";
    if (nq > 0 && !out_grad_queries) return "invalid query / output pointers";
    return nullptr;
}

// Every shard ran with the GLOBAL (max_score, log_rel, values): its result is the sum over its own rows of the one formula, so the
// shards simply add.  Shard g's rows at parts + g * nq * dim; in increasing shard order, in double, rounded once.
inline void fold_posterior_expectation_backward(const float* parts, int n_shards, int64_t nq, int64_t dim, float* out_grad_queries) {
    const int64_t n = nq * dim;
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int g = 0; g < n_shards; ++g) s += (double)parts[(int64_t)g * n + i];
        out_grad_queries[i] = (float)s;
    }
}

}  // namespace vodhip
