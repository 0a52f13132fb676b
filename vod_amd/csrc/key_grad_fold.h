// Host-side pieces of the posterior's gradient in the stored rows (kernels_key_grad.hip, include/vodhip.h H2k): the argument checks
// shared by the flat and the node entry points, and the column maxima a node index hands to its shards.  The slab a shard owns is the
// adjoint's (place_posterior_adjoint_slab with n_cols = dim).  Plain C++ (no HIP): tests/sanitize/key_grad_check.cpp compiles this
// header alone under the sanitizers.
#pragma once
#include "readout_adjoint_fold.h"

namespace vodhip {

constexpr int64_t KEY_GRAD_SLICE = 1024;  // queries of one scan launch: later slices add to the result in slice order

// the key-gradient call: log_partition's refusals (the forward's two words are inputs here and checked like its outputs), then the
// gradients.  `out` is needed whenever the index may hold a row
inline const char* posterior_key_gradient_args_error(const void* queries, int q_dtype, int64_t nq, float beta, const void* q_labels, int n_per_query,
                                                     const void* max_score, const void* log_rel, const void* grad_log_z, const void* values,
                                                     const void* grad_values, const void* out) {
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, max_score, log_rel)) return msg;
    if (!grad_log_z && !grad_values) return "grad_log_z and grad_values are both NULL";
    if (grad_values && !values) return "grad_values without values";
    if (!out) return "out is NULL";
    return nullptr;
}

// The batch-wide scales are functions of (grad_log_z, grad_values, values, vmax) alone.  A node index hands every shard the GLOBAL
// first three; this makes the fourth global as well: vmax[c] = the largest of the shards' cached column maxima (shard g's at
// parts + g * c_pad), the column maximum over all the rows.  Every shard then forms the same scales as one index holding all the rows.
inline void fold_key_grad_vmax(const float* parts, int n_shards, int64_t c_pad, float* vmax) {
    for (int64_t c = 0; c < c_pad; ++c) {
        float m = 0.f;
        for (int g = 0; g < n_shards; ++g) m = std::max(m, parts[(int64_t)g * c_pad + c]);
        vmax[c] = m;
    }
}

}  // namespace vodhip
