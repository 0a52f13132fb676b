// Host-side pieces of the read-out's adjoint (kernels_readout_adjoint.hip, include/vodhip.h H2a): the argument checks shared by the flat
// and the node entry points, the padded width of the weights, and the slab of the result a shard of a node index owns.  Plain C++ (no
// HIP): tests/sanitize/readout_adjoint_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include "readout_fold.h"

#include <cstring>

namespace vodhip {

constexpr int64_t READOUT_ADJOINT_SLICE = 1024;  // queries of one scan launch: later slices add to the result in slice order

// columns of the weights as the kernel reads them: whole 64-column slices (the read-out's)
inline int64_t readout_adjoint_c_pad(int64_t n_cols) { return readout_c_pad(n_cols); }

// the adjoint call: log_partition's refusals (the forward's two words are inputs here and checked like its outputs), then the width
// and the NULL pointers.  The width is refused for every nq; `out` is needed whenever the index may hold a row
inline const char* posterior_adjoint_args_error(const void* queries, int q_dtype, int64_t nq, float beta, const void* q_labels, int n_per_query,
                                                const void* max_score, const void* log_rel, const void* weights, int64_t n_cols, const void* out) {
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, max_score, log_rel)) return msg;
    if (n_cols < 1 || n_cols > READOUT_MAX_COLS) return "n_cols must be in [1, 256]";
    if (nq > 0 && !weights) return "weights is NULL";
    if (!out) return "out is NULL";
    return nullptr;
}

// Shard g of a node index computes the global rows [*lo, *hi) of the result (readout_shard_rows) from the GLOBAL (max_score, log_rel):
// an element depends on its row and the queries alone, so the slabs are concatenated and nothing is folded.  Shard g's slab sits at
// parts + g * slab_stride floats; rows [lo, hi) of `out` [ntotal][n_cols] receive it.
inline void place_posterior_adjoint_slab(const float* parts, int64_t slab_stride, int g, int64_t ntotal, int64_t rows_per_shard, int64_t n_cols, float* out) {
    int64_t lo, hi;
    readout_shard_rows(ntotal, rows_per_shard, g, &lo, &hi);
    if (hi > lo) std::memcpy(out + lo * n_cols, parts + (int64_t)g * slab_stride, (size_t)((hi - lo) * n_cols) * sizeof(float));
}

}  // namespace vodhip
