// Host-side pieces of the posterior read-out (kernels_readout.hip, include/vodhip.h H2e): the argument checks shared by the flat and
// the node entry points, the split of a node index's value table by shard row ranges, and the fold of the per-shard results.  Plain
// C++ (no HIP): tests/sanitize/readout_fold_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include "partition_fold.h"

namespace vodhip {

constexpr int64_t READOUT_MAX_COLS = 256;  // VODHIP_READOUT_MAX_COLS

// columns of the table as the kernel reads it: whole 64-column slices
inline int64_t readout_c_pad(int64_t n_cols) { return (n_cols + 63) / 64 * 64; }

// set_row_values with a table (values != NULL): the refusals that need no device; `ntotal` = the rows the index holds
inline const char* row_values_args_error(int64_t n_rows, int64_t n_cols, int src_dtype, int location, int64_t ntotal) {
    if (src_dtype < 0 || src_dtype > 2) return "invalid src_dtype";
    if (location != 0 && location != 1) return "invalid location";
    if (n_cols < 1 || n_cols > READOUT_MAX_COLS) return "n_cols must be in [1, 256]";
    if (n_rows != ntotal) return "n_rows must equal ntotal";
    return nullptr;
}

// the read-out call: log_partition's refusals, then the output
inline const char* posterior_expectation_args_error(const void* queries, int q_dtype, int64_t nq, float beta, const void* q_labels, int n_per_query,
                                                    const void* out_max, const void* out_log_rel, const void* out_values) {
    if (const char* msg = log_partition_args_error(queries, q_dtype, nq, beta, q_labels, n_per_query, out_max, out_log_rel)) return msg;
    if (nq > 0 && !out_values) return "invalid query / output pointers";
    return nullptr;
}

// Shard g of a node index owns the global rows [g * rows_per_shard, (g + 1) * rows_per_shard): of a table of n_rows rows it holds
// rows [*lo, *hi) - an empty range (lo == hi == n_rows) for a shard past the table's end.
inline void readout_shard_rows(int64_t n_rows, int64_t rows_per_shard, int g, int64_t* lo, int64_t* hi) {
    *lo = std::min<int64_t>(n_rows, (int64_t)g * rows_per_shard);
    *hi = std::min<int64_t>(n_rows, *lo + rows_per_shard);
}

// Folds the results of `n_shards` shards, shard g's at parts + g * per_shard floats laid out [max nq | log_rel nq | values nq * n_cols]:
// the pair by fold_log_partition, the value rows by fold_posterior_mean with dim = n_cols (partition_fold.h): in increasing shard
// order, in double, a shard with no eligible row carries weight 0 and its rows are not read.
inline void fold_posterior_expectation(const float* parts, int n_shards, int64_t nq, int64_t n_cols, float beta, float* out_max, float* out_log_rel,
                                       float* out_values) {
    const int64_t per_shard = nq * (2 + n_cols);
    fold_log_partition(parts, parts + nq, n_shards, per_shard, nq, beta, out_max, out_log_rel);
    fold_posterior_mean(parts, parts + nq, parts + 2 * nq, n_shards, per_shard, per_shard, nq, n_cols, beta, out_max, out_log_rel, out_values);
}

}  // namespace vodhip
