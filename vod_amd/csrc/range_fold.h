// Host-side pieces of range_search (kernels_range.hip): the argument checks shared by the flat and the node entry points, and the fold
// of a node index - the per-shard CSR lists of a query concatenated in shard order, which is ascending id order since shards own
// ascending id ranges.  Plain C++ (no HIP): tests/sanitize/range_fold_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace vodhip {

// the refusals that need no index state; the message of the first one that applies, or nullptr
inline const char* range_args_error(const void* queries, int q_dtype, int64_t nq, const void* thresholds, const void* q_labels, int n_per_query,
                                    const void* lims, const void* out_scores, const void* out_ids, int64_t capacity) {
    if (nq < 0 || (nq > 0 && !queries)) return "invalid query pointer";
    if (q_dtype < 0 || q_dtype > 2) return "invalid q_dtype";
    if (q_labels && (n_per_query < 1 || n_per_query > 64)) return "n_per_query must be in [1, 64]";
    if (nq > 0 && !thresholds) return "thresholds is NULL";
    if (!lims) return "lims is NULL";
    if ((out_scores == nullptr) != (out_ids == nullptr)) return "out_scores and out_ids must both be given or both be NULL";
    if (capacity < 0) return "capacity must be >= 0";
    return nullptr;
}

// lims_g: [n_shards][nq + 1], shard g's own CSR limits.  lims [nq + 1]: lims[q + 1] - lims[q] = the sum of the shards' list lengths of
// query q, in int64.  Returns lims[nq].
inline int64_t fold_range_lims(const int64_t* lims_g, int n_shards, int64_t nq, int64_t* lims) {
    lims[0] = 0;
    for (int64_t q = 0; q < nq; ++q) {
        int64_t len = 0;
        for (int g = 0; g < n_shards; ++g) len += lims_g[(int64_t)g * (nq + 1) + q + 1] - lims_g[(int64_t)g * (nq + 1) + q];
        lims[q + 1] = lims[q] + len;
    }
    return lims[nq];
}

// Shard g's lists start at scores_g + g * shard_stride / ids_g + g * shard_stride and hold its first min(lims_g[g][nq], shard_stride)
// hits.  Query q's hits of shard 0, then of shard 1, ... go to positions lims[q] .. of out_scores / out_ids; a position at or past
// `capacity` is not written, a hit a shard did not hold (past shard_stride) is not read.
inline void fold_range_lists(const int64_t* lims_g, const float* scores_g, const int64_t* ids_g, int64_t shard_stride, int n_shards, int64_t nq,
                             const int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity) {
    for (int64_t q = 0; q < nq; ++q) {
        int64_t pos = lims[q];
        for (int g = 0; g < n_shards; ++g) {
            const int64_t b = lims_g[(int64_t)g * (nq + 1) + q], e = lims_g[(int64_t)g * (nq + 1) + q + 1];
            const int64_t n = std::min(std::min(e, shard_stride) - b, capacity - pos);  // what was held and what fits
            if (n > 0) {
                std::memcpy(out_scores + pos, scores_g + (int64_t)g * shard_stride + b, (size_t)n * sizeof(float));
                std::memcpy(out_ids + pos, ids_g + (int64_t)g * shard_stride + b, (size_t)n * sizeof(int64_t));
            }
            pos += e - b;
        }
    }
}

}  // namespace vodhip
