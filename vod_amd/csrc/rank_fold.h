// Host-side pieces of the rank calls (kernels_rank.hip): the argument checks shared by the flat and the node entry points, and the two
// folds of a node index - the per-shard scan scores of listed rows combined by OWNERSHIP (no comparison of values), and the per-shard
// counts added in int64.  Plain C++ (no HIP): tests/sanitize/rank_fold_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include <cstdint>
#include <limits>

namespace vodhip {

constexpr int64_t RANK_FOLD_MAX_LISTED = 64;  // = VODHIP_RANK_MAX_LISTED (include/vodhip.h)

// the refusals that need no index state; the message of the first one that applies, or nullptr
inline const char* rank_args_error(const void* queries, int q_dtype, int64_t nq, int64_t m, const void* q_labels, int n_per_query) {
    if (nq < 0 || (nq > 0 && !queries)) return "invalid query pointer";
    if (q_dtype < 0 || q_dtype > 2) return "invalid q_dtype";
    if (m < 1 || m > RANK_FOLD_MAX_LISTED) return "m must be in [1, 64]";
    if (q_labels && (n_per_query < 1 || n_per_query > 64)) return "n_per_query must be in [1, 64]";
    return nullptr;
}

// Shard g of `n_shards` owns the global ids [g * rows_per_shard, (g + 1) * rows_per_shard); its scores of the n slots are at
// score_g[g * n + i], its local rows (-1 = absent there) at row_g[g * n + i].  Slot i takes the score of the shard that owns ids[i], as
// that shard computed it; a slot nobody owns (id < 0, id past the last shard) or that its owner calls absent is absent:
// out_score = -inf, out_present = 0.  No values are compared: a present row that scores -inf stays present.
inline void combine_scan_scores(const float* score_g, const int32_t* row_g, const int64_t* ids, int64_t n, int n_shards, int64_t rows_per_shard,
                                float* out_score, uint8_t* out_present) {
    const float ninf = -std::numeric_limits<float>::infinity();
    for (int64_t i = 0; i < n; ++i) {
        const int64_t id = ids[i];
        float s = ninf;
        uint8_t present = 0;
        if (id >= 0 && rows_per_shard > 0) {
            const int64_t g = id / rows_per_shard;
            if (g < (int64_t)n_shards && row_g[g * n + i] >= 0) {
                s = score_g[g * n + i];
                present = 1;
            }
        }
        out_score[i] = s;
        out_present[i] = present;
    }
}

// The thresholds every shard counts against: the combined score, NaN for an absent slot (a NaN threshold counts -1 on every shard).
inline void rank_thresholds(const float* score, const uint8_t* present, int64_t n, float* out) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t i = 0; i < n; ++i) out[i] = present[i] ? score[i] : nan;
}

// out[i] = sum over the shards of count_g[g * n + i], in int64 (a shard's count is below 2^31, their sum need not be); -1 as soon as
// one shard says -1 (a NaN threshold says so on every shard).
inline void sum_counts(const int64_t* count_g, int64_t n, int n_shards, int64_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        int64_t sum = 0;
        bool none = false;
        for (int g = 0; g < n_shards; ++g) {
            const int64_t c = count_g[(int64_t)g * n + i];
            if (c < 0) none = true;
            else sum += c;
        }
        out[i] = none ? -1 : sum;
    }
}

}  // namespace vodhip
