// Host side of sample_posterior (include/vodhip.h H2s): the argument checks that need no device, and the merge of the per-shard
// sample lists of a node index.  Plain C++ (no HIP): tests/sanitize/sample_fold_check.cpp compiles this header alone under the
// sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace vodhip {

// The argument errors of vodhip_index_sample_posterior / vodhip_node_index_sample_posterior behind those of log_partition_args_error,
// or nullptr.
inline const char* sample_posterior_args_error(int64_t nq, int k, int64_t query_offset, int64_t id_base, const void* out_ids,
                                               const void* out_scores, const void* out_log_p, const void* out_log_weight,
                                               const void* out_keys) {
    if (k < 1 || k > 255) return "k must be in [1, 255]";
    if (query_offset < 0 || nq > (1ll << 32) || query_offset > (1ll << 32) - nq) return "query_offset must be >= 0 and query_offset + nq <= 2^32";
    if (id_base < 0) return "id_base must be >= 0";
    if (nq > 0 && (!out_ids || !out_scores || !out_log_p || !out_log_weight || !out_keys)) return "invalid query / output pointers";
    return nullptr;
}

// The priority-sampling words of one drawn row from the float32 words of the call, in double:
//   log_p = beta (s - max) - log_rel,  log_tau = (key_tau - beta max) - log_rel (key_tau = -inf: -inf),
//   log_weight = log_p - log(-expm1(-exp(log_p - log_tau)))  (log_tau = -inf: log_p).
inline void sample_weight(float beta, float s, float key_tau, float max_score, float log_rel, float* log_p, float* log_weight) {
    const double lp = (double)beta * ((double)s - (double)max_score) - (double)log_rel;
    const double lt = key_tau == -std::numeric_limits<float>::infinity()
                          ? -std::numeric_limits<double>::infinity()
                          : ((double)key_tau - (double)beta * (double)max_score) - (double)log_rel;
    *log_p = (float)lp;
    *log_weight = (float)(lp - std::log(-std::expm1(-std::exp(lp - lt))));
}

// Merges the lists of `n_shards` shards.  Shard g holds, for query q, keys_g[g * key_stride + q * (k + 1) ..] (k + 1 unnormalised keys,
// descending, -inf padded), ids_g[g * id_stride + q * k ..] and scores_g[g * score_stride + q * k ..] (the rows of the first k keys; pads id -1).  The k + 1 best
// of the union by (key desc, id asc) are the k + 1 best of the whole store; a shard's (k + 1)-th key carries no row and sorts behind
// every row of an equal key - it can only land at rank k + 1 or later, where the key alone is read.  (out_max, out_log_rel): the
// FOLDED pair of fold_log_partition.  A query whose folded pair is not finite is all pads.
inline void fold_sample_posterior(const float* keys_g, const int64_t* ids_g, const float* scores_g, int n_shards, int64_t key_stride,
                                  int64_t id_stride, int64_t score_stride, int64_t nq, int k, float beta, const float* out_max, const float* out_log_rel,
                                  int64_t* out_ids, float* out_scores, float* out_log_p, float* out_log_weight, float* out_keys) {
    const float inf = std::numeric_limits<float>::infinity();
    struct Entry {
        float key;
        int64_t id;  // -1: a shard's (k + 1)-th key
        float score;
    };
    std::vector<Entry> all;
    all.reserve((size_t)(n_shards > 0 ? n_shards : 0) * (size_t)(k + 1));
    for (int64_t q = 0; q < nq; ++q) {
        int64_t* ids = out_ids + q * k;
        float* sc = out_scores + q * k;
        float* lp = out_log_p + q * k;
        float* lw = out_log_weight + q * k;
        float* keys = out_keys + q * (k + 1);
        for (int p = 0; p < k; ++p) {
            ids[p] = -1;
            sc[p] = lp[p] = lw[p] = -inf;
        }
        for (int p = 0; p <= k; ++p) keys[p] = -inf;
        const float m = out_max[q], lr = out_log_rel[q];
        if (!(m > -inf && m < inf && lr > -inf && lr < inf)) continue;
        all.clear();
        for (int g = 0; g < n_shards; ++g) {
            const float* kg = keys_g + (int64_t)g * key_stride + q * (k + 1);
            const int64_t* ig = ids_g + (int64_t)g * id_stride + q * k;
            const float* sg = scores_g + (int64_t)g * score_stride + q * k;
            for (int p = 0; p <= k; ++p) {
                if (!(kg[p] > -inf)) break;  // (the pads follow the keys)
                if (p < k && ig[p] < 0) break;
                all.push_back(Entry{kg[p], p < k ? ig[p] : (int64_t)-1, p < k ? sg[p] : -inf});
            }
        }
        std::sort(all.begin(), all.end(), [](const Entry& a, const Entry& b) {
            if (a.key != b.key) return a.key > b.key;
            if ((a.id < 0) != (b.id < 0)) return b.id < 0;
            return a.id < b.id;
        });
        const size_t n = all.size();
        const float key_tau = n > (size_t)k ? all[(size_t)k].key : -inf;
        for (size_t p = 0; p < n && p <= (size_t)k; ++p) keys[p] = all[p].key;
        for (size_t p = 0; p < n && p < (size_t)k; ++p) {
            ids[p] = all[p].id;
            sc[p] = all[p].score;
            sample_weight(beta, all[p].score, key_tau, m, lr, &lp[p], &lw[p]);
        }
    }
}

}  // namespace vodhip
