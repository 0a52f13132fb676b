// Host-side pieces of the posterior-divergence call (kernels_divergence.hip): the argument checks shared by the flat and the node entry
// point, and the fold of the per-shard words of a node index.  Plain C++ (no HIP): tests/sanitize/divergence_fold_check.cpp compiles
// this header alone under the sanitizers.
#pragma once
#include "partition_fold.h"

namespace vodhip {

// the refusals that need no index state; the message of the first one that applies, or nullptr.  out: the eight output pointers
inline const char* posterior_divergence_args_error(const void* queries_a, const void* queries_b, int q_dtype, int64_t nq, float beta_a, float beta_b,
                                                   const void* q_labels, int n_per_query, const void* const out[8]) {
    if (nq < 0 || nq > (1ll << 19)) return "invalid query / output pointers";
    if (nq > 0) {
        if (!queries_a || !queries_b) return "invalid query / output pointers";
        for (int k = 0; k < 8; ++k)
            if (!out[k]) return "invalid query / output pointers";
    }
    if (q_dtype < 0 || q_dtype > 2) return "invalid q_dtype";
    if (!(beta_a > 0.f) || !std::isfinite(beta_a)) return "beta_a must be finite and > 0";
    if (!(beta_b > 0.f) || !std::isfinite(beta_b)) return "beta_b must be finite and > 0";
    if (q_labels && (n_per_query < 1 || n_per_query > 64)) return "n_per_query must be in [1, 64]";
    return nullptr;
}

// One pair's fold in double.  words[k] points at shard 0's word k of the pair, shard g's at words[k][g * stride]; the words are
// (max_a, log_rel_a, mean_rel_a, cross_rel_ab, max_b, log_rel_b, mean_rel_b, cross_rel_ba); T = float (the shards' words) or double
// (tests/sanitize/divergence_fold_check.cpp folds folds).  A shard is a mixture component: relative to the folded maxima M_a, M_b,
//   weight     w^a_g = exp(beta_a (max_a_g - M_a) + log_rel_a_g - log_rel_a),  log_rel_a = log sum_g exp(..)  (unrounded), as stats_fold.h
//   mean_rel_a   = sum_g w^a_g (mean_rel_a_g + max_a_g - M_a)
//   cross_rel_ab = sum_g w^a_g (cross_rel_ab_g + max_b_g - M_b)
// and the mirror, summed in increasing shard order.  A shard in which a side has no eligible row (or no finite score) carries weight 0
// on that side and its words are not read; a shard in which side a has mass and side b has no finite score contributes -inf to
// cross_rel_ab (0 * inf is never formed: a weight that underflowed to 0 is left out).  A side whose folded maximum is not finite is
// (M, M, NaN), and both cross words are NaN then.
template <class T>
inline void fold_posterior_divergence_pair(const T* const words[8], int n_shards, int64_t stride, double beta_a, double beta_b, double out[8]) {
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double beta[2] = {beta_a, beta_b};
    double M[2] = {-inf, -inf};
    for (int s = 0; s < 2; ++s)
        for (int g = 0; g < n_shards; ++g) {
            const double v = (double)words[4 * s][(int64_t)g * stride];
            if (v > M[s]) M[s] = v;
        }
    const bool fin[2] = {M[0] != inf && M[0] != -inf, M[1] != inf && M[1] != -inf};
    for (int s = 0; s < 2; ++s) {
        const int o = 1 - s;
        out[4 * s] = M[s];
        if (!fin[s]) {
            out[4 * s + 1] = M[s];
            out[4 * s + 2] = out[4 * s + 3] = nan;
            continue;
        }
        double sum = 0.0, first = 0.0, cross = 0.0;
        for (int g = 0; g < n_shards; ++g) {
            const int64_t at = (int64_t)g * stride;
            const double mg = (double)words[4 * s][at], lg = (double)words[4 * s + 1][at];
            if (mg == -inf || lg == -inf) continue;
            const double w = std::exp(beta[s] * (mg - M[s]) + lg);  // (before the division by the sum)
            const double u = (double)words[4 * s + 2][at] + (mg - M[s]);
            sum += w;
            first += w * u;
            if (!fin[o] || w == 0.0) continue;
            const double mo = (double)words[4 * o][at];
            if (mo == -inf) cross += -inf;  // mass on rows the other side scores -inf
            else cross += w * ((double)words[4 * s + 3][at] + (mo - M[o]));
        }
        out[4 * s + 1] = std::log(sum);
        out[4 * s + 2] = first / sum;
        out[4 * s + 3] = fin[o] ? cross / sum : nan;
    }
}

// Every pair of a node call: shard g's word k of pair q at parts[(g * 8 + k) * nq + q].  (max, log_rel) of each side are
// fold_log_partition's - the words vodhip_node_index_log_partition returns for that side -, the other four the fold above rounded to
// float32 once.  out: the eight outputs in the order of the words.
inline void fold_posterior_divergence(const float* parts, int n_shards, int64_t nq, float beta_a, float beta_b, float* const out[8]) {
    const int64_t stride = 8 * nq;
    fold_log_partition(parts, parts + nq, n_shards, stride, nq, beta_a, out[0], out[1]);
    fold_log_partition(parts + 4 * nq, parts + 5 * nq, n_shards, stride, nq, beta_b, out[4], out[5]);
    for (int64_t q = 0; q < nq; ++q) {
        const float* words[8];
        for (int k = 0; k < 8; ++k) words[k] = parts + k * nq + q;
        double w[8];
        fold_posterior_divergence_pair<float>(words, n_shards, stride, (double)beta_a, (double)beta_b, w);
        out[2][q] = (float)w[2];
        out[3][q] = (float)w[3];
        out[6][q] = (float)w[6];
        out[7][q] = (float)w[7];
    }
}

}  // namespace vodhip
