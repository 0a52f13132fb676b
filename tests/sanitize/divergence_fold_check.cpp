// Stand-alone check of the host side of the posterior-divergence call (vod_amd/csrc/divergence_fold.h): the fold of per-shard words
// against long-double moments of the rows behind them - one shard against split shards (1, 2, 3 and 8 of them, some empty), folds of
// folds, a shard with -inf scores on one side, the special values, and the argument checks.  Built with -fsanitize=address,undefined
// by tests/test_posterior_divergence_cpu.py and run directly; prints "<n> folds checked, <e> errors".
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "divergence_fold.h"

namespace {

long g_checked = 0, g_errors = 0;

void expect(bool ok, const char* what) {
    ++g_checked;
    if (!ok) {
        ++g_errors;
        std::printf("FAILED: %s\n", what);
    }
}

bool close(double got, double want, double tol) {
    if (std::isinf(want) || std::isnan(want)) return (std::isnan(want) && std::isnan(got)) || got == want;
    return std::fabs(got - want) <= tol * std::fmax(1.0, std::fabs(want));
}

struct Row { double a, b; };

// the eight words of the rows in double: what one shard that holds exactly these rows reports
void words_of(const std::vector<Row>& rows, double beta_a, double beta_b, double out[8]) {
    long double m[2] = {-INFINITY, -INFINITY};
    for (const Row& r : rows) {
        m[0] = std::fmax(m[0], (long double)r.a);
        m[1] = std::fmax(m[1], (long double)r.b);
    }
    const double beta[2] = {beta_a, beta_b};
    for (int s = 0; s < 2; ++s) {
        out[4 * s] = (double)m[s];
        if (std::isinf(m[s])) {
            out[4 * s + 1] = (double)m[s];
            out[4 * s + 2] = NAN;
        }
        out[4 * s + 3] = NAN;
    }
    for (int s = 0; s < 2; ++s) {
        if (std::isinf(m[s])) continue;
        long double z = 0, a = 0, c = 0;
        for (const Row& r : rows) {
            const long double own = s == 0 ? r.a : r.b, other = s == 0 ? r.b : r.a;
            if (own == -INFINITY) continue;
            const long double e = std::exp((long double)beta[s] * (own - m[s]));
            z += e;
            a += e * (own - m[s]);
            if (!std::isinf(m[1 - s])) c += other == -INFINITY ? -INFINITY : e * (other - m[1 - s]);
        }
        out[4 * s + 1] = (double)std::log(z);
        out[4 * s + 2] = (double)(a / z);
        if (!std::isinf(m[1 - s])) out[4 * s + 3] = (double)(c / z);
    }
}

void fold(const std::vector<double> (&w)[8], int first, int count, double beta_a, double beta_b, double out[8]) {
    const double* p[8];
    for (int k = 0; k < 8; ++k) p[k] = w[k].data() + first;
    vodhip::fold_posterior_divergence_pair<double>(p, count, 1, beta_a, beta_b, out);
}

}  // namespace

int main() {
    const float inf = INFINITY;
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> pick(0.0, 1.0);
    const int shard_counts[4] = {1, 2, 3, 8};
    for (int trial = 0; trial < 1600; ++trial) {
        const int G = shard_counts[trial % 4];
        const double beta_a = trial % 3 == 0 ? 1.0 : (trial % 3 == 1 ? 1.0 / 64.0 : 4.0);
        const double beta_b = trial % 5 == 0 ? beta_a : (trial % 5 < 3 ? 1.0 : 1.0 / 64.0);
        std::uniform_real_distribution<double> sa(-6.0 / beta_a, 6.0 / beta_a), sb(-6.0 / beta_b, 6.0 / beta_b);
        const bool minus_inf = trial % 7 == 3;  // some rows score -inf on side b: under mass of side a
        std::vector<Row> all;
        std::vector<double> w[8];
        for (int k = 0; k < 8; ++k) w[k].resize((size_t)G);
        bool any = false, any_minus_inf = false;
        for (int g = 0; g < G; ++g) {
            std::vector<Row> rows;
            if (G == 1 || pick(rng) >= 0.25) {
                const int n = 1 + (int)(rng() % 30);
                const bool dead_b = minus_inf && g == 0;  // shard 0: side b has no finite score at all
                for (int i = 0; i < n; ++i)
                    rows.push_back({std::floor(sa(rng) * 8.0) / 8.0, dead_b || (minus_inf && i % 4 == 1) ? -INFINITY : std::floor(sb(rng) * 8.0) / 8.0});
            }
            any = any || !rows.empty();
            for (const Row& r : rows) any_minus_inf = any_minus_inf || r.b == -INFINITY;
            all.insert(all.end(), rows.begin(), rows.end());
            double ww[8];
            words_of(rows, beta_a, beta_b, ww);
            for (int k = 0; k < 8; ++k) w[k][(size_t)g] = ww[k];
        }
        double want[8], split[8], one[8];
        words_of(all, beta_a, beta_b, want);
        fold(w, 0, G, beta_a, beta_b, split);
        if (!any) {
            expect(split[0] == -inf && split[1] == -inf && std::isnan(split[2]) && std::isnan(split[3]) && split[4] == -inf && split[5] == -inf &&
                       std::isnan(split[6]) && std::isnan(split[7]), "all shards empty -> (-inf, -inf, NaN, NaN) twice");
            continue;
        }
        {   // a one-shard fold of the words of all the rows
            std::vector<double> w1[8];
            for (int k = 0; k < 8; ++k) w1[k].assign(1, want[k]);
            fold(w1, 0, 1, beta_a, beta_b, one);
        }
        const double scale[8] = {1, 1, 1.0 / beta_a, 1.0 / beta_b, 1, 1, 1.0 / beta_b, 1.0 / beta_a};
        bool ok = split[0] == want[0] && split[4] == want[4] && one[0] == want[0] && one[4] == want[4];
        for (int k : {1, 2, 3, 5, 6, 7})
            ok = ok && close(split[k] / scale[k], want[k] / scale[k], 1e-11) && close(one[k] / scale[k], want[k] / scale[k], 1e-11);
        expect(ok, "split shards == one shard == the rows' own words");
        if (std::isfinite(want[0]) && std::isfinite(want[4])) {
            expect(split[2] <= 0 && split[3] <= 0 && split[6] <= 0 && split[7] <= 0, "every relative word <= 0");
            if (any_minus_inf) expect(split[3] == -inf && !std::isnan(split[7]), "mass of side a on rows side b scores -inf: cross_rel_ab == -inf, no NaN");
        }
        if (G >= 3) {  // a fold of folds: shards [0, h) and [h, G) folded apart, then their two results folded
            const int h = 1 + (int)(rng() % (G - 1));
            double left[8], right[8], both[8];
            fold(w, 0, h, beta_a, beta_b, left);
            fold(w, h, G - h, beta_a, beta_b, right);
            std::vector<double> w2[8];
            for (int k = 0; k < 8; ++k) w2[k] = {left[k], right[k]};
            fold(w2, 0, 2, beta_a, beta_b, both);
            bool same = both[0] == split[0] && both[4] == split[4];
            for (int k : {1, 2, 3, 5, 6, 7}) same = same && close(both[k] / scale[k], split[k] / scale[k], 1e-11);
            expect(same, "a fold of folds == the fold of all the shards");
        }
    }
    {   // the float entry point: layout [(g * 8 + k) * nq + q], outputs rounded once; empty shards are skipped, their NaN words never read
        const int G = 3;
        const int64_t nq = 2;
        const float nan = NAN;
        // pair 0: shard 0 holds the row (a 4, b 1), shard 2 the row (a 2, b 3); pair 1: shard 0 (1, 1), shard 2 (1, -inf)
        const float parts[G * 8 * 2] = {
            4.f, 1.f,  0.f, 0.f,  0.f, 0.f,  0.f, 0.f,   1.f, 1.f,  0.f, 0.f,  0.f, 0.f,  0.f, 0.f,          // shard 0
            -inf, -inf,  -inf, -inf,  nan, nan,  nan, nan,   -inf, -inf,  -inf, -inf,  nan, nan,  nan, nan,  // shard 1: empty
            2.f, 1.f,  0.f, 0.f,  0.f, 0.f,  0.f, nan,   3.f, -inf,  0.f, -inf,  0.f, nan,  0.f, nan};       // shard 2
        float o[8][2];
        float* outs[8];
        for (int k = 0; k < 8; ++k) outs[k] = o[k];
        vodhip::fold_posterior_divergence(parts, G, nq, 1.f, 1.f, outs);
        const double pa = std::exp(-2.0) / (1.0 + std::exp(-2.0));  // p of the row (2, 3) under a; under b the row (4, 1) has the same mass
        expect(o[0][0] == 4.f && o[4][0] == 3.f && close(o[1][0], std::log1p(std::exp(-2.0)), 2e-7) && close(o[5][0], std::log1p(std::exp(-2.0)), 2e-7),
               "two one-row shards: the pairs");
        expect(close(o[2][0], -2.0 * pa, 2e-7) && close(o[6][0], -2.0 * pa, 2e-7), "two one-row shards: mean_rel");
        expect(close(o[3][0], -2.0 * (1.0 - pa), 2e-7) && close(o[7][0], -2.0 * (1.0 - pa), 2e-7), "two one-row shards: the cross words");
        expect(o[0][1] == 1.f && close(o[1][1], std::log(2.0), 2e-7) && o[2][1] == 0.f && o[3][1] == -inf, "side a has mass in a shard where b is dead: -inf");
        expect(o[4][1] == 1.f && o[5][1] == 0.f && o[6][1] == 0.f && o[7][1] == 0.f, "side b's dead shard carries no weight");
        float m1[2], r1[2];
        vodhip::fold_log_partition(parts, parts + nq, G, 8 * nq, nq, 1.f, m1, r1);
        expect(m1[0] == o[0][0] && r1[0] == o[1][0] && m1[1] == o[0][1] && r1[1] == o[1][1], "each side's pair is fold_log_partition's, bit for bit");

        // a +inf score on side b of one shard: side b (+inf, +inf, NaN), both cross words NaN, side a's three words intact
        const float pi[2 * 8] = {1.f, 0.f, 0.f, 0.f, 2.f, 0.f, 0.f, 0.f,   3.f, 0.f, 0.f, nan, inf, inf, nan, nan};
        vodhip::fold_posterior_divergence(pi, 2, 1, 1.f, 1.f, outs);
        expect(o[0][0] == 3.f && close(o[1][0], std::log1p(std::exp(-2.0)), 2e-7) && close(o[2][0], -2.0 * pa, 2e-7), "+inf on side b: side a intact");
        expect(o[4][0] == inf && o[5][0] == inf && std::isnan(o[6][0]) && std::isnan(o[3][0]) && std::isnan(o[7][0]), "+inf on side b: NaN words");
        vodhip::fold_posterior_divergence(pi, 2, 0, 1.f, 1.f, outs);  // nq == 0 touches nothing
    }
    {
        using vodhip::posterior_divergence_args_error;
        float a = 0.f;
        const int lab = 0;
        const void* good[8] = {&a, &a, &a, &a, &a, &a, &a, &a};
        const void* none[8] = {};
        expect(posterior_divergence_args_error(&a, &a, 2, 1, 1.f, 2.f, nullptr, 0, good) == nullptr, "valid arguments");
        expect(posterior_divergence_args_error(nullptr, nullptr, 2, 0, 1.f, 1.f, nullptr, 0, none) == nullptr, "nq == 0 needs no pointers");
        expect(posterior_divergence_args_error(nullptr, &a, 2, 1, 1.f, 1.f, nullptr, 0, good) != nullptr, "NULL queries_a");
        expect(posterior_divergence_args_error(&a, nullptr, 2, 1, 1.f, 1.f, nullptr, 0, good) != nullptr, "NULL queries_b");
        for (int k = 0; k < 8; ++k) {
            const void* bad[8] = {&a, &a, &a, &a, &a, &a, &a, &a};
            bad[k] = nullptr;
            expect(posterior_divergence_args_error(&a, &a, 2, 1, 1.f, 1.f, nullptr, 0, bad) != nullptr, "a NULL output");
        }
        expect(posterior_divergence_args_error(&a, &a, 2, -1, 1.f, 1.f, nullptr, 0, good) != nullptr, "nq < 0");
        expect(posterior_divergence_args_error(&a, &a, 2, (1ll << 19) + 1, 1.f, 1.f, nullptr, 0, good) != nullptr, "nq > 2^19");
        expect(posterior_divergence_args_error(&a, &a, 2, 1ll << 19, 1.f, 1.f, nullptr, 0, good) == nullptr, "nq == 2^19");
        expect(posterior_divergence_args_error(&a, &a, 3, 1, 1.f, 1.f, nullptr, 0, good) != nullptr, "q_dtype 3");
        for (float beta : {0.f, -1.f, inf, -inf, NAN}) {
            expect(posterior_divergence_args_error(&a, &a, 2, 1, beta, 1.f, nullptr, 0, good) != nullptr, "beta_a");
            expect(posterior_divergence_args_error(&a, &a, 2, 1, 1.f, beta, nullptr, 0, good) != nullptr, "beta_b");
        }
        expect(posterior_divergence_args_error(&a, &a, 2, 1, 1.f, 1.f, &lab, 0, good) != nullptr, "n_per_query 0");
        expect(posterior_divergence_args_error(&a, &a, 2, 1, 1.f, 1.f, &lab, 65, good) != nullptr, "n_per_query 65");
        expect(posterior_divergence_args_error(&a, &a, 2, 1, 1.f, 1.f, &lab, 64, good) == nullptr, "n_per_query 64");
    }
    std::printf("%ld folds checked, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
