// Stand-alone check of the host side of the posterior-statistics call (vod_amd/csrc/stats_fold.h): the fold of per-shard
// (max, log_rel, mean_rel, var) words against long-double moments of the rows behind them, one shard against split shards, the special
// values, and the argument checks.  Built with -fsanitize=address,undefined by tests/test_posterior_stats_cpu.py and run directly;
// prints "<n> folds checked, <e> errors".
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "stats_fold.h"

namespace {

long g_checked = 0, g_errors = 0;

void expect(bool ok, const char* what) {
    ++g_checked;
    if (!ok) {
        ++g_errors;
        std::printf("FAILED: %s\n", what);
    }
}

bool close(double got, double want, double tol) { return std::fabs(got - want) <= tol * std::fmax(1.0, std::fabs(want)); }

// the four words of the rows `s` in double: what one shard that holds exactly these rows reports
void words_of(const std::vector<double>& s, double beta, double out[4]) {
    if (s.empty()) {
        out[0] = out[1] = -INFINITY;
        out[2] = out[3] = NAN;
        return;
    }
    long double m = s[0];
    for (double v : s) m = std::fmax(m, (long double)v);
    long double z = 0, a = 0, b = 0;
    for (double v : s) {
        const long double d = v - m, e = std::exp((long double)beta * d);
        z += e;
        a += e * d;
        b += e * d * d;
    }
    out[0] = (double)m;
    out[1] = (double)std::log(z);
    out[2] = (double)(a / z);
    out[3] = (double)(b / z - (a / z) * (a / z));
}

}  // namespace

int main() {
    const float inf = INFINITY;
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> pick(0.0, 1.0);
    // one shard holding all the rows against the same rows split over G shards (some of them empty), words kept in double: 1e-12
    for (int trial = 0; trial < 1500; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const double beta = trial % 3 == 0 ? 1.0 : (trial % 3 == 1 ? 1.0 / 64.0 : 4.0);
        std::uniform_real_distribution<double> score(-6.0 / beta, 6.0 / beta);
        std::vector<double> all;
        std::vector<double> wm((size_t)G), wr((size_t)G), wa((size_t)G), wv((size_t)G);
        bool any = false;
        for (int g = 0; g < G; ++g) {
            std::vector<double> rows;
            if (pick(rng) >= 0.25) {
                const int n = 1 + (int)(rng() % 30);
                for (int i = 0; i < n; ++i) rows.push_back(std::floor(score(rng) * 8.0) / 8.0);
            }
            any = any || !rows.empty();
            all.insert(all.end(), rows.begin(), rows.end());
            double w[4];
            words_of(rows, beta, w);
            wm[(size_t)g] = w[0], wr[(size_t)g] = w[1], wa[(size_t)g] = w[2], wv[(size_t)g] = w[3];
        }
        double one[4], want[4], split[4];
        words_of(all, beta, want);
        vodhip::fold_posterior_stats_query(wm.data(), wr.data(), wa.data(), wv.data(), G, 1, beta, split);
        if (!any) {
            expect(split[0] == -inf && split[1] == -inf && std::isnan(split[2]) && std::isnan(split[3]), "all shards empty -> (-inf, -inf, NaN, NaN)");
            continue;
        }
        vodhip::fold_posterior_stats_query(&want[0], &want[1], &want[2], &want[3], 1, 1, beta, one);
        const double scale = 1.0 / beta;  // (scores span 12 / beta)
        expect(split[0] == want[0] && one[0] == want[0], "max of the shard maxima");
        expect(close(split[1], one[1], 1e-12) && close(one[1], want[1], 1e-12), "log_rel: one shard == split shards");
        expect(close(split[2] / scale, one[2] / scale, 1e-12) && close(one[2] / scale, want[2] / scale, 1e-12), "mean_rel: one shard == split shards");
        expect(close(split[3] / (scale * scale), one[3] / (scale * scale), 1e-12) && close(one[3], want[3], 1e-12 * scale * scale) && split[3] >= 0.0,
               "var: one shard == split shards");
    }
    {   // the float entry point: layout [g * stride + q], outputs rounded once; empty shards are skipped, their NaN words never read
        const int G = 3;
        const int64_t nq = 2;
        const float nan = NAN;
        //                      shard 0      shard 1 (empty)   shard 2
        const float mg[G * 2] = {4.f, 1.f,   -inf, -inf,       2.f, 1.f};
        const float lg[G * 2] = {0.f, 0.f,   -inf, -inf,       0.f, 0.f};
        const float ag[G * 2] = {0.f, 0.f,   nan, nan,         0.f, 0.f};
        const float vg[G * 2] = {0.f, 0.f,   nan, nan,         0.f, 0.f};
        float m[2], r[2], a[2], v[2];
        vodhip::fold_posterior_stats(mg, lg, ag, vg, G, nq, nq, 1.f, m, r, a, v);
        // query 0: rows {4, 2}: p = (1, e^-2) / (1 + e^-2); query 1: rows {1, 1}
        const double p2 = std::exp(-2.0) / (1.0 + std::exp(-2.0));
        expect(m[0] == 4.f && close(r[0], std::log1p(std::exp(-2.0)), 2e-7), "two one-row shards: the pair");
        expect(close(a[0], -2.0 * p2, 2e-7) && close(v[0], 4.0 * p2 * (1.0 - p2), 2e-7), "two one-row shards: mean_rel and var");
        expect(m[1] == 1.f && close(r[1], std::log(2.0), 2e-7) && a[1] == 0.f && v[1] == 0.f, "equal rows over two shards: mean_rel == 0, var == 0");
        float m1[2], r1[2];
        vodhip::fold_log_partition(mg, lg, G, nq, nq, 1.f, m1, r1);
        expect(m1[0] == m[0] && r1[0] == r[0] && m1[1] == m[1] && r1[1] == r[1], "the pair is fold_log_partition's, bit for bit");

        const float mi[3] = {1.f, inf, -inf}, li[3] = {0.f, inf, -inf}, ai[3] = {0.f, nan, nan}, vi[3] = {0.f, nan, nan};
        vodhip::fold_posterior_stats(mi, li, ai, vi, 3, 1, 1, 1.f, m, r, a, v);
        expect(m[0] == inf && r[0] == inf && std::isnan(a[0]) && std::isnan(v[0]), "+inf shard -> (+inf, +inf, NaN, NaN)");
        const float me[2] = {-inf, -inf}, ne[2] = {nan, nan};
        vodhip::fold_posterior_stats(me, me, ne, ne, 2, 1, 1, 1.f, m, r, a, v);
        expect(m[0] == -inf && r[0] == -inf && std::isnan(a[0]) && std::isnan(v[0]), "all shards empty -> (-inf, -inf, NaN, NaN)");
        vodhip::fold_posterior_stats(mi, li, ai, vi, 3, 1, 0, 1.f, nullptr, nullptr, nullptr, nullptr);  // nq == 0 touches nothing
    }
    {
        using vodhip::posterior_stats_args_error;
        float a = 0.f;
        const int lab = 0;
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, nullptr, 0, &a, &a, &a, &a) == nullptr, "valid arguments");
        expect(posterior_stats_args_error(nullptr, 2, 0, 1.f, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == nullptr, "nq == 0 needs no pointers");
        expect(posterior_stats_args_error(nullptr, 2, 1, 1.f, nullptr, 0, &a, &a, &a, &a) != nullptr, "NULL queries");
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, nullptr, 0, nullptr, &a, &a, &a) != nullptr, "NULL out_max");
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, nullptr, 0, &a, nullptr, &a, &a) != nullptr, "NULL out_log_rel");
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, nullptr, 0, &a, &a, nullptr, &a) != nullptr, "NULL out_mean_rel");
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, nullptr, 0, &a, &a, &a, nullptr) != nullptr, "NULL out_var");
        expect(posterior_stats_args_error(&a, 2, -1, 1.f, nullptr, 0, &a, &a, &a, &a) != nullptr, "nq < 0");
        expect(posterior_stats_args_error(&a, 3, 1, 1.f, nullptr, 0, &a, &a, &a, &a) != nullptr, "q_dtype 3");
        for (float beta : {0.f, -1.f, inf, -inf, NAN}) expect(posterior_stats_args_error(&a, 2, 1, beta, nullptr, 0, &a, &a, &a, &a) != nullptr, "beta");
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, &lab, 0, &a, &a, &a, &a) != nullptr, "n_per_query 0");
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, &lab, 65, &a, &a, &a, &a) != nullptr, "n_per_query 65");
        expect(posterior_stats_args_error(&a, 2, 1, 1.f, &lab, 64, &a, &a, &a, &a) == nullptr, "n_per_query 64");
    }
    std::printf("%ld folds checked, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
