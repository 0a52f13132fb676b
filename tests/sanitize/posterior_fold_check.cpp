// Stand-alone check of the host fold of per-shard posterior means (vod_amd/csrc/partition_fold.h, fold_posterior_mean) against a
// long-double weighted sum over random shard splits, with empty shards, the zero row of a query without a finite maximum, and
// non-finite rows behind empty shards.  Built with -fsanitize=address,undefined by tests/test_posterior_mean_cpu.py and run directly;
// prints "<n> folds checked, <e> errors".
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "partition_fold.h"

namespace {

long g_checked = 0, g_errors = 0;

void expect(bool ok, const char* what) {
    ++g_checked;
    if (!ok) {
        ++g_errors;
        std::printf("FAILED: %s\n", what);
    }
}

}  // namespace

int main() {
    const float inf = INFINITY;
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> score(-3000.0, 3000.0), rel(0.0, 12.0), pick(0.0, 1.0), val(-8.0, 8.0);
    for (int trial = 0; trial < 1000; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t nq = 1 + (int64_t)(rng() % 20);
        const int64_t dim = 1 + (int64_t)(rng() % 70);
        const float beta = trial % 3 == 0 ? 1.f : (trial % 3 == 1 ? 1.f / 64.f : 4.f);
        // shard g: [max | log_rel | mean rows] at g * nq (2 + dim), as the node index lays them out
        const size_t per = (size_t)nq * (size_t)(2 + dim);
        std::vector<float> parts((size_t)G * per);
        for (int g = 0; g < G; ++g)
            for (int64_t q = 0; q < nq; ++q) {
                const bool empty = pick(rng) < 0.25;
                parts[(size_t)g * per + q] = empty ? -inf : (float)std::floor(score(rng) / 100.0);
                parts[(size_t)g * per + nq + q] = empty ? -inf : (float)rel(rng);
                for (int64_t d = 0; d < dim; ++d)  // (an empty shard's row must not be read: poison it)
                    parts[(size_t)g * per + 2 * nq + q * dim + d] = empty ? NAN : (float)val(rng);
            }
        std::vector<float> m((size_t)nq), r((size_t)nq), mean((size_t)(nq * dim), 123.f);
        vodhip::fold_log_partition(parts.data(), parts.data() + nq, G, (int64_t)per, nq, beta, m.data(), r.data());
        vodhip::fold_posterior_mean(parts.data(), parts.data() + nq, parts.data() + 2 * nq, G, (int64_t)per, (int64_t)per, nq, dim, beta, m.data(),
                                    r.data(), mean.data());
        for (int64_t q = 0; q < nq; ++q) {
            if (m[q] == -inf) {
                bool zero = true;
                for (int64_t d = 0; d < dim; ++d) zero = zero && mean[q * dim + d] == 0.f;
                expect(zero, "all shards empty -> the zero row");
                continue;
            }
            long double total = 0.0L;
            std::vector<long double> w((size_t)G, 0.0L);
            for (int g = 0; g < G; ++g) {
                const float mg = parts[(size_t)g * per + q], lg = parts[(size_t)g * per + nq + q];
                if (mg != -inf) w[(size_t)g] = std::exp((long double)beta * ((long double)mg - m[q]) + lg);
                total += w[(size_t)g];
            }
            bool ok = true;
            for (int64_t d = 0; d < dim; ++d) {
                long double want = 0.0L, mag = 0.0L;
                for (int g = 0; g < G; ++g)
                    if (w[(size_t)g] > 0.0L) {
                        const long double v = parts[(size_t)g * per + 2 * nq + q * dim + d];
                        want += w[(size_t)g] / total * v;
                        mag += w[(size_t)g] / total * std::fabs(v);
                    }
                // the folded log_rel is a float32 (relative 2^-24 of up to ~16 -> 1e-6 in the weights), the result rounds once
                ok = ok && std::fabs((double)(mean[q * dim + d] - want)) <= 3e-6 * (double)mag + 1e-30;
            }
            expect(ok, "weighted mean of the shard means");
        }
    }
    {   // one shard: the row passes through within the float32 rounding of log_rel; a +inf maximum gives the zero row; nq == 0
        const float mg[1] = {5.f}, lg[1] = {3.25f}, row[3] = {1.f, -2.f, 0.5f};
        float m, r, out[3];
        vodhip::fold_log_partition(mg, lg, 1, 1, 1, 2.f, &m, &r);
        vodhip::fold_posterior_mean(mg, lg, row, 1, 1, 3, 1, 3, 2.f, &m, &r, out);
        expect(std::fabs(out[0] - 1.f) <= 1e-6f && std::fabs(out[1] + 2.f) <= 2e-6f && std::fabs(out[2] - 0.5f) <= 1e-6f, "one shard");
        const float mi[2] = {1.f, inf}, li[2] = {0.f, inf}, rows[2] = {7.f, NAN};
        float one = 9.f;
        vodhip::fold_log_partition(mi, li, 2, 1, 1, 1.f, &m, &r);
        vodhip::fold_posterior_mean(mi, li, rows, 2, 1, 1, 1, 1, 1.f, &m, &r, &one);
        expect(m == inf && one == 0.f, "+inf maximum -> the zero row");
        vodhip::fold_posterior_mean(mi, li, rows, 2, 1, 1, 0, 1, 1.f, nullptr, nullptr, nullptr);  // nq == 0 touches nothing
        vodhip::fold_posterior_mean(mi, li, rows, 2, 1, 1, 0, 0, 1.f, nullptr, nullptr, nullptr);
    }
    std::printf("%ld folds checked, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
