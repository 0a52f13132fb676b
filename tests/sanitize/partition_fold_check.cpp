// Stand-alone check of the host side of the log-partition call (vod_amd/csrc/partition_fold.h): the fold of per-shard (max, log_rel)
// pairs against a long-double log-sum-exp over random shard splits, the special values, and the argument checks.  Built with
// -fsanitize=address,undefined by tests/test_log_partition_cpu.py and run directly; prints "<n> folds checked, <e> errors".
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
    std::mt19937_64 rng(20261019);
    std::uniform_real_distribution<double> score(-3000.0, 3000.0), rel(0.0, 12.0), pick(0.0, 1.0);
    for (int trial = 0; trial < 2000; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t nq = 1 + (int64_t)(rng() % 40);
        const float beta = trial % 3 == 0 ? 1.f : (trial % 3 == 1 ? 1.f / 64.f : 4.f);
        // shard g's pair of query q at [g * 2 nq + q] and [g * 2 nq + nq + q], as the node index lays them out
        std::vector<float> parts((size_t)G * 2 * (size_t)nq);
        for (int g = 0; g < G; ++g)
            for (int64_t q = 0; q < nq; ++q) {
                const bool empty = pick(rng) < 0.2;
                parts[(size_t)g * 2 * nq + q] = empty ? -inf : (float)std::floor(score(rng));
                parts[(size_t)g * 2 * nq + nq + q] = empty ? -inf : (float)rel(rng);
            }
        std::vector<float> m((size_t)nq), r((size_t)nq);
        vodhip::fold_log_partition(parts.data(), parts.data() + nq, G, 2 * nq, nq, beta, m.data(), r.data());
        for (int64_t q = 0; q < nq; ++q) {
            float mx = -inf;
            for (int g = 0; g < G; ++g) mx = std::fmax(mx, parts[(size_t)g * 2 * nq + q]);
            if (mx == -inf) {
                expect(m[q] == -inf && r[q] == -inf, "all shards empty -> (-inf, -inf)");
                continue;
            }
            long double sum = 0.0L;
            for (int g = 0; g < G; ++g) {
                const float mg = parts[(size_t)g * 2 * nq + q], lg = parts[(size_t)g * 2 * nq + nq + q];
                if (mg != -inf) sum += std::exp((long double)beta * ((long double)mg - mx) + lg);
            }
            const double want = (double)std::log(sum);
            expect(m[q] == mx, "max of the shard maxima");
            expect(r[q] >= 0.f && std::fabs((double)r[q] - want) <= 1.2e-7 * std::fmax(1.0, std::fabs(want)), "log_rel within a float32 rounding");
        }
    }
    {   // one shard: the pair passes through unchanged (exp(log_rel) and back rounds within float32)
        const float mg[2] = {5.f, 0.f}, lg[2] = {3.25f, 0.f};
        float m, r;
        vodhip::fold_log_partition(mg, lg, 1, 1, 1, 2.f, &m, &r);
        expect(m == 5.f && std::fabs(r - 3.25f) <= 4e-7f, "one shard");
        const float mi[3] = {1.f, inf, -inf}, li[3] = {0.f, inf, -inf};
        vodhip::fold_log_partition(mi, li, 3, 1, 1, 1.f, &m, &r);
        expect(m == inf && r == inf, "+inf maximum -> (+inf, +inf)");
        vodhip::fold_log_partition(mi, li, 3, 1, 0, 1.f, nullptr, nullptr);  // nq == 0 touches nothing
    }
    {
        using vodhip::log_partition_args_error;
        float a = 0.f, b = 0.f;
        const int lab = 0;
        expect(log_partition_args_error(&a, 2, 1, 1.f, nullptr, 0, &a, &b) == nullptr, "valid arguments");
        expect(log_partition_args_error(nullptr, 2, 0, 1.f, nullptr, 0, nullptr, nullptr) == nullptr, "nq == 0 needs no pointers");
        expect(log_partition_args_error(nullptr, 2, 1, 1.f, nullptr, 0, &a, &b) != nullptr, "NULL queries");
        expect(log_partition_args_error(&a, 2, 1, 1.f, nullptr, 0, nullptr, &b) != nullptr, "NULL out_max");
        expect(log_partition_args_error(&a, 2, -1, 1.f, nullptr, 0, &a, &b) != nullptr, "nq < 0");
        expect(log_partition_args_error(&a, 3, 1, 1.f, nullptr, 0, &a, &b) != nullptr, "q_dtype 3");
        expect(log_partition_args_error(&a, -1, 1, 1.f, nullptr, 0, &a, &b) != nullptr, "q_dtype -1");
        for (float beta : {0.f, -1.f, inf, -inf, NAN}) expect(log_partition_args_error(&a, 2, 1, beta, nullptr, 0, &a, &b) != nullptr, "beta");
        expect(log_partition_args_error(&a, 2, 1, 1.f, &lab, 0, &a, &b) != nullptr, "n_per_query 0");
        expect(log_partition_args_error(&a, 2, 1, 1.f, &lab, 65, &a, &b) != nullptr, "n_per_query 65");
        expect(log_partition_args_error(&a, 2, 1, 1.f, &lab, 64, &a, &b) == nullptr, "n_per_query 64");
    }
    std::printf("%ld folds checked, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
