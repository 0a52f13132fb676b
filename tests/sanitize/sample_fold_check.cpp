// Stand-alone check of the host side of sample_posterior (vod_amd/csrc/sample_fold.h): the merge of per-shard sample lists against the
// k + 1 best of the whole store over random shard splits - empty shards, fewer than k + 1 rows, tied keys, exactly sized buffers (the
// sanitizer sees any access past them) - the weights against long-double arithmetic, the pads of a query without a finite log Z, and the
// argument checks.  Built with -fsanitize=address,undefined by tests/test_sample_posterior_cpu.py and run directly; prints
// "<n> folds checked, <e> errors".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "sample_fold.h"

namespace {

long g_checked = 0, g_errors = 0;

void expect(bool ok, const char* what) {
    ++g_checked;
    if (!ok) {
        ++g_errors;
        std::printf("FAILED: %s\n", what);
    }
}

struct Row {
    float key;
    int64_t id;
    float score;
};

bool better(const Row& a, const Row& b) { return a.key != b.key ? a.key > b.key : a.id < b.id; }

}  // namespace

int main() {
    const float inf = INFINITY;
    std::mt19937_64 rng(20261021);
    std::uniform_real_distribution<double> val(-20.0, 20.0), pick(0.0, 1.0);
    const int ks[] = {1, 2, 4, 32, 255};
    for (int trial = 0; trial < 600; ++trial) {
        const int G = 1 + (int)(rng() % 5);
        const int k = ks[trial % 5];
        const int64_t nq = 1 + (int64_t)(rng() % 6);
        const int64_t per = (int64_t)(rng() % (trial % 7 == 0 ? 3 : 2 * k + 40));  // rows per shard (shard g: ids [g per, g per + per))
        const float beta = trial % 3 == 0 ? 1.f : (trial % 3 == 1 ? 1.f / 8.f : 2.f);
        const bool ties = trial % 4 == 1;
        const size_t krows = (size_t)nq * (size_t)(k + 1), rows = (size_t)nq * (size_t)k;
        std::vector<float> keys_g((size_t)G * krows, -inf), scores_g((size_t)G * rows, -inf);
        std::vector<int64_t> ids_g((size_t)G * rows, -1);
        std::vector<float> m((size_t)nq), lr((size_t)nq);
        std::vector<std::vector<Row>> all((size_t)nq);
        for (int64_t q = 0; q < nq; ++q) {
            m[(size_t)q] = (float)std::floor(val(rng));
            lr[(size_t)q] = (float)(std::fabs(val(rng)) / 4.0);
            if (trial % 11 == 3 && q == 0) m[0] = lr[0] = pick(rng) < 0.5 ? inf : -inf;
            for (int g = 0; g < G; ++g) {
                std::vector<Row> mine;
                const bool empty = pick(rng) < 0.2;
                for (int64_t r = 0; r < (empty ? 0 : per); ++r) {
                    const float key = ties ? (float)std::floor(val(rng) / 4.0) : (float)val(rng);
                    mine.push_back(Row{key, (int64_t)g * per + r, (float)val(rng)});
                }
                all[(size_t)q].insert(all[(size_t)q].end(), mine.begin(), mine.end());
                std::sort(mine.begin(), mine.end(), better);
                for (size_t p = 0; p < mine.size() && p <= (size_t)k; ++p) {
                    keys_g[(size_t)g * krows + (size_t)q * (size_t)(k + 1) + p] = mine[p].key;
                    if (p < (size_t)k) {
                        ids_g[(size_t)g * rows + (size_t)q * (size_t)k + p] = mine[p].id;
                        scores_g[(size_t)g * rows + (size_t)q * (size_t)k + p] = mine[p].score;
                    }
                }
            }
            std::sort(all[(size_t)q].begin(), all[(size_t)q].end(), better);
        }
        std::vector<int64_t> ids(rows, 77);
        std::vector<float> sc(rows, 77.f), lp(rows, 77.f), lw(rows, 77.f), keys(krows, 77.f);
        vodhip::fold_sample_posterior(keys_g.data(), ids_g.data(), scores_g.data(), G, (int64_t)krows, (int64_t)rows, (int64_t)rows, nq, k, beta, m.data(),
                                      lr.data(), ids.data(), sc.data(), lp.data(), lw.data(), keys.data());
        for (int64_t q = 0; q < nq; ++q) {
            const std::vector<Row>& want = all[(size_t)q];
            const bool live = std::isfinite(m[(size_t)q]) && std::isfinite(lr[(size_t)q]);
            const size_t n = live ? want.size() : 0;
            bool ok = true, wok = true;
            const float key_tau = n > (size_t)k ? want[(size_t)k].key : -inf;
            for (size_t p = 0; p <= (size_t)k; ++p) ok = ok && keys[(size_t)q * (size_t)(k + 1) + p] == (p < n ? want[p].key : -inf);
            for (size_t p = 0; p < (size_t)k; ++p) {
                const size_t at = (size_t)q * (size_t)k + p;
                if (p >= n) {
                    ok = ok && ids[at] == -1 && sc[at] == -inf && lp[at] == -inf && lw[at] == -inf;
                    continue;
                }
                ok = ok && ids[at] == want[p].id && sc[at] == want[p].score;
                const long double b = beta, a = b * ((long double)want[p].score - m[(size_t)q]) - lr[(size_t)q];
                long double w = a;
                if (key_tau != -inf) {
                    const long double t = ((long double)key_tau - b * m[(size_t)q]) - lr[(size_t)q];
                    w = a - std::log(-std::expm1(-std::exp(a - t)));
                }
                wok = wok && std::fabs((double)(lp[at] - a)) <= 1e-6 * (1.0 + std::fabs((double)a));
                wok = wok && std::fabs((double)(lw[at] - w)) <= 1e-6 * (1.0 + std::fabs((double)w));
            }
            expect(ok, "the k + 1 best of the union, pads behind them");
            expect(wok, "log_p and log_weight against long double");
        }
    }
    {   // the weights: no threshold -> the probability itself; a far threshold -> log_tau; nq == 0 touches nothing
        float lp, lw;
        vodhip::sample_weight(2.f, 3.f, -inf, 5.f, 1.5f, &lp, &lw);
        expect(lp == -5.5f && lw == -5.5f, "log_tau = -inf: log_weight = log_p");
        vodhip::sample_weight(1.f, -30.f, 1.f, 0.f, 0.f, &lp, &lw);  // log_p = -30, log_tau = 1: weight = p / (1 - exp(-p / tau)) ~ tau
        expect(lp == -30.f && std::fabs(lw - 1.f) < 1e-6f, "a rare row weighs tau");
        vodhip::sample_weight(1.f, 0.f, -40.f, 0.f, 0.f, &lp, &lw);  // log_p = 0 far above log_tau: always drawn, weight p
        expect(lp == 0.f && lw == 0.f, "a sure row weighs its probability");
        vodhip::fold_sample_posterior(nullptr, nullptr, nullptr, 3, 0, 0, 0, 0, 4, 1.f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    }
    {   // the argument checks
        int x = 0;
        const void* p = &x;
        expect(vodhip::sample_posterior_args_error(1, 1, 0, 0, p, p, p, p, p) == nullptr, "k = 1");
        expect(vodhip::sample_posterior_args_error(1, 255, 0, 0, p, p, p, p, p) == nullptr, "k = 255");
        expect(vodhip::sample_posterior_args_error(1, 0, 0, 0, p, p, p, p, p) != nullptr, "k = 0");
        expect(vodhip::sample_posterior_args_error(1, 256, 0, 0, p, p, p, p, p) != nullptr, "k = 256");
        expect(vodhip::sample_posterior_args_error(1, 4, -1, 0, p, p, p, p, p) != nullptr, "query_offset < 0");
        expect(vodhip::sample_posterior_args_error(1, 4, (1ll << 32) - 1, 0, p, p, p, p, p) == nullptr, "the last stream index");
        expect(vodhip::sample_posterior_args_error(2, 4, (1ll << 32) - 1, 0, p, p, p, p, p) != nullptr, "query_offset + nq > 2^32");
        expect(vodhip::sample_posterior_args_error(1, 4, 0, -1, p, p, p, p, p) != nullptr, "id_base < 0");
        expect(vodhip::sample_posterior_args_error(1, 4, 0, 0, p, p, nullptr, p, p) != nullptr, "a NULL output");
        expect(vodhip::sample_posterior_args_error(0, 4, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == nullptr, "nq == 0 needs no buffer");
    }
    std::printf("%ld folds checked, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
