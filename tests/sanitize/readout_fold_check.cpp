// Stand-alone check of the host-only pieces of the posterior read-out (vod_amd/csrc/readout_fold.h): the argument checks, the split
// of a node index's value table by shard row ranges (with an empty last shard) and the fold of per-shard results (with empty shards
// and a +inf maximum) against a long-double weighted sum, at n_cols 1 and 256 and random widths between.  Built with
// -fsanitize=address,undefined by tests/test_posterior_expectation_cpu.py and run directly; prints "<n> checks, <e> errors".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "readout_fold.h"

namespace {

long g_checked = 0, g_errors = 0;

void expect(bool ok, const char* what) {
    ++g_checked;
    if (!ok) {
        ++g_errors;
        std::printf("FAILED: %s\n", what);
    }
}

bool says(const char* msg, const char* text) { return msg && std::strstr(msg, text); }

}  // namespace

int main() {
    const float inf = INFINITY;
    using namespace vodhip;

    // ---- argument refusals
    expect(row_values_args_error(10, 1, 2, 0, 10) == nullptr, "a one-column float32 host table");
    expect(row_values_args_error(10, 256, 0, 1, 10) == nullptr, "a 256-column fp16 device table");
    expect(row_values_args_error(0, 3, 1, 0, 0) == nullptr, "a table of no rows for an empty index");
    expect(says(row_values_args_error(10, 0, 2, 0, 10), "n_cols"), "n_cols 0");
    expect(says(row_values_args_error(10, 257, 2, 0, 10), "n_cols"), "n_cols 257");
    expect(says(row_values_args_error(10, -1, 2, 0, 10), "n_cols"), "n_cols -1");
    expect(says(row_values_args_error(9, 4, 2, 0, 10), "n_rows"), "a short table");
    expect(says(row_values_args_error(11, 4, 2, 0, 10), "n_rows"), "a long table");
    expect(says(row_values_args_error(10, 4, 3, 0, 10), "src_dtype"), "src_dtype 3");
    expect(says(row_values_args_error(10, 4, -1, 0, 10), "src_dtype"), "src_dtype -1");
    expect(says(row_values_args_error(10, 4, 2, 2, 10), "location"), "location 2");
    expect(readout_c_pad(1) == 64 && readout_c_pad(64) == 64 && readout_c_pad(65) == 128 && readout_c_pad(256) == 256, "c_pad");
    {
        int a = 0;
        const void* p = &a;
        expect(posterior_expectation_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p) == nullptr, "a good call");
        expect(posterior_expectation_args_error(nullptr, 2, 0, 1.f, nullptr, 0, nullptr, nullptr, nullptr) == nullptr, "nq == 0 needs nothing");
        expect(says(posterior_expectation_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, nullptr), "pointers"), "NULL out_values");
        expect(says(posterior_expectation_args_error(nullptr, 2, 5, 1.f, nullptr, 0, p, p, p), "pointers"), "NULL queries");
        expect(says(posterior_expectation_args_error(p, 2, -1, 1.f, nullptr, 0, p, p, p), "pointers"), "nq < 0");
        expect(says(posterior_expectation_args_error(p, 3, 5, 1.f, nullptr, 0, p, p, p), "q_dtype"), "q_dtype 3");
        expect(says(posterior_expectation_args_error(p, 2, 5, 0.f, nullptr, 0, p, p, p), "beta"), "beta 0");
        expect(says(posterior_expectation_args_error(p, 2, 5, NAN, nullptr, 0, p, p, p), "beta"), "beta NaN");
        expect(says(posterior_expectation_args_error(p, 2, 5, 1.f, p, 65, p, p, p), "n_per_query"), "n_per_query 65");
    }

    // ---- the shard split: the ranges tile [0, n_rows) in order; shards past the end are empty
    for (int64_t n_rows : {0ll, 1ll, 7ll, 1000ll, 1001ll, 2999ll, 3000ll})
        for (int64_t rps : {1ll, 334ll, 1000ll, 1500ll, 4000ll})
            for (int G : {1, 2, 3, 8}) {
                if ((int64_t)G * rps < n_rows) continue;  // (the capacity holds the rows)
                int64_t next = 0;
                bool ok = true;
                for (int g = 0; g < G; ++g) {
                    int64_t lo = -1, hi = -1;
                    readout_shard_rows(n_rows, rps, g, &lo, &hi);
                    ok = ok && lo == next && hi >= lo && hi - lo <= rps && hi <= n_rows;
                    next = hi;
                }
                expect(ok && next == n_rows, "the shard ranges tile the table");
            }
    {   // 3 shards of 1000 rows, 2000 rows: the last shard is empty; the split hands every shard its own rows of a 256-column table
        const int64_t n_rows = 2000, n_cols = 256;
        std::vector<float> table((size_t)(n_rows * n_cols));
        for (size_t i = 0; i < table.size(); ++i) table[i] = (float)(i % 1021);
        double sum = 0.0, want = 0.0;
        for (float v : table) want += v;
        for (int g = 0; g < 3; ++g) {
            int64_t lo, hi;
            readout_shard_rows(n_rows, 1000, g, &lo, &hi);
            expect(g < 2 ? (lo == 1000 * g && hi == lo + 1000) : (lo == 2000 && hi == 2000), "an empty last shard");
            const float* src = table.data() + lo * n_cols;
            for (int64_t i = 0; i < (hi - lo) * n_cols; ++i) sum += src[i];  // (ASan: nothing past the table is read)
        }
        expect(sum == want, "every row lands in exactly one shard");
    }

    // ---- the fold against a long-double weighted sum
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> score(-3000.0, 3000.0), rel(0.0, 12.0), pick(0.0, 1.0), val(-8.0, 8.0);
    for (int trial = 0; trial < 400; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t nq = 1 + (int64_t)(rng() % 12);
        const int64_t n_cols = trial % 5 == 0 ? 1 : (trial % 5 == 1 ? 256 : 1 + (int64_t)(rng() % 256));
        const float beta = trial % 3 == 0 ? 1.f : (trial % 3 == 1 ? 1.f / 64.f : 4.f);
        const size_t per = (size_t)nq * (size_t)(2 + n_cols);
        std::vector<float> parts((size_t)G * per);
        for (int g = 0; g < G; ++g)
            for (int64_t q = 0; q < nq; ++q) {
                const bool empty = g == G - 1 ? trial % 2 == 0 : pick(rng) < 0.25;  // (an empty LAST shard every other trial)
                const bool plus = !empty && q == 0 && trial % 7 == 0 && g == 0;     // (a +inf maximum now and then)
                parts[(size_t)g * per + q] = empty ? -inf : (plus ? inf : (float)std::floor(score(rng) / 100.0));
                parts[(size_t)g * per + nq + q] = empty ? -inf : (plus ? inf : (float)rel(rng));
                for (int64_t c = 0; c < n_cols; ++c)  // (an empty shard's row must not be read: poison it)
                    parts[(size_t)g * per + 2 * nq + q * n_cols + c] = empty ? NAN : (float)val(rng);
            }
        std::vector<float> m((size_t)nq), r((size_t)nq), out((size_t)(nq * n_cols), 123.f);
        fold_posterior_expectation(parts.data(), G, nq, n_cols, beta, m.data(), r.data(), out.data());
        for (int64_t q = 0; q < nq; ++q) {
            if (m[q] == -inf || m[q] == inf) {
                bool zero = r[q] == m[q];
                for (int64_t c = 0; c < n_cols; ++c) zero = zero && out[q * n_cols + c] == 0.f;
                expect(zero, "no finite maximum -> the zero row");
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
            for (int64_t c = 0; c < n_cols; ++c) {
                long double want = 0.0L, mag = 0.0L;
                for (int g = 0; g < G; ++g)
                    if (w[(size_t)g] > 0.0L) {
                        const long double v = parts[(size_t)g * per + 2 * nq + q * n_cols + c];
                        want += w[(size_t)g] / total * v;
                        mag += w[(size_t)g] / total * std::fabs(v);
                    }
                // the folded log_rel is a float32 (relative 2^-24 of up to ~16 -> 1e-6 in the weights), the result rounds once
                ok = ok && std::fabs((double)(out[q * n_cols + c] - want)) <= 3e-6 * (double)mag + 1e-30;
            }
            expect(ok, "weighted sum of the shard rows");
        }
    }
    {
        float none = 0.f;
        fold_posterior_expectation(&none, 3, 0, 5, 1.f, &none, &none, &none);  // nq == 0 touches nothing
        expect(none == 0.f, "nq == 0 writes nothing");
    }
    std::printf("%ld checks, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
