// Stand-alone check of the host-only pieces of the read-out's gradient (vod_amd/csrc/readout_grad_fold.h): the argument checks and
// the fold of per-shard results - a plain sum in increasing shard order, in double - against a long-double sum, at dim 1, 768 and
// random widths between, with exactly sized buffers (ASan: nothing past them is touched).  Built with -fsanitize=address,undefined by
// tests/test_expected_values_cpu.py and run directly; prints "<n> checks, <e> errors".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "readout_grad_fold.h"

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
    using namespace vodhip;

    // ---- argument refusals: H2e's, then the NULL inputs
    {
        int a = 0;
        const void* p = &a;
        expect(posterior_expectation_backward_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p, p, p) == nullptr, "a good call");
        expect(posterior_expectation_backward_args_error(p, 0, 5, 0.25f, p, 64, p, p, p, p, p) == nullptr, "a good call with labels");
        expect(posterior_expectation_backward_args_error(nullptr, 2, 0, 1.f, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == nullptr,
               "nq == 0 needs nothing");
        expect(says(posterior_expectation_backward_args_error(nullptr, 2, 5, 1.f, nullptr, 0, p, p, p, p, p), "pointers"), "NULL queries");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 1.f, nullptr, 0, nullptr, p, p, p, p), "pointers"), "NULL max_score");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 1.f, nullptr, 0, p, nullptr, p, p, p), "pointers"), "NULL log_rel");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, nullptr, p, p), "values is NULL"), "NULL values");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p, nullptr, p), "grad_values is NULL"), "NULL grad_values");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p, p, nullptr), "pointers"), "NULL out_grad_queries");
        expect(says(posterior_expectation_backward_args_error(p, 2, -1, 1.f, nullptr, 0, p, p, p, p, p), "pointers"), "nq < 0");
        expect(says(posterior_expectation_backward_args_error(p, 3, 5, 1.f, nullptr, 0, p, p, p, p, p), "q_dtype"), "q_dtype 3");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 0.f, nullptr, 0, p, p, p, p, p), "beta"), "beta 0");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, -INFINITY, nullptr, 0, p, p, p, p, p), "beta"), "beta -inf");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, NAN, nullptr, 0, p, p, p, p, p), "beta"), "beta NaN");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 1.f, p, 65, p, p, p, p, p), "n_per_query"), "n_per_query 65");
        expect(says(posterior_expectation_backward_args_error(p, 2, 5, 1.f, p, 0, p, p, p, p, p), "n_per_query"), "n_per_query 0");
    }

    // ---- the fold against a long-double sum; a single shard is copied bit for bit
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> val(-1.0, 1.0), mag(-30.0, 8.0);
    for (int trial = 0; trial < 300; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t nq = 1 + (int64_t)(rng() % 9);
        const int64_t dim = trial % 5 == 0 ? 1 : (trial % 5 == 1 ? 768 : 1 + (int64_t)(rng() % 300));
        const size_t per = (size_t)(nq * dim);
        std::vector<float> parts((size_t)G * per);
        for (int g = 0; g < G; ++g) {
            const bool empty = g == G - 1 && trial % 2 == 0;  // (a shard that holds no row returns zeros)
            for (size_t i = 0; i < per; ++i) parts[(size_t)g * per + i] = empty ? 0.f : (float)(val(rng) * std::exp2(std::floor(mag(rng))));
        }
        std::vector<float> out(per, 123.f);
        fold_posterior_expectation_backward(parts.data(), G, nq, dim, out.data());
        bool ok = true;
        for (size_t i = 0; i < per; ++i) {
            long double want = 0.0L, sum_abs = 0.0L;
            for (int g = 0; g < G; ++g) {
                want += parts[(size_t)g * per + i];
                sum_abs += std::fabs((long double)parts[(size_t)g * per + i]);
            }
            // G - 1 double additions and one rounding to float32
            ok = ok && std::fabs((double)((long double)out[i] - want)) <= (double)(sum_abs * (6.0e-8L + 8 * 1.2e-16L)) + 1e-45;
            if (G == 1) ok = ok && std::memcmp(&out[i], &parts[i], sizeof(float)) == 0;
        }
        expect(ok, "the shard rows add");
    }
    {   // a NaN row of one shard (a non-finite g) stays a NaN row, the other rows stay clean
        const int64_t nq = 2, dim = 3;
        std::vector<float> parts = {1.f, 2.f, 3.f, NAN, NAN, NAN, 4.f, 5.f, 6.f, NAN, NAN, NAN};
        std::vector<float> out((size_t)(nq * dim));
        fold_posterior_expectation_backward(parts.data(), 2, nq, dim, out.data());
        expect(out[0] == 5.f && out[1] == 7.f && out[2] == 9.f, "clean rows add");
        expect(std::isnan(out[3]) && std::isnan(out[4]) && std::isnan(out[5]), "a NaN row stays NaN");
    }
    {
        float none = 7.f;
        fold_posterior_expectation_backward(&none, 3, 0, 5, &none);  // nq == 0 touches nothing
        expect(none == 7.f, "nq == 0 writes nothing");
    }
    std::printf("%ld checks, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
