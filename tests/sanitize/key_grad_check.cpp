// Stand-alone check of the host-only pieces of the key gradient (vod_amd/csrc/key_grad_fold.h): the argument checks, the fold of the
// shards' column maxima against a direct maximum over the rows, and the placement of the per-shard slabs of [rows][dim] - with exactly
// sized buffers (ASan: nothing past them is touched).  Built with -fsanitize=address,undefined by tests/test_key_gradient_cpu.py and run
// directly; prints "<n> checks, <e> errors".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "key_grad_fold.h"

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

    // ---- argument refusals: log_partition's, then the gradients and the output
    {
        int a = 0;
        const void* p = &a;
        const void* N = nullptr;
        expect(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, p, p, N, N, p) == nullptr, "log Z only");
        expect(posterior_key_gradient_args_error(p, 0, 5, 0.25f, p, 64, p, p, N, p, p, p) == nullptr, "the table term only, with labels");
        expect(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, p, p, p, p, p) == nullptr, "both");
        expect(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, p, p, p, N, p) == nullptr, "values without grad_values are ignored");
        expect(posterior_key_gradient_args_error(N, 2, 0, 1.f, N, 0, N, N, p, N, N, p) == nullptr, "nq == 0 needs a gradient and out");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, p, N, N, N, p), "both NULL"), "no gradient");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, p, N, p, N, p), "both NULL"), "values alone is no gradient");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, p, p, N, p, p), "without values"), "grad_values without values");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, p, p, N, N, N), "out is NULL"), "NULL out");
        expect(says(posterior_key_gradient_args_error(N, 2, 0, 1.f, N, 0, N, N, p, N, N, N), "out is NULL"), "NULL out at nq == 0");
        expect(says(posterior_key_gradient_args_error(N, 2, 5, 1.f, N, 0, p, p, p, N, N, p), "pointers"), "NULL queries");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, N, p, p, N, N, p), "pointers"), "NULL max_score");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 1.f, N, 0, p, N, p, N, N, p), "pointers"), "NULL log_rel");
        expect(says(posterior_key_gradient_args_error(p, 2, -1, 1.f, N, 0, p, p, p, N, N, p), "pointers"), "nq < 0");
        expect(says(posterior_key_gradient_args_error(p, 3, 5, 1.f, N, 0, p, p, p, N, N, p), "q_dtype"), "q_dtype 3");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 0.f, N, 0, p, p, p, N, N, p), "beta"), "beta 0");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, INFINITY, N, 0, p, p, p, N, N, p), "beta"), "beta inf");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, NAN, N, 0, p, p, p, N, N, p), "beta"), "beta NaN");
        expect(says(posterior_key_gradient_args_error(p, 2, 5, 1.f, p, 65, p, p, p, N, N, p), "n_per_query"), "n_per_query 65");
    }
    expect(KEY_GRAD_SLICE % 256 == 0 && KEY_GRAD_SLICE == READOUT_ADJOINT_SLICE, "a slice is whole query tiles, the adjoint's");

    // ---- the column maxima: the largest of the shards' maxima is the maximum over all the rows; empty shards hold zeros
    std::mt19937_64 rng(20261021);
    for (int trial = 0; trial < 200; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t c_pad = 64 * (1 + (int64_t)(rng() % 4));
        const int64_t capacity = 1 + (int64_t)(rng() % 300);
        const int64_t rps = (capacity + G - 1) / G;
        const int64_t ntotal = trial % 5 == 0 ? capacity : (int64_t)(rng() % (uint64_t)(capacity + 1));
        std::vector<float> table((size_t)(ntotal * c_pad));
        for (float& t : table) t = (float)((int64_t)(rng() % 2001) - 1000) / 8.f;
        std::vector<float> parts((size_t)(G * c_pad), 0.f), want((size_t)c_pad, 0.f), got((size_t)c_pad, -1.f);
        for (int g = 0; g < G; ++g) {
            int64_t lo, hi;
            readout_shard_rows(ntotal, rps, g, &lo, &hi);
            for (int64_t z = lo; z < hi; ++z)
                for (int64_t c = 0; c < c_pad; ++c) parts[(size_t)(g * c_pad + c)] = std::max(parts[(size_t)(g * c_pad + c)], std::fabs(table[(size_t)(z * c_pad + c)]));
        }
        for (int64_t z = 0; z < ntotal; ++z)
            for (int64_t c = 0; c < c_pad; ++c) want[(size_t)c] = std::max(want[(size_t)c], std::fabs(table[(size_t)(z * c_pad + c)]));
        fold_key_grad_vmax(parts.data(), G, c_pad, got.data());
        expect(got == want, "the folded maxima are the maxima over all the rows");
    }
    {
        float none = 7.f;
        fold_key_grad_vmax(&none, 3, 0, &none);  // no table: nothing is read or written
        expect(none == 7.f, "c_pad == 0 touches nothing");
    }

    // ---- the slabs of [rows][dim]: the adjoint's placement with n_cols = dim
    for (int trial = 0; trial < 100; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t dim = trial % 3 == 0 ? 1 : 1 + (int64_t)(rng() % 90);
        const int64_t capacity = 1 + (int64_t)(rng() % 200);
        const int64_t rps = (capacity + G - 1) / G;
        const int64_t ntotal = (int64_t)(rng() % (uint64_t)(capacity + 1));
        const int64_t slab = rps * dim;
        std::vector<float> parts((size_t)(G * slab));
        for (int g = 0; g < G; ++g)
            for (int64_t i = 0; i < slab; ++i) parts[(size_t)(g * slab + i)] = (float)(g * 100000 + i);
        std::vector<float> out((size_t)(ntotal * dim), -1.f);
        for (int g = 0; g < G; ++g) place_posterior_adjoint_slab(parts.data(), slab, g, ntotal, rps, dim, out.data());
        bool ok = true;
        for (int64_t z = 0; z < ntotal; ++z)
            for (int64_t d = 0; d < dim; ++d) ok = ok && out[(size_t)(z * dim + d)] == (float)((z / rps) * 100000 + (z % rps) * dim + d);
        expect(ok, "the slabs are concatenated");
    }
    std::printf("%ld checks, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
