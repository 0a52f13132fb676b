// Stand-alone check of the host-only pieces of the read-out's adjoint (vod_amd/csrc/readout_adjoint_fold.h): the argument checks, the
// padded width, and the placement of the per-shard slabs into the global result - against a direct statement of the shard row ranges,
// with exactly sized buffers (ASan: nothing past them is touched).  Built with -fsanitize=address,undefined by
// tests/test_posterior_adjoint_cpu.py and run directly; prints "<n> checks, <e> errors".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "readout_adjoint_fold.h"

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

    // ---- argument refusals: log_partition's, then the width and the NULL pointers
    {
        int a = 0;
        const void* p = &a;
        expect(posterior_adjoint_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p, 1, p) == nullptr, "a good call");
        expect(posterior_adjoint_args_error(p, 0, 5, 0.25f, p, 64, p, p, p, 256, p) == nullptr, "a good call with labels, 256 columns");
        expect(posterior_adjoint_args_error(nullptr, 2, 0, 1.f, nullptr, 0, nullptr, nullptr, nullptr, 7, p) == nullptr, "nq == 0 needs only out");
        expect(says(posterior_adjoint_args_error(nullptr, 2, 5, 1.f, nullptr, 0, p, p, p, 1, p), "pointers"), "NULL queries");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, nullptr, 0, nullptr, p, p, 1, p), "pointers"), "NULL max_score");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, nullptr, 0, p, nullptr, p, 1, p), "pointers"), "NULL log_rel");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, nullptr, 1, p), "weights is NULL"), "NULL weights");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p, 1, nullptr), "out is NULL"), "NULL out");
        expect(says(posterior_adjoint_args_error(nullptr, 2, 0, 1.f, nullptr, 0, nullptr, nullptr, nullptr, 1, nullptr), "out is NULL"), "NULL out at nq == 0");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p, 0, p), "n_cols"), "width 0");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, nullptr, 0, p, p, p, 257, p), "n_cols"), "width 257");
        expect(says(posterior_adjoint_args_error(p, 2, 0, 1.f, nullptr, 0, p, p, p, -3, p), "n_cols"), "a negative width at nq == 0");
        expect(says(posterior_adjoint_args_error(p, 2, -1, 1.f, nullptr, 0, p, p, p, 1, p), "pointers"), "nq < 0");
        expect(says(posterior_adjoint_args_error(p, 3, 5, 1.f, nullptr, 0, p, p, p, 1, p), "q_dtype"), "q_dtype 3");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 0.f, nullptr, 0, p, p, p, 1, p), "beta"), "beta 0");
        expect(says(posterior_adjoint_args_error(p, 2, 5, -INFINITY, nullptr, 0, p, p, p, 1, p), "beta"), "beta -inf");
        expect(says(posterior_adjoint_args_error(p, 2, 5, NAN, nullptr, 0, p, p, p, 1, p), "beta"), "beta NaN");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, p, 65, p, p, p, 1, p), "n_per_query"), "n_per_query 65");
        expect(says(posterior_adjoint_args_error(p, 2, 5, 1.f, p, 0, p, p, p, 1, p), "n_per_query"), "n_per_query 0");
    }

    // ---- the padded width
    expect(readout_adjoint_c_pad(1) == 64 && readout_adjoint_c_pad(64) == 64 && readout_adjoint_c_pad(65) == 128 && readout_adjoint_c_pad(129) == 192 &&
               readout_adjoint_c_pad(193) == 256 && readout_adjoint_c_pad(256) == 256,
           "c_pad");
    expect(READOUT_ADJOINT_SLICE % 256 == 0, "a slice is whole query tiles");

    // ---- the slabs: shard g's first (hi - lo) rows land at rows [lo, hi) of the result, every row is written exactly once, empty shards
    // write nothing
    std::mt19937_64 rng(20261021);
    for (int trial = 0; trial < 300; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t n_cols = trial % 4 == 0 ? 1 : (trial % 4 == 1 ? 256 : 1 + (int64_t)(rng() % 70));
        const int64_t capacity = 1 + (int64_t)(rng() % 400);
        const int64_t rps = (capacity + G - 1) / G;
        const int64_t ntotal = trial % 7 == 0 ? capacity : (int64_t)(rng() % (uint64_t)(capacity + 1));
        const int64_t slab = rps * n_cols;
        std::vector<float> parts((size_t)(G * slab));
        for (int g = 0; g < G; ++g)
            for (int64_t i = 0; i < slab; ++i) parts[(size_t)(g * slab + i)] = (float)(g * 1000000 + i);
        std::vector<float> out((size_t)(ntotal * n_cols), -1.f);
        for (int g = 0; g < G; ++g) place_posterior_adjoint_slab(parts.data(), slab, g, ntotal, rps, n_cols, out.data());
        bool ok = true;
        for (int64_t z = 0; z < ntotal; ++z)
            for (int64_t c = 0; c < n_cols; ++c) {
                const int64_t g = z / rps, local = z % rps;
                ok = ok && out[(size_t)(z * n_cols + c)] == (float)(g * 1000000 + local * n_cols + c);
            }
        expect(ok, "the slabs are concatenated");
        int64_t covered = 0;
        for (int g = 0; g < G; ++g) {
            int64_t lo, hi;
            readout_shard_rows(ntotal, rps, g, &lo, &hi);
            ok = ok && lo <= hi && hi <= ntotal && hi - lo <= rps;
            covered += hi - lo;
        }
        expect(ok && covered == ntotal, "the shard ranges cover the rows once");
    }
    {
        float none = 7.f;
        place_posterior_adjoint_slab(&none, 0, 2, 0, 5, 3, &none);  // ntotal == 0 touches nothing
        expect(none == 7.f, "ntotal == 0 writes nothing");
    }
    std::printf("%ld checks, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
