// Stand-alone check of vod_amd/csrc/rank_fold.h (the host side of a node index's rank calls) for the sanitizers: ownership at shard
// edges, absent slots, a present -inf score, the NaN thresholds of absent slots, int64 sums past 2^32, the -1 of a NaN threshold, and the
// argument checks.  Exact-size heap buffers, so that any read or write past a shard's part is a report.  Prints "<n> errors".
#include "rank_fold.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static int errors = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            ++errors;                                              \
            std::printf("line %d: %s\n", __LINE__, #c);            \
        }                                                          \
    } while (0)

int main() {
    using namespace vodhip;
    const float inf = std::numeric_limits<float>::infinity();
    {   // 3 shards of 100 rows; shard 2 holds only 50 (its rows 50 .. 99 are absent there)
        const int G = 3;
        const int64_t R = 100;
        const std::vector<int64_t> ids = {0, 99, 100, 199, 200, 249, 250, 299, 300, -1, -7, 150, 150, 1ll << 40, 5};
        const int64_t n = (int64_t)ids.size();
        std::vector<float> score_g((size_t)(G * n));
        std::vector<int32_t> row_g((size_t)(G * n));
        for (int g = 0; g < G; ++g)
            for (int64_t i = 0; i < n; ++i) {
                const int64_t local = ids[(size_t)i] - g * R;
                const int64_t held = g == 2 ? 50 : R;
                const bool here = ids[(size_t)i] >= 0 && local >= 0 && local < held;
                row_g[(size_t)(g * n + i)] = here ? (int32_t)local : -1;
                score_g[(size_t)(g * n + i)] = here ? (float)(1000 * g + local) : -inf;  // a wrong shard's value would show
            }
        // slot 14 (id 5, shard 0): present with a -inf score
        score_g[(size_t)(0 * n + 14)] = -inf;
        // a non-owner that claims the row must be ignored: shard 1 "has" id 0
        row_g[(size_t)(1 * n + 0)] = 3;
        score_g[(size_t)(1 * n + 0)] = 777.f;
        std::vector<float> out((size_t)n), thr((size_t)n);
        std::vector<uint8_t> present((size_t)n);
        combine_scan_scores(score_g.data(), row_g.data(), ids.data(), n, G, R, out.data(), present.data());
        rank_thresholds(out.data(), present.data(), n, thr.data());
        const float want[] = {0.f, 99.f, 1000.f, 1099.f, 2000.f, 2049.f, -inf, -inf, -inf, -inf, -inf, 1050.f, 1050.f, -inf, -inf};
        const int pres[] = {1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 1};
        for (int64_t i = 0; i < n; ++i) {
            CHECK(out[(size_t)i] == want[i]);
            CHECK(present[(size_t)i] == pres[i]);
            if (pres[i]) CHECK(std::memcmp(&thr[(size_t)i], &out[(size_t)i], 4) == 0);
            else CHECK(std::isnan(thr[(size_t)i]));
        }
        // rows_per_shard == 0 (a degenerate handle): nothing is owned, nothing divides by zero
        combine_scan_scores(score_g.data(), row_g.data(), ids.data(), n, G, 0, out.data(), present.data());
        for (int64_t i = 0; i < n; ++i) CHECK(out[(size_t)i] == -inf && present[(size_t)i] == 0);
    }
    {   // sums in int64: three shards near 2^31 rows each pass 2^32; a -1 anywhere makes the slot -1; one shard is the identity
        const int G = 3;
        const int64_t n = 4;
        const int64_t big = (1ll << 31) - 600;
        const std::vector<int64_t> count_g = {big, 0, -1, 7, big, 0, -1, 0, big, 5, -1, 1};
        std::vector<int64_t> out((size_t)n);
        sum_counts(count_g.data(), n, G, out.data());
        CHECK(out[0] == 3 * big && out[0] > (1ll << 32));
        CHECK(out[1] == 5);
        CHECK(out[2] == -1);
        CHECK(out[3] == 8);
        const std::vector<int64_t> mixed = {4, -1, 4, 9};  // 2 shards x 2 slots: slot 1 has a -1 in shard 0 only
        std::vector<int64_t> out2(2);
        sum_counts(mixed.data(), 2, 2, out2.data());
        CHECK(out2[0] == 8 && out2[1] == -1);
        sum_counts(count_g.data(), n, 1, out.data());
        CHECK(out[0] == big && out[1] == 0 && out[2] == -1 && out[3] == 7);
        sum_counts(count_g.data(), 0, G, nullptr);  // n == 0 touches nothing
    }
    {   // the argument checks, in their order
        int x = 0;
        CHECK(rank_args_error(&x, 0, 1, 1, nullptr, 0) == nullptr);
        CHECK(rank_args_error(nullptr, 0, 0, 1, nullptr, 0) == nullptr);
        CHECK(!std::strcmp(rank_args_error(nullptr, 0, 1, 1, nullptr, 0), "invalid query pointer"));
        CHECK(!std::strcmp(rank_args_error(&x, 0, -1, 1, nullptr, 0), "invalid query pointer"));
        CHECK(!std::strcmp(rank_args_error(&x, 3, 1, 1, nullptr, 0), "invalid q_dtype"));
        CHECK(!std::strcmp(rank_args_error(&x, -1, 1, 1, nullptr, 0), "invalid q_dtype"));
        CHECK(!std::strcmp(rank_args_error(&x, 0, 1, 0, nullptr, 0), "m must be in [1, 64]"));
        CHECK(!std::strcmp(rank_args_error(&x, 0, 1, 65, nullptr, 0), "m must be in [1, 64]"));
        CHECK(rank_args_error(&x, 0, 1, 64, nullptr, 0) == nullptr);
        CHECK(!std::strcmp(rank_args_error(&x, 0, 1, 1, &x, 0), "n_per_query must be in [1, 64]"));
        CHECK(!std::strcmp(rank_args_error(&x, 0, 1, 1, &x, 65), "n_per_query must be in [1, 64]"));
        CHECK(rank_args_error(&x, 0, 1, 1, &x, 64) == nullptr);
    }
    std::printf("rank_fold_check: %d errors\n", errors);
    return errors ? 1 : 0;
}
