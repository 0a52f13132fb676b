// Stand-alone check of vod_amd/csrc/range_fold.h (the host side of a node index's range_search) for the sanitizers: the concatenation of
// per-shard CSR lists in shard order with empty shards and empty queries, a capacity that cuts a list, a shard block shorter than the
// shard's list, int64 limits past 2^31 (lims only: no list of that size is allocated), and the argument checks.  Exact-size heap buffers,
// so that any read or write past a part is a report.  Prints "<n> errors".
#include "range_fold.h"

#include <cstdio>
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
    {   // 3 shards x 4 queries; shard 1 is empty, query 2 is empty everywhere
        const int G = 3;
        const int64_t nq = 4;
        // list lengths [g][q]
        const int64_t len[G][4] = {{2, 0, 0, 1}, {0, 0, 0, 0}, {1, 3, 0, 2}};
        std::vector<int64_t> lims_g((size_t)(G * (nq + 1)));
        int64_t stride = 0;
        for (int g = 0; g < G; ++g) {
            lims_g[(size_t)(g * (nq + 1))] = 0;
            for (int64_t q = 0; q < nq; ++q) lims_g[(size_t)(g * (nq + 1) + q + 1)] = lims_g[(size_t)(g * (nq + 1) + q)] + len[g][q];
            stride = std::max(stride, lims_g[(size_t)(g * (nq + 1) + nq)]);
        }
        CHECK(stride == 6);
        std::vector<float> scores_g((size_t)(G * stride));
        std::vector<int64_t> ids_g((size_t)(G * stride));
        for (int g = 0; g < G; ++g)
            for (int64_t k = 0; k < stride; ++k) {  // shard g, position k: id 1000 g + k, score the same
                ids_g[(size_t)(g * stride + k)] = 1000 * g + k;
                scores_g[(size_t)(g * stride + k)] = (float)(1000 * g + k);
            }
        std::vector<int64_t> lims((size_t)(nq + 1));
        const int64_t total = fold_range_lims(lims_g.data(), G, nq, lims.data());
        CHECK(total == 9);
        const int64_t want_lims[] = {0, 3, 6, 6, 9};
        for (int64_t q = 0; q <= nq; ++q) CHECK(lims[(size_t)q] == want_lims[q]);
        const int64_t want_ids[] = {0, 1, 2000, 2001, 2002, 2003, 2, 2004, 2005};
        {
            std::vector<float> out_s((size_t)total);
            std::vector<int64_t> out_i((size_t)total);
            fold_range_lists(lims_g.data(), scores_g.data(), ids_g.data(), stride, G, nq, lims.data(), out_s.data(), out_i.data(), total);
            for (int64_t k = 0; k < total; ++k) CHECK(out_i[(size_t)k] == want_ids[k] && out_s[(size_t)k] == (float)want_ids[k]);
        }
        for (int64_t cap = 0; cap < total; ++cap) {  // every shorter capacity: an exact-size buffer, the prefix alone is written
            std::vector<float> out_s((size_t)cap);
            std::vector<int64_t> out_i((size_t)cap);
            fold_range_lists(lims_g.data(), scores_g.data(), ids_g.data(), stride, G, nq, lims.data(), out_s.data(), out_i.data(), cap);
            for (int64_t k = 0; k < cap; ++k) CHECK(out_i[(size_t)k] == want_ids[k] && out_s[(size_t)k] == (float)want_ids[k]);
        }
        {   // shard blocks of 4 elements: shard 2's hits 4 and 5 were not held and are not read; their positions keep the fill
            const int64_t short_stride = 4;
            std::vector<float> ss((size_t)(G * short_stride));
            std::vector<int64_t> si((size_t)(G * short_stride));
            for (int g = 0; g < G; ++g)
                for (int64_t k = 0; k < short_stride; ++k) {
                    si[(size_t)(g * short_stride + k)] = 1000 * g + k;
                    ss[(size_t)(g * short_stride + k)] = (float)(1000 * g + k);
                }
            std::vector<float> out_s((size_t)total, -1.f);
            std::vector<int64_t> out_i((size_t)total, -1);
            fold_range_lists(lims_g.data(), ss.data(), si.data(), short_stride, G, nq, lims.data(), out_s.data(), out_i.data(), total);
            for (int64_t k = 0; k < total; ++k) CHECK(out_i[(size_t)k] == (want_ids[k] >= 2004 ? -1 : want_ids[k]));
        }
    }
    {   // limits past 2^31: two shards whose lists of one query are 2^31 - 600 rows each, then a second query
        const int G = 2;
        const int64_t nq = 2;
        const int64_t big = (1ll << 31) - 600;
        const std::vector<int64_t> lims_g = {0, big, big + 5, 0, big, big};
        std::vector<int64_t> lims((size_t)(nq + 1));
        const int64_t total = fold_range_lims(lims_g.data(), G, nq, lims.data());
        CHECK(lims[0] == 0 && lims[1] == 2 * big && lims[2] == 2 * big + 5 && total == lims[2]);
        CHECK(lims[1] > (1ll << 31));
        // a capacity of 3 against that result: query 0 of shard 0 fills it, every later part computes a negative room and copies nothing
        std::vector<float> scores_g = {1.f, 2.f, 3.f, 4.f, 11.f, 12.f, 13.f, 14.f};
        std::vector<int64_t> ids_g = {1, 2, 3, 4, 11, 12, 13, 14};
        std::vector<float> out_s(3);
        std::vector<int64_t> out_i(3);
        fold_range_lists(lims_g.data(), scores_g.data(), ids_g.data(), 4, G, nq, lims.data(), out_s.data(), out_i.data(), 3);
        CHECK(out_i[0] == 1 && out_i[1] == 2 && out_i[2] == 3 && out_s[2] == 3.f);
    }
    {   // no queries, no shards' worth of data: nothing is touched but lims[0]
        int64_t lims0 = -1;
        const int64_t lims_g[2] = {0, 0};
        CHECK(fold_range_lims(lims_g, 2, 0, &lims0) == 0 && lims0 == 0);
        fold_range_lists(lims_g, nullptr, nullptr, 0, 2, 0, &lims0, nullptr, nullptr, 0);
    }
    {   // the argument checks, in their order
        int x = 0;
        CHECK(range_args_error(&x, 0, 1, &x, nullptr, 0, &x, nullptr, nullptr, 0) == nullptr);
        CHECK(range_args_error(nullptr, 0, 0, nullptr, nullptr, 0, &x, nullptr, nullptr, 0) == nullptr);
        CHECK(!std::strcmp(range_args_error(nullptr, 0, 1, &x, nullptr, 0, &x, nullptr, nullptr, 0), "invalid query pointer"));
        CHECK(!std::strcmp(range_args_error(&x, 0, -1, &x, nullptr, 0, &x, nullptr, nullptr, 0), "invalid query pointer"));
        CHECK(!std::strcmp(range_args_error(&x, 3, 1, &x, nullptr, 0, &x, nullptr, nullptr, 0), "invalid q_dtype"));
        CHECK(!std::strcmp(range_args_error(&x, 0, 1, &x, &x, 0, &x, nullptr, nullptr, 0), "n_per_query must be in [1, 64]"));
        CHECK(!std::strcmp(range_args_error(&x, 0, 1, &x, &x, 65, &x, nullptr, nullptr, 0), "n_per_query must be in [1, 64]"));
        CHECK(!std::strcmp(range_args_error(&x, 0, 1, nullptr, nullptr, 0, &x, nullptr, nullptr, 0), "thresholds is NULL"));
        CHECK(!std::strcmp(range_args_error(&x, 0, 1, &x, nullptr, 0, nullptr, nullptr, nullptr, 0), "lims is NULL"));
        CHECK(!std::strcmp(range_args_error(&x, 0, 1, &x, nullptr, 0, &x, &x, nullptr, 4), "out_scores and out_ids must both be given or both be NULL"));
        CHECK(!std::strcmp(range_args_error(&x, 0, 1, &x, nullptr, 0, &x, nullptr, &x, 4), "out_scores and out_ids must both be given or both be NULL"));
        CHECK(!std::strcmp(range_args_error(&x, 0, 1, &x, nullptr, 0, &x, &x, &x, -1), "capacity must be >= 0"));
        CHECK(range_args_error(&x, 2, 1, &x, &x, 64, &x, &x, &x, 0) == nullptr);
    }
    std::printf("range_fold_check: %d errors\n", errors);
    return errors ? 1 : 0;
}
