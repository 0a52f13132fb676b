// Stand-alone check of the host-only pieces of the in-place row update (vod_amd/csrc/update_fold.h): every refusal of the argument
// check, the routing of a listed call's slots to 1, 2, 3 and 8 shards against a direct restatement (ids on shard edges, duplicates,
// pads, exactly sized buffers), that "the last slot wins" survives the routing, and the dense form's split at shard boundaries.  Built
// with -fsanitize=address,undefined by tests/test_update_rows_cpu.py and run directly; prints "<n> checks, <e> errors".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "update_fold.h"

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

// which slot writes which global row when the slots are applied in the given order: the last one that lists it
std::map<int64_t, int64_t> winners(const std::vector<int64_t>& ids, const std::vector<int64_t>& order, int64_t ntotal) {
    std::map<int64_t, int64_t> w;
    for (int64_t j : order)
        if (ids[(size_t)j] >= 0 && ids[(size_t)j] < ntotal) w[ids[(size_t)j]] = j;
    return w;
}

void check_route(const std::vector<int64_t>& ids, int64_t rps, int G, int64_t ntotal, const char* what) {
    using namespace vodhip;
    const int64_t n = (int64_t)ids.size();
    const UpdateRoute r = route_update_slots(ids.data(), n, rps, G, ntotal);  // (ids.data() of an empty vector may be NULL: nothing is read)
    expect((int)r.first.size() == G + 1 && r.first[0] == 0 && r.first[(size_t)G] == (int64_t)r.slot.size(), what);
    int64_t skipped = 0;
    for (int64_t id : ids) skipped += id < 0 || id >= ntotal;
    expect(r.skipped == skipped && (int64_t)r.slot.size() == n - skipped, what);
    bool ok = true;
    std::vector<char> seen((size_t)n, 0);
    for (int g = 0; g < G; ++g) {
        ok = ok && r.first[(size_t)g] <= r.first[(size_t)g + 1];
        for (int64_t i = r.first[(size_t)g]; i < r.first[(size_t)g + 1]; ++i) {
            const int64_t j = r.slot[(size_t)i];
            ok = ok && j >= 0 && j < n && !seen[(size_t)j];
            if (!(j >= 0 && j < n)) continue;
            seen[(size_t)j] = 1;
            ok = ok && ids[(size_t)j] >= 0 && ids[(size_t)j] < ntotal && ids[(size_t)j] / rps == g;  // its owning shard
            if (i > r.first[(size_t)g]) ok = ok && r.slot[(size_t)i - 1] < j;                          // slot order kept inside a shard
        }
    }
    expect(ok, what);
    // the shards applied in any order, each in its own slot order, leave every row to the slot the unrouted call leaves it to
    std::vector<int64_t> plain((size_t)n);
    for (int64_t j = 0; j < n; ++j) plain[(size_t)j] = j;
    std::vector<int64_t> backwards;
    for (int g = G - 1; g >= 0; --g)
        for (int64_t i = r.first[(size_t)g]; i < r.first[(size_t)g + 1]; ++i) backwards.push_back(r.slot[(size_t)i]);
    expect(winners(ids, plain, ntotal) == winners(ids, backwards, ntotal), what);
}

}  // namespace

int main() {
    using namespace vodhip;

    // ---- every refusal of the argument check, and what passes
    {
        int a = 0;
        const void* p = &a;
        const void* N = nullptr;
        expect(update_rows_args_error(true, 0, p, 5, 2, 0, UPDATE_SET, 1.f, 100) == nullptr, "a listed SET");
        expect(update_rows_args_error(true, -99, p, 5, 0, 1, UPDATE_ADD, -0.5f, 0) == nullptr, "a listed call reads neither row_begin nor ntotal");
        expect(update_rows_args_error(false, 95, p, 5, 1, 1, UPDATE_ADD, 3e-4f, 100) == nullptr, "a dense range up to the end");
        expect(update_rows_args_error(false, 100, N, 0, 2, 0, UPDATE_SET, 1.f, 100) == nullptr, "n == 0 at the end, NULL rows");
        expect(update_rows_args_error(true, 0, N, 0, 2, 0, UPDATE_SET, 1.f, 0) == nullptr, "n == 0, listed");
        expect(update_rows_args_error(true, 0, p, 5, 2, 0, UPDATE_SET, NAN, 100) == nullptr, "SET ignores alpha");
        expect(update_rows_args_error(true, 0, p, 5, 2, 0, UPDATE_SET, INFINITY, 100) == nullptr, "SET ignores alpha (inf)");
        expect(says(update_rows_args_error(true, 0, p, -1, 2, 0, UPDATE_SET, 1.f, 100), "negative"), "n < 0");
        expect(says(update_rows_args_error(true, 0, N, 1, 2, 0, UPDATE_SET, 1.f, 100), "rows is NULL"), "NULL rows");
        expect(says(update_rows_args_error(true, 0, p, 1, 3, 0, UPDATE_SET, 1.f, 100), "src_dtype"), "dtype 3");
        expect(says(update_rows_args_error(true, 0, p, 1, -1, 0, UPDATE_SET, 1.f, 100), "src_dtype"), "dtype -1");
        expect(says(update_rows_args_error(true, 0, p, 1, 2, 2, UPDATE_SET, 1.f, 100), "location"), "location 2");
        expect(says(update_rows_args_error(true, 0, p, 1, 2, -1, UPDATE_SET, 1.f, 100), "location"), "location -1");
        expect(says(update_rows_args_error(true, 0, p, 1, 2, 0, 2, 1.f, 100), "mode"), "mode 2");
        expect(says(update_rows_args_error(true, 0, p, 1, 2, 0, -1, 1.f, 100), "mode"), "mode -1");
        expect(says(update_rows_args_error(true, 0, p, 1, 2, 0, UPDATE_ADD, NAN, 100), "alpha"), "ADD with NaN");
        expect(says(update_rows_args_error(true, 0, p, 1, 2, 0, UPDATE_ADD, INFINITY, 100), "alpha"), "ADD with inf");
        expect(says(update_rows_args_error(true, 0, p, 1, 2, 0, UPDATE_ADD, -INFINITY, 100), "alpha"), "ADD with -inf");
        expect(says(update_rows_args_error(true, 0, p, (1ll << 31) - 1, 2, 0, UPDATE_SET, 1.f, 100), "2^31"), "a slot number beyond an int32");
        expect(update_rows_args_error(true, 0, p, (1ll << 31) - 2, 2, 0, UPDATE_SET, 1.f, 100) == nullptr, "the largest list");
        expect(says(update_rows_args_error(false, -1, p, 1, 2, 0, UPDATE_SET, 1.f, 100), "out of bounds"), "row_begin < 0");
        expect(says(update_rows_args_error(false, 96, p, 5, 2, 0, UPDATE_SET, 1.f, 100), "out of bounds"), "one row past the end");
        expect(says(update_rows_args_error(false, 101, p, 0, 2, 0, UPDATE_SET, 1.f, 100), "out of bounds"), "an empty range past the end");
        expect(says(update_rows_args_error(false, INT64_MAX, p, 5, 2, 0, UPDATE_SET, 1.f, 100), "out of bounds"), "row_begin + n overflows");
        expect(says(update_rows_args_error(false, 0, p, 1, 2, 0, UPDATE_SET, 1.f, 0), "out of bounds"), "an empty store");
    }

    // ---- routing: hand-written lists at 1, 2, 3 and 8 shards
    for (int G : {1, 2, 3, 8}) {
        const int64_t ntotal = 96, rps = (ntotal + G - 1) / G;
        check_route({}, rps, G, ntotal, "the empty list");
        check_route({5}, rps, G, ntotal, "one slot");
        check_route({0, rps - 1, rps, 2 * rps - 1, 2 * rps, ntotal - 1}, rps, G, ntotal, "ids on the shard edges");
        check_route({7, 7, 7}, rps, G, ntotal, "three slots, one id");
        check_route({rps - 1, rps, rps - 1, rps, rps - 1}, rps, G, ntotal, "duplicates on both sides of an edge");
        check_route({-1, ntotal, -5, ntotal + 1000, INT64_MAX, INT64_MIN}, rps, G, ntotal, "nothing but pads and strangers");
        check_route({3, -1, 3, ntotal, 90, 3, -1, 90}, rps, G, ntotal, "pads between duplicates");
        std::vector<int64_t> all;
        for (int64_t i = ntotal - 1; i >= 0; --i) all.push_back(i);
        check_route(all, rps, G, ntotal, "every row once, backwards");
        std::vector<int64_t> same((size_t)257, ntotal - 1);
        check_route(same, rps, G, ntotal, "257 slots, the last row");
    }
    // a store that does not fill its last shards: ids behind ntotal belong to no shard even when a shard's range covers them
    check_route({0, 49, 50, 51, 99, 100}, 25, 8, 51, "a half-filled node index");
    {
        const int64_t ids[] = {10, 60, 10};
        const vodhip::UpdateRoute r = route_update_slots(ids, 3, 50, 2, 100);
        expect(r.first == std::vector<int64_t>({0, 2, 3}) && r.slot == std::vector<int64_t>({0, 2, 1}) && r.skipped == 0, "the partition by hand");
    }
    // ---- routing: random lists with duplicates that straddle nothing and everything
    std::mt19937_64 rng(20261021);
    for (int trial = 0; trial < 300; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t capacity = 1 + (int64_t)(rng() % 400);
        const int64_t rps = (capacity + G - 1) / G;
        const int64_t ntotal = trial % 4 == 0 ? capacity : (int64_t)(rng() % (uint64_t)(capacity + 1));
        const int64_t n = (int64_t)(rng() % 600);
        const int64_t span = trial % 3 == 0 ? 3 : capacity + 20;  // few distinct ids: nearly every slot is a duplicate
        std::vector<int64_t> ids((size_t)n);
        for (int64_t& id : ids) id = (int64_t)(rng() % (uint64_t)span) - 5;
        check_route(ids, rps, G, ntotal, "a random list");
    }

    // ---- the dense form splits at shard boundaries: the parts are disjoint, in order, and cover the range exactly
    for (int trial = 0; trial < 300; ++trial) {
        const int G = 1 + (int)(rng() % 8);
        const int64_t capacity = 1 + (int64_t)(rng() % 400);
        const int64_t rps = (capacity + G - 1) / G;
        const int64_t begin = (int64_t)(rng() % (uint64_t)capacity), n = (int64_t)(rng() % (uint64_t)(capacity - begin + 1));
        int64_t next = 0;
        bool ok = true;
        for (int g = 0; g < G; ++g) {
            int64_t lo = -1, hi = -1;
            split_update_range(begin, n, rps, g, &lo, &hi);
            if (hi == lo) continue;
            ok = ok && lo == next && hi > lo && hi <= n;
            ok = ok && (begin + lo) / rps == g && (begin + hi - 1) / rps == g;  // every row of the part is the shard's
            next = hi;
        }
        expect(ok && next == n, "the dense split");
    }
    {
        int64_t lo, hi;
        split_update_range(90, 30, 100, 0, &lo, &hi);
        expect(lo == 0 && hi == 10, "rows 90 .. 99 are shard 0's");
        split_update_range(90, 30, 100, 1, &lo, &hi);
        expect(lo == 10 && hi == 30, "rows 100 .. 119 are shard 1's");
        split_update_range(90, 30, 100, 2, &lo, &hi);
        expect(lo == hi, "shard 2 gets nothing");
        split_update_range(50, 0, 100, 0, &lo, &hi);
        expect(lo == hi, "an empty range");
    }
    std::printf("%ld checks, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
