// Stand-alone check of the host-only pieces of row removal (vod_amd/csrc/remove_fold.h): every refusal of the argument check, the
// SLAB PLAN of a flat index against a brute-force simulation on a host array, and the SEGMENT PLAN of a node index against the layout
// `add` fills.  The simulation models a launch as the device may run it: a DIRECT slab's reads may all happen AFTER all writes of the
// same launch (the writes are applied first, the reads are taken from the array as it then is); a BOUNCED slab reads the array as the
// earlier launches left it, then writes.  Executed in order, the launches must leave exactly the survivors, in order, in rows
// [0, survivors) - and must not write below the first removed row.  Built with -fsanitize=address,undefined by
// tests/test_remove_rows_cpu.py and run directly; prints "<n> checks, <e> errors".
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "remove_fold.h"

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

// what the count and scan launches hand the host: tiles of tile_rows from tile_base, cut at ntotal
std::vector<int32_t> tile_offsets(const std::vector<char>& removed, int64_t tile_base, int64_t tile_rows) {
    const int64_t ntotal = (int64_t)removed.size();
    const int64_t n_tiles = (ntotal - tile_base + tile_rows - 1) / tile_rows;
    std::vector<int32_t> off((size_t)n_tiles + 1, 0);
    for (int64_t t = 0; t < n_tiles; ++t) {
        int32_t c = 0;
        for (int64_t r = tile_base + t * tile_rows; r < ntotal && r < tile_base + (t + 1) * tile_rows; ++r) c += !removed[(size_t)r];
        off[(size_t)t + 1] = off[(size_t)t] + c;
    }
    return off;
}

void check_slabs(const std::vector<char>& removed, int64_t slab_rows, int64_t tile_base, const char* what) {
    using namespace vodhip;
    const int64_t ntotal = (int64_t)removed.size();
    const int64_t T = remove_tile_rows(slab_rows);
    expect(remove_slab_rows_ok(slab_rows) && slab_rows % T == 0 && 256 % T == 0 && tile_base % T == 0, what);
    int64_t first = ntotal, survivors = 0;
    for (int64_t r = ntotal - 1; r >= 0; --r) {
        if (removed[(size_t)r]) first = r;
        else ++survivors;
    }
    if (first < tile_base) return;  // (not a case the caller produces: the tiles start at or below the first removed row)
    const std::vector<int32_t> off = tile_offsets(removed, tile_base, T);
    const int64_t n_tiles = (int64_t)off.size() - 1;
    const RemovePlan plan = plan_remove_slabs(off.data(), n_tiles, tile_base, T, ntotal, first, slab_rows);
    expect(plan.survivors == survivors, what);
    std::vector<int64_t> x((size_t)ntotal);  // the store: row r holds the value r
    for (int64_t r = 0; r < ntotal; ++r) x[(size_t)r] = r;
    std::vector<int64_t> new_id((size_t)ntotal, -1);
    for (int64_t r = 0, k = 0; r < ntotal; ++r)
        if (!removed[(size_t)r]) new_id[(size_t)r] = k++;
    bool ok = true;
    int64_t prev_end = first;
    int64_t n_direct = 0, n_bounced = 0;
    for (const RemoveSlab& s : plan.slabs) {
        ok = ok && s.src_begin >= first && s.src_begin >= prev_end && s.src_rows > 0 && s.src_begin + s.src_rows <= ntotal && s.n_keep > 0 && s.n_keep <= slab_rows;
        ok = ok && s.dst_begin >= first && s.dst_begin <= s.src_begin && s.dst_begin + s.n_keep <= s.src_begin + s.src_rows;
        ok = ok && s.bounced == (s.dst_begin + s.n_keep > s.src_begin);
        if (!ok) break;
        prev_end = s.src_begin + s.src_rows;
        // the launch's moves (source row -> destination row), from the marks alone
        std::vector<int64_t> src_of, dst_of;
        for (int64_t r = s.src_begin; r < s.src_begin + s.src_rows; ++r)
            if (!removed[(size_t)r]) src_of.push_back(r), dst_of.push_back(new_id[(size_t)r]);
        ok = ok && (int64_t)src_of.size() == s.n_keep && (src_of.empty() || (dst_of.front() == s.dst_begin && dst_of.back() == s.dst_begin + s.n_keep - 1));
        if (!ok) break;
        if (s.bounced) {
            ++n_bounced;
            std::vector<int64_t> bounce((size_t)s.n_keep);
            for (size_t i = 0; i < src_of.size(); ++i) bounce[(size_t)(dst_of[i] - s.dst_begin)] = x[(size_t)src_of[i]];
            for (int64_t i = 0; i < s.n_keep; ++i) x[(size_t)(s.dst_begin + i)] = bounce[(size_t)i];
        } else {
            ++n_direct;
            // the worst order a launch may take: every write lands before any read happens.  The value a write carries is the one the
            // row held BEFORE the launch only if no write of the launch covers that row - which is what the plan must guarantee
            std::vector<char> written((size_t)ntotal, 0);
            for (int64_t d : dst_of) written[(size_t)d] = 1;
            for (size_t i = 0; i < src_of.size(); ++i) {
                ok = ok && !written[(size_t)src_of[i]];  // a read after the writes would see another row's bytes
                x[(size_t)dst_of[i]] = x[(size_t)src_of[i]];
            }
        }
    }
    expect(ok, what);
    bool same = true;
    for (int64_t r = 0, k = 0; r < ntotal; ++r)
        if (!removed[(size_t)r]) same = same && x[(size_t)k++] == r;
    expect(same, what);
    if (survivors == ntotal || survivors == 0) expect(plan.slabs.empty() || survivors == 0, what);
    (void)n_direct;
    (void)n_bounced;
}

void slab_cases() {
    std::mt19937_64 rng(7);
    const int64_t slabs[] = {4, 64, 65536};
    const int64_t sizes[] = {1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1029, 2000};
    for (int64_t slab : slabs) {
        for (int64_t n : sizes) {
            std::vector<char> m((size_t)n, 0);
            check_slabs(m, slab, 0, "none removed");
            std::fill(m.begin(), m.end(), 1);
            check_slabs(m, slab, 0, "all removed");
            std::fill(m.begin(), m.end(), 0);
            m[0] = 1;
            check_slabs(m, slab, 0, "only row 0");
            m[0] = 0;
            m[(size_t)n - 1] = 1;
            check_slabs(m, slab, 0, "only the last row");
            const int64_t T = vodhip::remove_tile_rows(slab);
            check_slabs(m, slab, (n - 1) / T * T, "only the last row, tiles from its tile (the range form)");
            for (int64_t r = 0; r < n; ++r) m[(size_t)r] = (char)(r & 1);
            check_slabs(m, slab, 0, "alternating rows, odd removed");
            for (int64_t r = 0; r < n; ++r) m[(size_t)r] = (char)!(r & 1);
            check_slabs(m, slab, 0, "alternating rows, even removed");
            // a slab without a survivor in the middle, and a removed range by the range form
            std::fill(m.begin(), m.end(), 0);
            for (int64_t r = n / 3; r < n / 3 + 2 * slab && r < n; ++r) m[(size_t)r] = 1;
            check_slabs(m, slab, 0, "a slab with no survivor");
            check_slabs(m, slab, (n / 3) / T * T, "a removed range, tiles from its first row's tile");
            for (int rep = 0; rep < 12; ++rep) {
                const double p = rep < 4 ? 0.01 : rep < 8 ? 0.25 : 0.9;
                for (int64_t r = 0; r < n; ++r) m[(size_t)r] = (char)(std::uniform_real_distribution<double>(0, 1)(rng) < p);
                check_slabs(m, slab, 0, "random mask");
            }
        }
    }
    // a store larger than one default slab: 3 slabs of 65536, ntotal no multiple of tile or slab
    std::vector<char> big(3 * 65536 - 77, 0);
    big[0] = 1;
    check_slabs(big, 65536, 0, "row 0 of a three-slab store: every slab bounced");
    for (size_t r = 0; r < big.size(); ++r) big[r] = (char)(r & 1);
    check_slabs(big, 65536, 0, "every other row of a three-slab store");
    {
        using namespace vodhip;
        const std::vector<int32_t> off = tile_offsets(big, 0, 256);
        const RemovePlan plan = plan_remove_slabs(off.data(), (int64_t)off.size() - 1, 0, 256, (int64_t)big.size(), 0, 65536);
        expect(plan.slabs.size() == 3 && plan.slabs[0].bounced && !plan.slabs[1].bounced && !plan.slabs[2].bounced, "every other row: the first slab bounced, the others direct");
    }
    expect(!vodhip::remove_slab_rows_ok(0) && !vodhip::remove_slab_rows_ok(2) && !vodhip::remove_slab_rows_ok(6) && !vodhip::remove_slab_rows_ok(96) &&
               vodhip::remove_slab_rows_ok(4) && vodhip::remove_slab_rows_ok(64) && vodhip::remove_slab_rows_ok(65536) && !vodhip::remove_slab_rows_ok(1ll << 31),
           "remove_slab_rows_ok");
    expect(vodhip::remove_tile_rows(4) == 4 && vodhip::remove_tile_rows(64) == 64 && vodhip::remove_tile_rows(256) == 256 && vodhip::remove_tile_rows(65536) == 256,
           "remove_tile_rows");
}

// ---- the segment plan ---------------------------------------------------------------------------------------------------------------
struct SegmentFacts { bool crosses = false, empties = false, stays_full = false, overlaps = false; };

SegmentFacts check_segments(const std::vector<int64_t>& before, const std::vector<int64_t>& keep, int64_t rps, const char* what) {
    using namespace vodhip;
    const int G = (int)keep.size();
    SegmentFacts f;
    // shard g rows [0, keep[g]) hold the survivors' global ranks in order (after the local compaction); behind them stale values
    std::vector<std::vector<int64_t>> x((size_t)G);
    int64_t rank = 0;
    for (int g = 0; g < G; ++g) {
        x[(size_t)g].assign((size_t)rps, -7);
        for (int64_t r = 0; r < keep[(size_t)g]; ++r) x[(size_t)g][(size_t)r] = rank++;
    }
    const int64_t total = rank;
    const RemoveSegmentPlan plan = plan_remove_segments(keep.data(), G, rps);
    bool ok = (int)plan.ntotal.size() == G;
    for (const RemoveSegment& s : plan.segments) {
        ok = ok && s.n > 0 && s.src_shard >= 0 && s.src_shard < G && s.dst_shard >= 0 && s.dst_shard <= s.src_shard && s.src_row >= 0 &&
             s.src_row + s.n <= keep[(size_t)s.src_shard] && s.dst_row >= 0 && s.dst_row + s.n <= rps;  // (split at the destination shard's end)
        if (!ok) break;
        const bool same = s.src_shard == s.dst_shard;
        ok = ok && (!same || s.dst_row < s.src_row) && s.overlaps == (same && s.dst_row + s.n > s.src_row);
        f.overlaps = f.overlaps || s.overlaps;
        f.crosses = f.crosses || !same;
        std::vector<int64_t>& src = x[(size_t)s.src_shard];
        std::vector<int64_t>& dst = x[(size_t)s.dst_shard];
        if (s.overlaps) {  // through the bounce buffer: all reads, then all writes
            const std::vector<int64_t> tmp(src.begin() + s.src_row, src.begin() + s.src_row + s.n);
            for (int64_t i = 0; i < s.n; ++i) dst[(size_t)(s.dst_row + i)] = tmp[(size_t)i];
        } else {  // a plain copy, in the worst order for a forward overlap: back to front would be safe, so go front to back AND check disjointness
            ok = ok && (!same || s.dst_row + s.n <= s.src_row);
            for (int64_t i = 0; i < s.n; ++i) dst[(size_t)(s.dst_row + i)] = src[(size_t)(s.src_row + i)];
        }
    }
    expect(ok, what);
    bool laid = true;
    int64_t sum = 0;
    for (int g = 0; g < G; ++g) {
        const int64_t want = total - g * rps < 0 ? 0 : (total - g * rps > rps ? rps : total - g * rps);
        laid = laid && plan.ntotal[(size_t)g] == want;
        for (int64_t r = 0; r < want; ++r) laid = laid && x[(size_t)g][(size_t)r] == g * rps + r;
        sum += plan.ntotal[(size_t)g];
        f.empties = f.empties || (before[(size_t)g] > 0 && want == 0);
        f.stays_full = f.stays_full || (before[(size_t)g] == rps && keep[(size_t)g] == rps && want == rps);
    }
    expect(laid && sum == total, what);
    return f;
}

void segment_cases() {
    std::mt19937_64 rng(11);
    SegmentFacts seen;
    auto note = [&](const SegmentFacts& f) {
        seen.crosses |= f.crosses, seen.empties |= f.empties, seen.stays_full |= f.stays_full, seen.overlaps |= f.overlaps;
    };
    for (int G : {1, 2, 3, 8}) {
        for (int64_t rps : {1, 5, 400}) {
            // before the removal the shards are filled in order
            for (int rep = 0; rep < 40; ++rep) {
                const int64_t ntotal = std::uniform_int_distribution<int64_t>(0, G * rps)(rng);
                std::vector<int64_t> before((size_t)G), keep((size_t)G);
                for (int g = 0; g < G; ++g) {
                    before[(size_t)g] = ntotal - g * rps < 0 ? 0 : (ntotal - g * rps > rps ? rps : ntotal - g * rps);
                    const int kind = std::uniform_int_distribution<int>(0, 3)(rng);
                    keep[(size_t)g] = kind == 0 ? before[(size_t)g] : kind == 1 ? 0 : std::uniform_int_distribution<int64_t>(0, before[(size_t)g])(rng);
                }
                note(check_segments(before, keep, rps, "random survivors"));
            }
        }
    }
    // by hand: 3 shards of 400, all full
    note(check_segments({400, 400, 400}, {400, 400, 400}, 400, "nothing removed"));
    expect(vodhip::plan_remove_segments(std::vector<int64_t>{400, 400, 400}.data(), 3, 400).segments.empty(), "nothing removed: no segment");
    note(check_segments({400, 400, 400}, {400, 0, 400}, 400, "the middle shard empties: the last one moves down whole"));
    note(check_segments({400, 400, 400}, {390, 400, 400}, 400, "ten rows of shard 0 left: every later shard shifts by ten, overlapping itself"));
    note(check_segments({400, 400, 300}, {400, 395, 300}, 400, "shard 0 stays full, shard 1 loses five"));
    note(check_segments({400, 400, 400}, {0, 0, 0}, 400, "all removed"));
    note(check_segments({400, 400, 400}, {1, 1, 1}, 400, "one survivor per shard"));
    {
        using namespace vodhip;
        const std::vector<int64_t> keep = {390, 400, 400};
        const RemoveSegmentPlan p = plan_remove_segments(keep.data(), 3, 400);
        // shard 1 -> (0, 390, 10), (1, 0, 390 overlapping); shard 2 -> (1, 390, 10), (2, 0, 390 overlapping)
        expect(p.segments.size() == 4 && p.segments[0].dst_shard == 0 && p.segments[0].dst_row == 390 && p.segments[0].n == 10 && !p.segments[0].overlaps &&
                   p.segments[1].src_shard == 1 && p.segments[1].dst_shard == 1 && p.segments[1].src_row == 10 && p.segments[1].dst_row == 0 && p.segments[1].n == 390 &&
                   p.segments[1].overlaps && p.ntotal[0] == 400 && p.ntotal[1] == 400 && p.ntotal[2] == 390,
               "a segment that crosses a shard boundary is split there");
    }
    expect(seen.crosses && seen.empties && seen.stays_full && seen.overlaps, "the cases cover a crossing, an emptied shard, a full one and an overlap");
    // the dense form's split
    int64_t lo, hi;
    vodhip::split_remove_range(390, 20, 400, 0, &lo, &hi);
    expect(lo == 390 && hi == 400, "range split, shard 0");
    vodhip::split_remove_range(390, 20, 400, 1, &lo, &hi);
    expect(lo == 0 && hi == 10, "range split, shard 1");
    vodhip::split_remove_range(390, 20, 400, 2, &lo, &hi);
    expect(lo == 0 && hi == 0, "range split, a shard the range misses");
    vodhip::split_remove_range(0, 0, 400, 0, &lo, &hi);
    expect(lo == 0 && hi == 0, "range split, an empty range");
}

void argument_cases() {
    using namespace vodhip;
    expect(remove_rows_args_error(true, 0, 5, 0, 10) == nullptr && remove_rows_args_error(false, 3, 7, 1, 10) == nullptr, "accepted calls");
    expect(remove_rows_args_error(true, 0, 0, 0, 0) == nullptr && remove_rows_args_error(false, 10, 0, 0, 10) == nullptr, "empty calls");
    expect(says(remove_rows_args_error(true, 0, -1, 0, 10), "negative"), "n < 0");
    expect(says(remove_rows_args_error(true, 0, (1ll << 31) - 1, 0, 10), "2^31"), "n = 2^31 - 1");
    expect(remove_rows_args_error(true, 0, (1ll << 31) - 2, 0, 10) == nullptr, "n = 2^31 - 2 (a list may repeat ids)");
    expect(says(remove_rows_args_error(true, 0, 1, 2, 10), "location") && says(remove_rows_args_error(false, 0, 1, -1, 10), "location"), "a bad location");
    expect(says(remove_rows_args_error(false, -1, 1, 0, 10), "out of bounds") && says(remove_rows_args_error(false, 4, 7, 0, 10), "out of bounds") &&
               says(remove_rows_args_error(false, 11, 0, 0, 10), "out of bounds"),
           "a range outside the store");
    expect(remove_rows_args_error(true, -5, 1, 0, 10) == nullptr, "the listed form does not read row_begin");
    expect(says(remove_rows_args_error(false, INT64_MAX, 2, 0, 10), "out of bounds"), "no overflow in the range check");
}

}  // namespace

int main() {
    argument_cases();
    slab_cases();
    segment_cases();
    std::printf("%ld checks, %ld errors\n", g_checked, g_errors);
    return g_errors ? 1 : 0;
}
