// Host-side pieces of the in-place row update (kernels_update.hip, include/vodhip.h H2u): the argument check shared by the flat and
// the node entry points, and how a node index routes a call's slots to its shards.  Plain C++ (no HIP):
// tests/sanitize/update_rows_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace vodhip {

constexpr int UPDATE_SET = 0, UPDATE_ADD = 1;  // VODHIP_UPDATE_SET / VODHIP_UPDATE_ADD

// the refusals of an update call that do not depend on the device; `listed` = the call has an id list (row_begin is not read then)
inline const char* update_rows_args_error(bool listed, int64_t row_begin, const void* rows, int64_t n, int src_dtype, int location, int mode,
                                          float alpha, int64_t ntotal) {
    if (n < 0) return "n is negative";
    if (n > 0 && !rows) return "rows is NULL";
    if (src_dtype < 0 || src_dtype > 2) return "invalid src_dtype";
    if (location != 0 && location != 1) return "invalid location";
    if (mode != UPDATE_SET && mode != UPDATE_ADD) return "invalid mode";
    if (mode == UPDATE_ADD && !std::isfinite(alpha)) return "alpha is not finite";
    if (n >= (1ll << 31) - 1) return "n is 2^31 - 1 or more";  // (the owner word of a listed slot is slot + 1 as an int32)
    if (!listed && (row_begin < 0 || row_begin > ntotal || n > ntotal - row_begin)) return "row range out of bounds";
    return nullptr;
}

// The slots of a listed node call by owning shard (shard = id / rows_per_shard): slot[first[g] .. first[g + 1]) are shard g's, in
// increasing slot order - a STABLE partition, so that the last slot that lists a row is still the last one its shard sees.  A slot
// whose id is negative or not below ntotal has no shard: it is counted in `skipped` and goes nowhere.
struct UpdateRoute {
    std::vector<int64_t> slot;
    std::vector<int64_t> first;  // [n_shards + 1]
    int64_t skipped = 0;
};
inline UpdateRoute route_update_slots(const int64_t* ids, int64_t n, int64_t rows_per_shard, int n_shards, int64_t ntotal) {
    UpdateRoute r;
    r.first.assign((size_t)n_shards + 1, 0);
    auto shard_of = [&](int64_t id) -> int64_t {
        if (id < 0 || id >= ntotal || rows_per_shard <= 0) return -1;
        const int64_t g = id / rows_per_shard;
        return g < n_shards ? g : -1;
    };
    for (int64_t j = 0; j < n; ++j) {
        const int64_t g = shard_of(ids[j]);
        if (g < 0) ++r.skipped;
        else ++r.first[(size_t)g + 1];
    }
    for (int g = 0; g < n_shards; ++g) r.first[(size_t)g + 1] += r.first[(size_t)g];
    r.slot.resize((size_t)r.first[(size_t)n_shards]);
    std::vector<int64_t> at(r.first.begin(), r.first.end() - 1);
    for (int64_t j = 0; j < n; ++j) {
        const int64_t g = shard_of(ids[j]);
        if (g >= 0) r.slot[(size_t)at[(size_t)g]++] = j;
    }
    return r;
}

// The dense form: the part of the global rows [row_begin, row_begin + n) inside shard g's range, as rows [*lo, *hi) of the CALL's
// source (0-based slots); empty (*lo == *hi) when the range misses the shard
inline void split_update_range(int64_t row_begin, int64_t n, int64_t rows_per_shard, int g, int64_t* lo, int64_t* hi) {
    const int64_t s_lo = (int64_t)g * rows_per_shard, s_hi = s_lo + rows_per_shard;
    const int64_t a = row_begin > s_lo ? row_begin : s_lo, b = row_begin + n < s_hi ? row_begin + n : s_hi;
    *lo = b > a ? a - row_begin : 0;
    *hi = b > a ? b - row_begin : 0;
}

}  // namespace vodhip
