// Host-side pieces of row removal (kernels_remove.hip, include/vodhip.h H2r): the argument check shared by the flat and the node
// entry points, the SLAB PLAN of a flat index's compaction and the SEGMENT PLAN that puts a node index's shards back into the layout
// `add` fills.  Plain C++ (no HIP): tests/sanitize/remove_rows_check.cpp compiles this header alone under the sanitizers.
#pragma once
#include <stdint.h>

#include <vector>

namespace vodhip {

constexpr int64_t REMOVE_SLAB_ROWS = 65536;  // the default of the parameter "remove_slab_rows"

// "remove_slab_rows" is a power of two >= 4 (one workgroup of the gather kernel moves four rows): a slab is then a whole number of
// count tiles, and a count tile a whole number of slabs' worth of nothing - remove_tile_rows() rows, 256 unless the slab is smaller
inline bool remove_slab_rows_ok(int64_t v) { return v >= 4 && v <= (1ll << 30) && (v & (v - 1)) == 0; }
inline int64_t remove_tile_rows(int64_t slab_rows) { return slab_rows < 256 ? slab_rows : 256; }

// the refusals of a removal that do not depend on the device; `listed` = the call has an id list (row_begin is not read then)
inline const char* remove_rows_args_error(bool listed, int64_t row_begin, int64_t n, int location, int64_t ntotal) {
    if (n < 0) return "n is negative";
    if (location != 0 && location != 1) return "invalid location";
    if (n >= (1ll << 31) - 1) return "n is 2^31 - 1 or more";
    if (!listed && (row_begin < 0 || row_begin > ntotal || n > ntotal - row_begin)) return "row range out of bounds";
    return nullptr;
}

// ---- flat index: the slab plan ----------------------------------------------------------------------------------------------------
// Compaction moves every survivor DOWN, so a row's destination may be the not yet read source of another workgroup: one launch over
// the store would race.  The source rows [first removed row, ntotal) are cut into slabs of `slab_rows`, run in ascending order on one
// stream; a slab is
//   DIRECT   when its destination rows [dst_begin, dst_begin + n_keep) end at or below its first source row: everything the launch
//            writes lies in rows that EARLIER launches consumed, so one gather launch moves source -> destination;
//   BOUNCED  otherwise: one gather launch packs the survivors into the bounce buffer, its contents are then copied to the destination
//            (which ends at or below the slab's last source row: rows this launch or earlier ones consumed).
// A slab without a survivor has no launch.  Rows below the first removed row are in no slab.
struct RemoveSlab {
    int64_t src_begin = 0, src_rows = 0;  // source rows [src_begin, src_begin + src_rows)
    int64_t dst_begin = 0, n_keep = 0;    // its survivors, in order, become rows [dst_begin, dst_begin + n_keep)
    bool bounced = false;
};
struct RemovePlan {
    int64_t survivors = 0;  // the new ntotal
    std::vector<RemoveSlab> slabs;
};
// tile_off [n_tiles + 1]: the exclusive scan of the survivors per count tile; tile t holds rows [tile_base + t * tile_rows, .. + tile_rows)
// cut at ntotal, tile_base a multiple of tile_rows, every row below tile_base survives.  first_removed: the lowest removed row (>= tile_base),
// or >= ntotal when no row is removed.  slab_rows is a multiple of tile_rows.
inline RemovePlan plan_remove_slabs(const int32_t* tile_off, int64_t n_tiles, int64_t tile_base, int64_t tile_rows, int64_t ntotal,
                                    int64_t first_removed, int64_t slab_rows) {
    RemovePlan p;
    p.survivors = tile_base + (n_tiles > 0 ? (int64_t)tile_off[n_tiles] : 0);
    if (first_removed < tile_base || first_removed >= ntotal || n_tiles <= 0) return p;
    const int64_t tiles_per_slab = slab_rows / tile_rows;
    const int64_t t_first = (first_removed - tile_base) / tile_rows;
    for (int64_t ta = t_first; ta < n_tiles; ta += tiles_per_slab) {
        const int64_t tb = ta + tiles_per_slab < n_tiles ? ta + tiles_per_slab : n_tiles;
        RemoveSlab s;
        s.src_begin = tile_base + ta * tile_rows;
        const int64_t src_end = tile_base + tb * tile_rows < ntotal ? tile_base + tb * tile_rows : ntotal;
        s.dst_begin = tile_base + tile_off[ta];
        s.n_keep = (int64_t)tile_off[tb] - tile_off[ta];
        if (ta == t_first) {  // the rows of the first tile below the first removed row stay where they are: not part of the slab
            const int64_t below = first_removed - s.src_begin;
            s.src_begin += below;
            s.dst_begin += below;
            s.n_keep -= below;
        }
        s.src_rows = src_end - s.src_begin;
        s.bounced = s.dst_begin + s.n_keep > s.src_begin;
        if (s.n_keep > 0) p.slabs.push_back(s);
    }
    return p;
}

// ---- node index: the segment plan -------------------------------------------------------------------------------------------------
// After every shard compacted locally, shard g holds keep[g] survivors in rows [0, keep[g]); `add` fills the shards in order, shard g
// owning the global rows [g * rows_per_shard, (g + 1) * rows_per_shard): the survivor of global rank p belongs in shard
// p / rows_per_shard, row p % rows_per_shard.  The segments below, run ONE AFTER THE OTHER in this order, restore that: the ranks
// ascend, a segment's destination lies at or below its source in the global order, so it never covers a row that a later segment
// still reads; only a segment of ONE shard can cover its own source (`overlaps`): that one goes through the shard's bounce buffer.
struct RemoveSegment {
    int src_shard = 0;
    int64_t src_row = 0;
    int dst_shard = 0;
    int64_t dst_row = 0;
    int64_t n = 0;
    bool overlaps = false;
};
struct RemoveSegmentPlan {
    std::vector<RemoveSegment> segments;
    std::vector<int64_t> ntotal;  // [n_shards] rows of every shard afterwards
};
inline RemoveSegmentPlan plan_remove_segments(const int64_t* keep, int n_shards, int64_t rows_per_shard) {
    RemoveSegmentPlan p;
    p.ntotal.assign((size_t)n_shards, 0);
    int64_t rank = 0;
    for (int g = 0; g < n_shards; ++g) {
        int64_t r = 0;
        while (r < keep[g] && rows_per_shard > 0) {
            const int h = (int)(rank / rows_per_shard);
            const int64_t d = rank % rows_per_shard;
            const int64_t n = keep[g] - r < rows_per_shard - d ? keep[g] - r : rows_per_shard - d;  // split at the destination shard's end
            if (h != g || d != r) {
                RemoveSegment s;
                s.src_shard = g, s.src_row = r, s.dst_shard = h, s.dst_row = d, s.n = n;
                s.overlaps = h == g && d + n > r;
                p.segments.push_back(s);
            }
            p.ntotal[(size_t)h] += n;
            r += n;
            rank += n;
        }
    }
    return p;
}

// The dense form of a node call: the part of the global rows [row_begin, row_begin + n) inside shard g, as LOCAL rows [*lo, *hi) of
// that shard; empty (*lo == *hi == 0) when the range misses the shard
inline void split_remove_range(int64_t row_begin, int64_t n, int64_t rows_per_shard, int g, int64_t* lo, int64_t* hi) {
    const int64_t s_lo = (int64_t)g * rows_per_shard, s_hi = s_lo + rows_per_shard;
    const int64_t a = row_begin > s_lo ? row_begin : s_lo, b = row_begin + n < s_hi ? row_begin + n : s_hi;
    *lo = b > a ? a - s_lo : 0;
    *hi = b > a ? b - s_lo : 0;
}

}  // namespace vodhip
