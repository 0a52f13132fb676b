// The planner of a search: which stages it runs and which filter kernel launches each one.  Host-only: search_plan.cpp is compiled by the
// host compiler (see the Makefile), so the planner makes no device and no HIP runtime call, and vodhip_debug_schedule checks on a CPU the
// very plan a search issues.
#pragma once
#include <stdint.h>

#include <vector>

namespace vodhip {

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

constexpr int64_t ROW_ALIGN = 256;  // largest tile height; chunk boundaries and capacity padding
constexpr int64_t MAX_NQ_PER_PASS = 2048;
constexpr int64_t MAX_SURVIVOR_RING = 8192;       // records per wave a caller may force (vodhip_index_set_param "survivor_ring")
constexpr int64_t MAX_AUTO_SURVIVOR_RING = 1024;  // ... and the planner's own sizes stop at: 8 x 256 waves x 1024 x 132 B = 277 MB per lane

// The production filter kernels.  The values are the public "tile" ids (vodhip_index_set_param, bench.py --tile).
enum class FilterKernel : int { Generic128 = 1, Generic256x64 = 42, Generic256x128 = 46, Persistent = 8, Staggered = 9, EightPhase = 14 };

struct FilterGeometry {
    FilterKernel kernel;
    int rows, cols;   // BM x BN: store rows x queries per workgroup tile (nq_pad is a multiple of BN)
    int group_rows;   // rows per GMAX group (one lane's rows of one column block)
    bool persistent;  // one workgroup per CU walking the tiles
};
constexpr FilterGeometry FILTER_KERNELS[] = {
    {FilterKernel::Generic128, 128, 128, 16, false},      // kernels_mips.hip; 64 KB LDS, 2 workgroups / CU: short and dense stages
    {FilterKernel::Generic256x64, 256, 64, 16, false},    // 3-slot ring: batches of <= 64 queries (HBM-bound)
    {FilterKernel::Generic256x128, 256, 128, 16, false},  // 3-slot ring: 65..128 queries
    {FilterKernel::Persistent, 256, 256, 32, true},       // both waves of a SIMD in lockstep
    {FilterKernel::Staggered, 256, 256, 32, true},        // waves 4..7 staggered by one k-step
    {FilterKernel::EightPhase, 256, 256, 32, true},       // kernels_mips_8phase.hip: the 8-phase K loop, FILTER stages only
};
constexpr const FilterGeometry* find_kernel(int64_t id) {  // nullptr: `id` names no production kernel
    for (const FilterGeometry& g : FILTER_KERNELS)
        if ((int64_t)g.kernel == id) return &g;
    return nullptr;
}
constexpr const FilterGeometry& geometry(FilterKernel f) { return *find_kernel((int64_t)f); }

// A search is a list of stages, each one filter launch + one select launch:
//   GMAX    threshold bootstrap.  S sampled rows (8-row groups spread evenly over the whole store) are scored and every
//           lane writes the maximum of its group of 16 / 32 rows; the k-th largest group maximum is a lower bound of the
//           k-th best score (k distinct rows reach it) however the rows are ordered.  Emits no candidates.
//   FILTER  rows [b, e) filtered against the running threshold; survivors -> candidate lists -> running top-k.
//           Stage i covers `growth` x the rows the threshold was calibrated on, so it emits ~ growth * k survivors per
//           query for exchangeable row order, and never more than the GMAX bound allows (~ k * rows / S) for any order.
//   DENSE   every score of <= cap rows becomes a candidate (indexes of a few thousand rows; the exhaustive fallback).
enum : int { ST_FILTER = 0, ST_DENSE = 1, ST_GMAX = 2 };
struct Stage {
    int kind;
    int64_t b, e;        // rows (FILTER / DENSE)
    int64_t n_tiles;     // sampled tiles (GMAX)
    int64_t rstride;     // store rows between consecutive sampled rows (GMAX)
    int64_t n_groups;    // lane groups of the sample = candidate slots per query (GMAX)
    FilterKernel kernel = FilterKernel::Persistent;  // what launches it (SearchPlan::kernel: short FILTER stages of a small pass may not)
    int64_t sample_offset = 0;  // GMAX: first sampled row
};

// The index's tunables the planner reads (vodhip_index_set_param)
struct PlanTunables {
    int64_t cand_cap = 16384;
    int64_t dense_rows = 2048;   // indexes up to this many rows are scored densely in one launch
    int64_t growth_x100 = 0;     // FILTER stage = growth x the rows its threshold was calibrated on; 0 = auto (8; 3 for batches above 512 queries on stores of 4 M rows and more)
    int64_t sample_div = 0;      // GMAX bootstrap scores ~ ntotal / sample_div sampled rows; 0 = auto (96; 192 where growth is 3)
    int64_t tile = 0;            // the requested kernel: 0 = auto (by nq), else a FilterKernel id (find_kernel)
    int64_t tile_order = 0;      // 0 = FILTER stages walk the store's super-tiles in a low-discrepancy order (default); 1 = in row order
    int64_t small_chunk_tiles = 256;  // launches with fewer 256x256 tiles than this (less than one per CU) use the 128x128 kernel
    int64_t survivor_ring = 0;   // survivor records per wave of the 8-phase kernel's rings: 0 = auto (survivor_ring_records), n = n
    int n_cu = 256;              // compute units of the device
};

// At most MAX_NQ_PER_PASS queries go through the stages at once: a search of more runs them once per pass of queries, each padded to bn.
struct SearchPlan {
    int64_t bn = 256;         // nq_pad granularity
    bool corpus_nt = false;   // FILTER_FLAG_CORPUS_NT
    int64_t perm_mul = 0, perm_mod = 0;  // FilterExtra: the stage order (0: row order)
    int64_t small_tiles = 0;  // FILTER stages of fewer 256x256 tiles than this on a pass run on the 128x128 kernel (less than one per CU)
    std::vector<Stage> stages;
    int64_t ring = 0;         // survivor records per wave of the 8-phase FILTER launches (0: no stage runs that kernel)
    FilterKernel kernel(const Stage& sg, int64_t nq_pad) const {  // the kernel of stage `sg` on a pass of nq_pad queries
        return sg.kind == ST_FILTER && (sg.e - sg.b + 255) / 256 * (nq_pad / 256) < small_tiles ? FilterKernel::Generic128 : sg.kernel;
    }
};

// recovery > 0: pass number after a candidate-list overflow; safe: exhaustive DENSE stages only; subset: a subset filter is in force
SearchPlan plan_search(int64_t ntotal, int k, int64_t nq, const PlanTunables& t, bool subset, bool safe, int recovery);

// Survivor records per wave the rings of the 8-phase FILTER kernel (kernels_mips_8phase.hip) are sized for: `per_query` expected
// survivors per query in a stage, shared by the waves of the persistent grid that see the query (two wave rows per workgroup of its
// query tile), twice that plus one record per lane, in whole 64-record steps, at most MAX_AUTO_SURVIVOR_RING (large k, many query
// tiles: the blocks that do not fit take the in-loop path).
int64_t survivor_ring_records(double per_query, int64_t nq_pad, int n_cu);

// The multiplier of the low-discrepancy stage order over T super-tiles (FilterExtra::perm_mul); <= 1: no permutation.
int64_t tile_order_multiplier(int64_t T);

}  // namespace vodhip
