// Host-only plan of merge_hybrid_kernel's LDS: the size of its open-addressing table and the dynamic LDS the launch asks for.
// Plain C++ (no HIP includes), so the rule is checked on the CPU for every width (tests/test_hybrid_plan_cpu.py).  The constants
// the footprint depends on live here, next to it: the kernel (kernels_hybrid.hip) carves its LDS up with the same ones.
#pragma once
#include <cstddef>

namespace vodhip {

constexpr int HY_THREADS = 512;  // 8 wavefronts: one entry per thread up to W = 512 (the probes are latency chains: width beats depth)
constexpr int HY_WAVES = HY_THREADS / 64;
constexpr int HY_MAX_WIDTH = 4096;               // lookup + every engine, entries per row (the C ABI refuses more)
constexpr size_t HY_LDS_CAP = 150 * 1024;        // what a 1/4-loaded table may cost; a 1/2-loaded one may go past it (below)
constexpr size_t HY_LDS_LIMIT = 160 * 1024;      // LDS of one gfx950 workgroup
constexpr size_t HY_LDS_SLACK = 16;

struct HybridPlan {
    int T;       // table slots, a power of two
    size_t lds;  // dynamic LDS of the launch in bytes
};

// bytes of the kernel's carve-up for a row of W entries and a table of T slots:
//   ids [W] i64, table [T] u64, wsc [W] f32, nsc [W] f32, pre [W + 1] i32, s_min [HY_WAVES][4] f32, s_misc [HY_WAVES + 1] i32, multi [T] u8
constexpr size_t hybrid_lds_bytes(int W, int T) {
    return (size_t)W * (8 + 4 + 4) + (size_t)(W + 1) * 4 + (size_t)HY_WAVES * 4 * 4 + (size_t)(HY_WAVES + 1) * 4 + (size_t)T * (8 + 1) +
           HY_LDS_SLACK;
}

// T >= 64.  Load factor <= 1/4 (T >= 4 W: short probe chains - a wavefront waits for its longest one) wherever that table fits
// HY_LDS_CAP, and never above 1/2 (T >= 2 W): the table is halved only while the HALVED table still has 2 W slots.  For every
// W <= HY_MAX_WIDTH the result fits HY_LDS_LIMIT: the largest footprint is 155,832 B at W = 4096 (T = 8192), above HY_LDS_CAP,
// which therefore bounds the 1/4-loaded table only.
constexpr HybridPlan hybrid_plan(int W) {
    int T = 64;
    while (T < 4 * W) T <<= 1;
    while (hybrid_lds_bytes(W, T) > HY_LDS_CAP && T / 2 >= 2 * W && T / 2 >= 64) T >>= 1;
    return HybridPlan{T, hybrid_lds_bytes(W, T)};
}

static_assert(hybrid_plan(HY_MAX_WIDTH).T >= 2 * HY_MAX_WIDTH && hybrid_plan(HY_MAX_WIDTH).lds <= HY_LDS_LIMIT, "the widest row must fit one workgroup's LDS");

}  // namespace vodhip
