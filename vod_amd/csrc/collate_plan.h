// Host-only plan of the collate-side kernels' LDS (kernels_sample.hip): the dynamic LDS priority_sample_kernel and
// flatten_inbatch_kernel are launched with, and the shapes the one-launch flattening admits.  Plain C++ (no HIP includes), so the
// arithmetic is checked on the CPU for every shape the C ABI admits (tests/test_collate_plan_cpu.py).  The constants the footprints
// depend on live here, next to them: the kernels carve their LDS up with the same ones.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vodhip {

constexpr size_t CL_LDS_LIMIT = 160 * 1024;  // LDS of one gfx950 workgroup
constexpr size_t CL_LDS_SLACK = 16;

// ---- priority_sample_kernel: one workgroup per query row ----
constexpr int SM_THREADS = 256;
constexpr int SM_MAX_WIDTH = 4096;    // candidates per row (the C ABI refuses more)
constexpr int SM_MAX_K_TOTAL = 4096;  // samples per row (the C ABI refuses more)

// capacity of the kernel's sort buffer: the power of two >= the widest row, at least one key per thread
constexpr int sample_sort_capacity(int max_width) {
    int P = SM_THREADS;
    while (P < max_width) P <<= 1;
    return P;
}

// bytes of the kernel's carve-up for a sort buffer of P keys and k_total samples per row:
//   keys [P] u64, lp [P] f32, wsel [k_total] f32, isel [k_total] i32, sel_all [k_total] i32, order [P] i32, red [waves] f32, red_i [16] i32
//   and, when a proposal output is asked for, mass_s [2] f32, wall [k_total] f32
constexpr size_t sample_lds_bytes(int P, int k_total, bool proposal) {
    return (size_t)P * (8 + 4 + 4) + (size_t)k_total * (4 + 4 + 4) + (size_t)(SM_THREADS / 64) * 4 + 16 * 4 + CL_LDS_SLACK +
           (proposal ? 2 * 4 + (size_t)k_total * 4 : 0);
}

static_assert(sample_lds_bytes(sample_sort_capacity(SM_MAX_WIDTH), SM_MAX_K_TOTAL, true) <= CL_LDS_LIMIT,
              "the widest row with the most samples must fit one workgroup's LDS");

// ---- flatten_inbatch_kernel: one workgroup per row, each sorts the ids of the whole batch ----
constexpr int FL_THREADS = 1024;  // 16 wavefronts: the sort network is a latency chain per stage, so wide and shallow (2 keys per thread at U = 2048)
constexpr int FL_MAX_IDS = 8192;   // U = n_rows * n_keys: the largest sort
constexpr int FL_MAX_KEYS = 1024;  // ids per row staged in LDS
constexpr int FL_MAX_VALUES = 8;   // value arrays per launch; `vals` is carved for all of them whatever the launch carries

struct FlattenPlan {
    int U;       // ids in the batch
    int P;       // keys sorted: the power of two >= U, at least one per thread
    size_t lds;  // dynamic LDS of the launch in bytes
};

// bytes of the kernel's carve-up:
//   srt [P] i64, uq [U] i64, vals [FL_MAX_VALUES][n_keys] f32, lab [n_keys rounded up to 4] u8, s_w [waves] i32
constexpr size_t flatten_lds_bytes(int U, int P, int n_keys) {
    return (size_t)P * 8 + (size_t)U * 8 + (size_t)n_keys * FL_MAX_VALUES * 4 + (size_t)((n_keys + 3) & ~3) + (size_t)(FL_THREADS / 64) * 4 +
           CL_LDS_SLACK;
}

// n_rows * n_keys <= FL_MAX_IDS
constexpr FlattenPlan flatten_plan(int64_t n_rows, int n_keys) {
    const int U = (int)(n_rows * n_keys);
    int P = FL_THREADS;
    while (P < U) P <<= 1;
    return FlattenPlan{U, P, flatten_lds_bytes(U, P, n_keys)};
}

// The shapes the one-launch flattening takes: at most FL_MAX_IDS ids, FL_MAX_KEYS per row, and a footprint inside one workgroup's
// LDS.  Of the shapes within the first two bounds the third excludes exactly 8 rows x 1013 ... 1024 ids (163,880 ... 164,944 B;
// 8 x 1012 takes 163,780 B and 7 x 1024 156,752 B): those go through vodhip_gather_by_id.
constexpr bool flatten_admits(int64_t n_rows, int64_t n_keys) {
    return n_rows >= 0 && n_keys >= 0 && n_keys <= FL_MAX_KEYS && (n_keys == 0 || n_rows <= FL_MAX_IDS / n_keys) &&
           flatten_plan(n_rows, (int)n_keys).lds <= CL_LDS_LIMIT;
}

static_assert(flatten_admits(8, 1012) && !flatten_admits(8, 1013) && !flatten_admits(8, 1024) && flatten_admits(7, 1024) && flatten_admits(1, 1024),
              "the admitted region ends where the footprint passes one workgroup's LDS");

}  // namespace vodhip
