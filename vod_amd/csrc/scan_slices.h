// How the whole-store scans cut a query batch into slices (host code only, no HIP: tests/test_scan_slices_cpu.py compiles it alone).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

namespace vodhip {

constexpr int64_t SCAN_SLICE_MIN = 64;    // the 64-query instantiation of the scan kernels
constexpr int64_t SCAN_SLICE_MAX = 1024;  // queries per launch
constexpr int64_t SCAN_SLICE_STEP = 128;  // the query tile

// queries per slice of a batch: a multiple of 128 (or 64) up to 1024 that keeps temporaries of per_query bytes each under `budget`
// bytes (VODHIP_POSTERIOR_TEMP_BYTES, or the index's "scan_temp_bytes") unless a 64-query slice alone needs more
inline int64_t scan_slice_queries(int64_t budget, size_t per_query) {
    const int64_t slice = (int64_t)((size_t)budget / per_query) / SCAN_SLICE_STEP * SCAN_SLICE_STEP;
    return std::min<int64_t>(SCAN_SLICE_MAX, std::max<int64_t>(SCAN_SLICE_MIN, slice));
}

}  // namespace vodhip
