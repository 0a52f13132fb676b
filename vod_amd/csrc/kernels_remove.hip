// Removal of stored rows with the gaps closed in place (include/vodhip.h H2r): a STABLE compaction, survivors keep their order and
// move down.  Nothing is computed: rows are moved whole, every plane of a row in the same launch, so what `add` wrote for a row is
// what the row still holds at its new place.  Four steps, all on the call's stream (the host side: vodhip_index_remove_rows):
//   MARK    the int32 owner word per capacity row that update_rows keeps (zero between calls) is set for every row that leaves: one
//           thread per slot of a list (atomicExch: a second slot of a row finds the word set and counts itself a duplicate; a slot
//           whose id is outside the store counts itself skipped), or a plain store per row of a range;
//   COUNT   survivors per count tile (T = remove_tile_rows() <= 256 rows) from ballots, then ONE workgroup scans the tile counts:
//           integers, the same words on every repeat; no workgroup ever waits for another one - the launch boundary is the only
//           synchronisation;
//   MOVE    remove_gather_kernel, once per slab of the host's plan (remove_fold.h): one wavefront per SOURCE row, four rows per
//           256-thread workgroup, 16-byte loads and stores (32 bytes of the float32 plane per lane and step).  A survivor's new row is
//           tile_off[its tile] + its rank inside the tile, the rank from ballots over the tile's owner words below it.  The
//           destination planes are the store's own (a DIRECT slab) or the bounce buffer's (a BOUNCED one);
//   FINISH  new_ids when asked for (remove_map_kernel, before the owner words are cleared).
// The hazard the slabs exist for is stated in remove_fold.h.  Every access is bounded by ntotal (source rows) or by the slab's
// survivor count (destination rows): a destination row is below its source row.
#include "mips_common.h"
#include "remove_fold.h"

namespace vodhip {

namespace {

__global__ __launch_bounds__(256) void remove_mark_listed_kernel(const int64_t* __restrict__ ids, int64_t n, int64_t id_base, int64_t ntotal,
                                                                 int* __restrict__ owner, unsigned int* __restrict__ words) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t id = ids[j], row = id - id_base;
    if (id < 0 || row < 0 || row >= ntotal) {
        atomicAdd(words + RMW_SKIPPED, 1u);
        return;
    }
    if (atomicExch(owner + row, 1) != 0) atomicAdd(words + RMW_DUPLICATES, 1u);
}

__global__ __launch_bounds__(256) void remove_mark_range_kernel(int64_t row_begin, int64_t n, int* __restrict__ owner) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) owner[row_begin + j] = 1;
}

// one workgroup per 256 rows from tile_base: 256 / tile_rows count tiles; the lowest removed row -> words[RMW_FIRST] (atomicMin, one
// per wavefront that holds a removed row)
__global__ __launch_bounds__(256) void remove_count_kernel(const int* __restrict__ owner, int64_t tile_base, int tile_rows, int64_t ntotal,
                                                           int64_t n_tiles, int* __restrict__ tile_cnt, unsigned int* __restrict__ words) {
    __shared__ int cnt[64];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 64) cnt[tid] = 0;
    __syncthreads();
    const int64_t row = tile_base + (int64_t)blockIdx.x * 256 + tid;
    const bool in = row < ntotal;
    const bool removed = in && owner[row] != 0;
    const unsigned long long bk = __ballot(in && !removed), br = __ballot(removed);
    const int g = tile_rows < 64 ? tile_rows : 64;  // lanes of one tile inside a wavefront
    if (lane % g == 0) {
        const unsigned long long m = (g == 64 ? ~0ull : ((1ull << g) - 1ull)) << lane;
        atomicAdd(&cnt[tid / tile_rows], __popcll(bk & m));
    }
    if (lane == 0 && br != 0ull) atomicMin(words + RMW_FIRST, (unsigned int)(row + (__ffsll((long long)br) - 1)));
    __syncthreads();
    const int tiles_here = 256 / tile_rows;
    const int64_t t = (int64_t)blockIdx.x * tiles_here + tid;
    if (tid < tiles_here && t < n_tiles) tile_cnt[t] = cnt[tid];
}

// exclusive scan of the tile counts by ONE workgroup, 1024 tiles a step with the running total carried in a register
__global__ __launch_bounds__(1024) void remove_scan_kernel(const int* __restrict__ tile_cnt, int64_t n_tiles, int* __restrict__ tile_off) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int64_t base = 0; base < n_tiles; base += 1024) {
        const int64_t i = base + tid;
        const int v = i < n_tiles ? tile_cnt[i] : 0;
        int x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? wsum[w] : 0;
            total += wsum[w];
        }
        if (i < n_tiles) tile_off[i] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) tile_off[n_tiles] = carry;
}

template <bool EXACT, bool LABEL, bool VALUE>
__global__ __launch_bounds__(256) void remove_gather_kernel(const RemoveGatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t local = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (local >= a.src_rows) return;  // (wave-uniform, as every branch below)
    const int64_t row = a.src_begin + local;
    if (a.owner[row] != 0) return;  // the row leaves
    const int64_t t = (row - a.tile_base) / a.tile_rows, t0 = a.tile_base + t * a.tile_rows;
    const int within = (int)(row - t0);
    int rank = 0;  // survivors of the tile below this row
    for (int k = 0; k < within; k += 64) {
        const int i = k + lane;
        rank += __popcll(__ballot(i < within && a.owner[t0 + i] == 0));
    }
    const int64_t dst = a.tile_base + a.tile_off[t] + rank - a.dst_sub;
    {
        const uint4* __restrict__ s = reinterpret_cast<const uint4*>(a.src.data + row * a.stride);
        uint4* __restrict__ d = reinterpret_cast<uint4*>(a.dst.data + dst * a.stride);
        for (int64_t c = lane; c < a.stride / 8; c += 64) d[c] = s[c];
    }
    if constexpr (EXACT) {
        const float4* __restrict__ s = reinterpret_cast<const float4*>(a.src.data32 + row * a.stride);
        float4* __restrict__ d = reinterpret_cast<float4*>(a.dst.data32 + dst * a.stride);
        for (int64_t c = lane; c < a.stride / 8; c += 64) {
            const float4 lo = s[2 * c], hi = s[2 * c + 1];
            d[2 * c] = lo;
            d[2 * c + 1] = hi;
        }
        if (lane == 0) {
            a.dst.row_n2[dst] = a.src.row_n2[row];
            a.dst.row_d2[dst] = a.src.row_d2[row];
        }
    }
    if constexpr (LABEL) {
        if (lane == 0) a.dst.label[dst] = a.src.label[row];
    }
    if constexpr (VALUE) {
        const uint4* __restrict__ s = reinterpret_cast<const uint4*>(a.src.value + row * a.c_pad);
        uint4* __restrict__ d = reinterpret_cast<uint4*>(a.dst.value + dst * a.c_pad);
        for (int64_t c = lane; c < a.c_pad / 8; c += 64) d[c] = s[c];
    }
}

// new_ids[row] = the row's new id, -1 for a removed one; one workgroup per 256 rows from row 0 (tile_base is a multiple of tile_rows,
// tile_rows divides 256: a tile never straddles a workgroup)
__global__ __launch_bounds__(256) void remove_map_kernel(const int* __restrict__ owner, const int* __restrict__ tile_off, int64_t tile_base,
                                                         int tile_rows, int64_t ntotal, int64_t* __restrict__ new_ids) {
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)blockIdx.x * 256 + tid;
    const bool in = row < ntotal;
    const bool removed = in && row >= tile_base && owner[row] != 0;
    const unsigned long long bk = __ballot(in && !removed);
    if (lane == 0) wcnt[wave] = __popcll(bk);
    __syncthreads();
    if (!in) return;
    if (row < tile_base) {
        new_ids[row] = row;
        return;
    }
    const int g = tile_rows < 64 ? tile_rows : 64;
    const int g_lo = lane - lane % g;
    int rank = __popcll(bk & ((1ull << lane) - 1ull) & ~((1ull << g_lo) - 1ull));
    if (tile_rows > 64) {
        const int per = tile_rows / 64;
        for (int w = wave - wave % per; w < wave; ++w) rank += wcnt[w];
    }
    new_ids[row] = removed ? -1 : tile_base + tile_off[(row - tile_base) / tile_rows] + rank;
}

}  // namespace

hipError_t launch_remove_mark(const int64_t* ids, int64_t row_begin, int64_t n, int64_t id_base, int64_t ntotal, int* owner, unsigned int* words,
                              hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (!owner || !words || n < 0 || n >= (1ll << 31) - 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (ids) {
        hipLaunchKernelGGL(remove_mark_listed_kernel, grid, dim3(256), 0, stream, ids, n, id_base, ntotal, owner, words);
    } else {
        if (row_begin < 0 || row_begin + n > ntotal) return hipErrorInvalidValue;
        hipLaunchKernelGGL(remove_mark_range_kernel, grid, dim3(256), 0, stream, row_begin, n, owner);
    }
    return hipGetLastError();
}

hipError_t launch_remove_count_scan(const int* owner, int64_t tile_base, int64_t tile_rows, int64_t ntotal, int64_t n_tiles, int* tile_cnt, int* tile_off,
                                    unsigned int* words, hipStream_t stream) {
    if (n_tiles <= 0) return hipSuccess;
    if (!owner || !tile_cnt || !tile_off || !words || tile_rows < 4 || tile_rows > 256 || 256 % tile_rows != 0 || tile_base < 0 || tile_base % tile_rows != 0 ||
        n_tiles != (ntotal - tile_base + tile_rows - 1) / tile_rows)
        return hipErrorInvalidValue;
    const int64_t blocks = (ntotal - tile_base + 255) / 256;
    hipLaunchKernelGGL(remove_count_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, owner, tile_base, (int)tile_rows, ntotal, n_tiles, tile_cnt, words);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(remove_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_cnt, n_tiles, tile_off);
    return hipGetLastError();
}

hipError_t launch_remove_gather(const RemoveGatherArgs& a, hipStream_t stream) {
    if (a.src_rows == 0) return hipSuccess;
    if (!a.owner || !a.tile_off || !a.src.data || !a.dst.data || a.stride <= 0 || a.stride % 64 != 0 || a.tile_rows < 4 || a.src_begin < a.tile_base ||
        a.src_rows < 0 || a.src_begin + a.src_rows > a.ntotal || a.src_rows > 4ll * 0x7fffffff)
        return hipErrorInvalidValue;
    const bool exact = a.src.data32 != nullptr, label = a.src.label != nullptr, value = a.src.value != nullptr;
    if (exact && (!a.dst.data32 || !a.src.row_n2 || !a.src.row_d2 || !a.dst.row_n2 || !a.dst.row_d2)) return hipErrorInvalidValue;
    if ((label && !a.dst.label) || (value && (!a.dst.value || a.c_pad <= 0 || a.c_pad % 64 != 0))) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.src_rows + 3) / 4));
#define VOD_RM(E, L, V)                                                                                              \
    if (exact == E && label == L && value == V) {                                                                    \
        hipLaunchKernelGGL((remove_gather_kernel<E, L, V>), grid, dim3(256), 0, stream, a);                         \
        return hipGetLastError();                                                                                    \
    }
    VOD_RM(false, false, false) VOD_RM(false, false, true) VOD_RM(false, true, false) VOD_RM(false, true, true)
    VOD_RM(true, false, false) VOD_RM(true, false, true) VOD_RM(true, true, false) VOD_RM(true, true, true)
#undef VOD_RM
    return hipErrorInvalidValue;
}

hipError_t launch_remove_map(const int* owner, const int* tile_off, int64_t tile_base, int64_t tile_rows, int64_t ntotal, int64_t* new_ids, hipStream_t stream) {
    if (ntotal <= 0) return hipSuccess;
    if (!owner || !tile_off || !new_ids || tile_rows < 4 || 256 % tile_rows != 0 || tile_base % tile_rows != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(remove_map_kernel, dim3((unsigned)((ntotal + 255) / 256)), dim3(256), 0, stream, owner, tile_off, tile_base, (int)tile_rows, ntotal, new_ids);
    return hipGetLastError();
}

}  // namespace vodhip
