// Scoring of LISTED rows: out[q, j] = <query q, row ids[q, j]> for a per-query list of section ids, and the top-k over such a list.
//
// The reference's SearchClient.search carries `ids`; its Elasticsearch client honours it with a `terms` filter on the section id - only
// the listed sections can be hits - and returns labels = scores > -inf (/root/reference/src/vod_search/es_search/client.py:145,177-183),
// while its faiss client drops the argument (faiss_search/client.py:70).  This is the dense engine's counterpart: the gold-section
// lookup of the hybrid search (core/search.py:42-50) and any re-scoring of known rows without a scan of the store.
//
// The work is a gather of whole rows (dim_pad x 2 bytes each) and one dot product per row: no MFMA - every row meets ONE query.
// Shape of the gather (MI355X_MICROARCH "Indexed rows"): a wave owns one (query, run of slots), keeps 4 rows in flight, loads 16 bytes
// per lane; 4 waves per workgroup share the query in LDS, 4 workgroups per CU.
//
// ONE summation order per (query, row), whatever the slot, m, nq or the grid: lane l takes columns 8l .. 8l+7 of every 512-column pass
// in increasing pass order, column c of them goes to accumulator c mod 4 with one fma; the four accumulators add as (0 + 1) + (2 + 3),
// the 64 lane sums by the fixed butterfly of exact_dot.h.  VODHIP_EXACT_F32 stores score from the float32 plane with the unrounded query
// through exact_dot: the bits a search returns for the pair.
//
// The WEIGHTED SUM of listed rows, out[q, :] = sum_j w[q, j] * row(ids[q, j]) - the backward of the scores with respect to the query -
// is the same gather with the roles turned: rows and weights are wave-uniform, lane l keeps columns 8l .. 8l+7 of every 512-column pass
// in registers and nothing crosses lanes (sum_listed_kernel below states its summation order).
#include "exact_dot.h"
#include "mips_common.h"
#include "wg_sort.h"

namespace vodhip {

namespace {

constexpr int LT = 256;        // threads of a scoring workgroup: 4 waves, one run of slots each
constexpr int LW = LT / 64;
constexpr int LR = 4;          // rows a wave has in flight
constexpr int ST = 1024;       // threads of the select workgroup
// the weighted sum.  SC is a CONSTANT (the forward adapts its slots per workgroup to the batch: it may, a score does not depend on it; a
// sum's order does): 32 slots = two groups of LR rows per wave, 13 workgroups per query at m = 385 - 64 queries are 832 workgroups
constexpr int SC = 32;         // slots of a sum workgroup
constexpr int SW = SC / LW;    // ... of one of its waves
constexpr int SP = 4;          // 512-column passes of a column block at most: 32 accumulators per lane
constexpr int SB = SP * 512;   // columns of a column block; wider stores take more column blocks in the grid

// the local row of a listed id, or -1: empty (id < 0), out of range (rows >= ntotal hold stale data after a reset), or not among the
// query's subset labels (the rule of vodhip_index_set_query_labels: all -1 = unrestricted)
__device__ __forceinline__ int listed_row(int64_t id, const ListedArgs& a, int64_t q) {
    const int64_t local = id - a.id_base;
    bool present = id >= 0 && local >= 0 && local < a.ntotal;
    if (present && a.q_label != nullptr) {
        const int lab = a.row_label[local];
        int any = 0, ok = 0;
        for (int s = 0; s < a.n_qlab; ++s) {
            const int ql = a.q_label[(size_t)q * a.n_qlab + s];
            any |= (ql != -1) ? 1 : 0;
            ok |= (ql == lab) ? 1 : 0;
        }
        present = ok != 0 || any == 0;
    }
    return present ? (int)local : -1;
}

template <int DT>
__device__ __forceinline__ float half_to_f32(uint16_t h) {
    if constexpr (DT == 0) return (float)__builtin_bit_cast(_Float16, h);
    else return (float)__builtin_bit_cast(__bf16, h);
}

// LR rows of the fp16 / bf16 plane against the rounded query in LDS (the fixed order described at the top of the file)
template <int DT>
__device__ __forceinline__ void listed_dot(const uint16_t* __restrict__ plane, int64_t stride, const int (&rows)[LR], const uint16_t* qs,
                                           int dim_pad, int lane, float (&out)[LR]) {
    float acc[LR][4];
#pragma unroll
    for (int n = 0; n < LR; ++n) acc[n][0] = acc[n][1] = acc[n][2] = acc[n][3] = 0.f;
    for (int c = lane * 8; c < dim_pad; c += 512) {
        uint4 xv[LR];
#pragma unroll
        for (int n = 0; n < LR; ++n)
            xv[n] = rows[n] >= 0 ? *reinterpret_cast<const uint4*>(plane + (size_t)rows[n] * stride + c) : make_uint4(0u, 0u, 0u, 0u);
        const uint4 qv = *reinterpret_cast<const uint4*>(qs + c);
        const uint16_t* qh = reinterpret_cast<const uint16_t*>(&qv);
        float qf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = half_to_f32<DT>(qh[e]);
#pragma unroll
        for (int n = 0; n < LR; ++n) {
            const uint16_t* xh = reinterpret_cast<const uint16_t*>(&xv[n]);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[n][e & 3] = __builtin_fmaf(half_to_f32<DT>(xh[e]), qf[e], acc[n][e & 3]);
        }
    }
#pragma unroll
    for (int n = 0; n < LR; ++n) out[n] = wave_sum_fixed((acc[n][0] + acc[n][1]) + (acc[n][2] + acc[n][3]));
}

// MODE 0 / 1: fp16 / bf16 plane, the query rounded to the store dtype as mips_prepare_kernel rounds it (saturating); MODE 2: the float32
// plane of an exact store, the query as given.  Workgroup b scores slots [chunk * spb, (chunk + 1) * spb) of query b / chunks.
template <int MODE>
__global__ __launch_bounds__(LT) void score_listed_kernel(ListedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = (int64_t)blockIdx.x / a.chunks;
    const int64_t slot0 = ((int64_t)blockIdx.x % a.chunks) * a.spb;

    for (int c = tid; c < a.dim_pad; c += LT) {
        float f = 0.f;
        if (c < a.dim) {
            if (a.q_dtype == 2) f = ((const float*)a.q_src)[q * a.dim + c];
            else if (a.q_dtype == 0) f = (float)(((const _Float16*)a.q_src)[q * a.dim + c]);
            else f = (float)(((const __bf16*)a.q_src)[q * a.dim + c]);
        }
        if constexpr (MODE == 2) {
            reinterpret_cast<float*>(smem)[c] = f;
        } else {
            float rounded;
            reinterpret_cast<uint16_t*>(smem)[c] = store_bits(f, MODE, &rounded);
        }
    }
    __syncthreads();

    // the wave's run of slots: their rows in ONE coalesced pass (a lane per slot), then LR rows at a time
    const int per_wave = a.spb / LW;  // <= 64
    const int64_t w0 = slot0 + (int64_t)wave * per_wave;
    int my_row = -1;
    if (lane < per_wave && w0 + lane < a.m) my_row = listed_row(a.ids[q * a.m + w0 + lane], a, q);
    for (int j0 = 0; j0 < per_wave && w0 + j0 < a.m; j0 += LR) {
        int rows[LR];
#pragma unroll
        for (int n = 0; n < LR; ++n) rows[n] = __builtin_amdgcn_readfirstlane(__shfl(my_row, j0 + n, 64));
        float s[LR];
        if constexpr (MODE == 2) {
            const float* qs = reinterpret_cast<const float*>(smem);
            const float* plane = reinterpret_cast<const float*>(a.plane);
            switch ((a.dim_pad + 255) >> 8) {
                case 1: exact_dot_preload<LR, 1>(plane, a.stride, rows, qs, a.dim_pad, lane, s); break;
                case 2: exact_dot_preload<LR, 2>(plane, a.stride, rows, qs, a.dim_pad, lane, s); break;
                case 3: exact_dot_preload<LR, 3>(plane, a.stride, rows, qs, a.dim_pad, lane, s); break;
                case 4: exact_dot_preload<LR, 4>(plane, a.stride, rows, qs, a.dim_pad, lane, s); break;
                default: exact_dot<LR>(plane, a.stride, rows, qs, a.dim_pad, lane, s); break;
            }
        } else {
            listed_dot<MODE>(reinterpret_cast<const uint16_t*>(a.plane), a.stride, rows, reinterpret_cast<const uint16_t*>(smem), a.dim_pad, lane, s);
        }
        if (lane == 0) {
#pragma unroll
            for (int n = 0; n < LR; ++n)
                if (j0 + n < per_wave && w0 + j0 + n < a.m) a.out[q * a.m + w0 + j0 + n] = rows[n] >= 0 ? s[n] : -__builtin_inff();  // (a computed NaN leaves as computed)
        }
    }
}

// The weighted sum of listed rows.  Workgroup (x, y) owns slots [chunk * SC, (chunk + 1) * SC) of query x / chunks and columns
// [y * SB, y * SB + P * 512); wave w of it owns the SW slots from chunk * SC + w * SW.  A lane per slot resolves (row, weight) in one
// coalesced pass; a slot that is absent (listed_row) or whose weight is 0.0 becomes (-1, 0): its row is not read, and what it adds is
// fma(0, 0, acc) - whatever the weight was, NaN and inf included.  A NaN weight is not 0: it stays.
// ONE summation order per (query, column), whatever nq, the query's place in the batch or the launch: the slots of a wave's run in
// increasing order, one fma(x, w, acc) each, from acc = 0; the four runs of a chunk as ((0 + 1) + 2) + 3; the chunks in increasing
// order (fold_listed_sum_kernel).  MODE 0 / 1: fp16 / bf16 plane, widened exactly; MODE 2: the float32 plane of an exact store.
template <int MODE, int P>
__global__ __launch_bounds__(LT) void sum_listed_kernel(ListedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* fold = reinterpret_cast<float*>(smem);  // [LW][P * 512]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = (int64_t)blockIdx.x / a.chunks, chunk = (int64_t)blockIdx.x % a.chunks;
    const int col0 = (int)blockIdx.y * SB;

    const int64_t slot = chunk * SC + wave * SW + lane;
    int my_row = -1;
    float my_w = 0.f;
    if (lane < SW && slot < a.m) {
        const int row = listed_row(a.ids[q * a.m + slot], a, q);
        const float w = a.weights[q * a.m + slot];
        if (row >= 0 && w != 0.f) {
            my_row = row;
            my_w = w;
        }
    }

    float acc[P][8];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[p][e] = 0.f;
#pragma unroll 1
    for (int j0 = 0; j0 < SW; j0 += LR) {
        int rows[LR];
        float w[LR];
#pragma unroll
        for (int n = 0; n < LR; ++n) {
            rows[n] = __builtin_amdgcn_readlane(my_row, j0 + n);
            w[n] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_w), j0 + n));
        }
        if ((rows[0] & rows[1] & rows[2] & rows[3]) < 0) continue;  // (all four negative; wave-uniform)
        static_assert(LR == 4, "the test above names four rows");
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int c = col0 + p * 512 + lane * 8;
            const bool in = c < a.dim_pad;
            if constexpr (MODE == 2) {
                const float* plane = reinterpret_cast<const float*>(a.plane);
                float4 lo[LR], hi[LR];
#pragma unroll
                for (int n = 0; n < LR; ++n) {
                    lo[n] = hi[n] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (in && rows[n] >= 0) {
                        const float4* src = reinterpret_cast<const float4*>(plane + (size_t)rows[n] * a.stride + c);
                        lo[n] = src[0];
                        hi[n] = src[1];
                    }
                }
#pragma unroll
                for (int n = 0; n < LR; ++n) {
                    const float x[8] = {lo[n].x, lo[n].y, lo[n].z, lo[n].w, hi[n].x, hi[n].y, hi[n].z, hi[n].w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[p][e] = __builtin_fmaf(x[e], w[n], acc[p][e]);
                }
            } else {
                const uint16_t* plane = reinterpret_cast<const uint16_t*>(a.plane);
                uint4 xv[LR];
#pragma unroll
                for (int n = 0; n < LR; ++n)
                    xv[n] = in && rows[n] >= 0 ? *reinterpret_cast<const uint4*>(plane + (size_t)rows[n] * a.stride + c) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (int n = 0; n < LR; ++n) {
                    const uint16_t* xh = reinterpret_cast<const uint16_t*>(&xv[n]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[p][e] = __builtin_fmaf(half_to_f32<MODE>(xh[e]), w[n], acc[p][e]);
                }
            }
        }
    }

    // the four runs meet in LDS and add in wave order; thread t then owns columns t, t + 256, ... of the block: coalesced stores
#pragma unroll
    for (int p = 0; p < P; ++p) {
        float4* dst = reinterpret_cast<float4*>(fold + wave * (P * 512) + p * 512 + lane * 8);
        dst[0] = make_float4(acc[p][0], acc[p][1], acc[p][2], acc[p][3]);
        dst[1] = make_float4(acc[p][4], acc[p][5], acc[p][6], acc[p][7]);
    }
    __syncthreads();
    float* dst = a.chunks == 1 ? a.out + q * a.dim : a.part + (q * a.chunks + chunk) * a.dim;
    for (int i = tid; i < P * 512 && col0 + i < a.dim; i += LT)
        dst[col0 + i] = ((fold[i] + fold[P * 512 + i]) + fold[2 * P * 512 + i]) + fold[3 * P * 512 + i];
    static_assert(LW == 4, "the fold above names four waves");
}

// out[q, d] = parts[0][q, d] + parts[1][q, d] + ... in increasing part order: the chunks of a list, or the shards of a node index
__global__ __launch_bounds__(256) void fold_listed_sum_kernel(const float* __restrict__ parts, int64_t n_parts, int64_t part_stride,
                                                              int64_t q_stride, int dim, float* __restrict__ out) {
    const int d = (int)blockIdx.y * 256 + (int)threadIdx.x;
    const int64_t q = blockIdx.x;
    if (d >= dim) return;
    const float* src = parts + q * q_stride + d;
    float s = src[0];
    int64_t p = 1;
    for (; p + 8 <= n_parts; p += 8) {  // eight loads in flight, added in part order
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = src[(p + i) * part_stride];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; p < n_parts; ++p) s += src[p * part_stride];
    out[q * dim + d] = s;
}

// out[i] = the score the OWNER of ids[i] computed (shard g of a node index holds the global rows [g * R, (g + 1) * R)): by ownership, not
// by comparing values - a NaN score survives, and a slot no shard owns is -inf
__global__ __launch_bounds__(256) void combine_listed_kernel(const float* __restrict__ parts, const int64_t* __restrict__ ids, int64_t n,
                                                             int n_shards, int64_t rows_per_shard, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    float v = -__builtin_inff();
    if (id >= 0 && rows_per_shard > 0) {
        const int64_t g = id / rows_per_shard;
        if (g < n_shards) v = parts[(size_t)g * n + i];
    }
    out[i] = v;
}

// One workgroup per query: keys (score, local row) of the m slots, sorted descending; an entry equal to its predecessor leaves (a listed
// id counts once, like a `terms` filter), NaN and -inf never enter; the k best by (score desc, id asc) leave, pads (-inf, -1).
__global__ __launch_bounds__(ST) void select_listed_kernel(const float* __restrict__ scores, const int64_t* __restrict__ ids, int m, int P,
                                                           int k, int64_t id_base, float* __restrict__ out_scores,
                                                           int64_t* __restrict__ out_ids) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    key_t64* kb = reinterpret_cast<key_t64*>(smem);
    __shared__ int wave_cnt[ST / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    for (int c = tid; c < P; c += ST) {
        key_t64 key = 0ull;
        if (c < m) {
            const float s = scores[q * m + c];
            const int64_t local = ids[q * m + c] - id_base;
            if (s == s && s > -__builtin_inff() && local >= 0 && local < 0xFFFFFFFFll) key = make_key(s, (unsigned)local);
        }
        kb[c] = key;
    }
    __syncthreads();
    (void)wg_sort_lds_1024<true>(kb, P, tid);  // (ends with a barrier)
    // compaction: thread t owns the E consecutive sorted entries [t * E, (t + 1) * E)
    const int E = P / ST;
    int mine = 0;
    for (int j = 0; j < E; ++j) {
        const int i = tid * E + j;
        const key_t64 key = kb[i];
        mine += (key != 0ull && (i == 0 || kb[i - 1] != key)) ? 1 : 0;
    }
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_cnt[wave] = incl;
    __syncthreads();
    int before = incl - mine, total = 0;
    for (int w = 0; w < ST / 64; ++w) {
        if (w < wave) before += wave_cnt[w];
        total += wave_cnt[w];
    }
    for (int j = 0; j < E; ++j) {
        const int i = tid * E + j;
        const key_t64 key = kb[i];
        if (key != 0ull && (i == 0 || kb[i - 1] != key)) {
            if (before < k) {
                out_scores[q * k + before] = unflip_f32((unsigned)(key >> 32));
                out_ids[q * k + before] = id_base + (int64_t)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
            }
            ++before;
        }
    }
    for (int c = total + tid; c < k; c += ST) {
        out_scores[q * k + c] = -__builtin_inff();
        out_ids[q * k + c] = -1;
    }
}

}  // namespace

hipError_t launch_score_listed(ListedArgs a, int64_t nq, hipStream_t stream) {
    if (nq <= 0 || a.m <= 0) return hipSuccess;
    // slots per workgroup: 64 where that still gives every CU its 4 workgroups twice over, down to 16 (one group of LR rows per wave)
    // for small batches - 64 queries x 385 slots are 1600 workgroups of 16 slots.  The scores do not depend on the choice.
    int spb = 64;
    while (spb > 16 && nq * ((a.m + spb - 1) / spb) < 2048) spb >>= 1;
    a.spb = spb;
    a.chunks = (a.m + spb - 1) / spb;
    const int64_t blocks = nq * a.chunks;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    const int bytes = a.dim_pad * (a.exact ? 4 : 2);
    const void* fn = a.exact ? (const void*)score_listed_kernel<2> : a.store_dtype == 0 ? (const void*)score_listed_kernel<0> : (const void*)score_listed_kernel<1>;
    if (hipError_t e = allow_dynamic_lds(fn, bytes); e != hipSuccess) return e;
    if (a.exact) hipLaunchKernelGGL(score_listed_kernel<2>, dim3((unsigned)blocks), dim3(LT), bytes, stream, a);
    else if (a.store_dtype == 0) hipLaunchKernelGGL(score_listed_kernel<0>, dim3((unsigned)blocks), dim3(LT), bytes, stream, a);
    else hipLaunchKernelGGL(score_listed_kernel<1>, dim3((unsigned)blocks), dim3(LT), bytes, stream, a);
    return hipGetLastError();
}

int64_t listed_sum_chunks(int64_t m) { return (m + SC - 1) / SC; }

template <int MODE>
static hipError_t sum_listed_passes(const ListedArgs& a, dim3 grid, int passes, hipStream_t stream) {
    const int bytes = LW * passes * 512 * (int)sizeof(float);  // <= 32 KiB
    switch (passes) {
        case 1: hipLaunchKernelGGL((sum_listed_kernel<MODE, 1>), grid, dim3(LT), bytes, stream, a); break;
        case 2: hipLaunchKernelGGL((sum_listed_kernel<MODE, 2>), grid, dim3(LT), bytes, stream, a); break;
        case 3: hipLaunchKernelGGL((sum_listed_kernel<MODE, 3>), grid, dim3(LT), bytes, stream, a); break;
        default: hipLaunchKernelGGL((sum_listed_kernel<MODE, SP>), grid, dim3(LT), bytes, stream, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_sum_listed(ListedArgs a, int64_t nq, hipStream_t stream) {
    if (nq <= 0 || a.m <= 0) return hipSuccess;
    a.chunks = listed_sum_chunks(a.m);
    const int64_t blocks = nq * a.chunks;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    // the passes of a column block follow from the store's width alone: narrow stores do not carry the accumulators of wide ones
    const int passes = std::min(SP, (a.dim_pad + 511) / 512);
    const dim3 grid((unsigned)blocks, (unsigned)((a.dim_pad + SB - 1) / SB));
    hipError_t e;
    if (a.exact) e = sum_listed_passes<2>(a, grid, passes, stream);
    else if (a.store_dtype == 0) e = sum_listed_passes<0>(a, grid, passes, stream);
    else e = sum_listed_passes<1>(a, grid, passes, stream);
    if (e != hipSuccess || a.chunks == 1) return e;
    return launch_fold_listed_sum(a.part, a.chunks, a.dim, a.chunks * a.dim, nq, a.dim, a.out, stream);
}

hipError_t launch_fold_listed_sum(const float* parts, int64_t n_parts, int64_t part_stride, int64_t q_stride, int64_t nq, int dim, float* out,
                                  hipStream_t stream) {
    if (nq <= 0 || dim <= 0 || n_parts <= 0) return hipSuccess;
    if (nq > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fold_listed_sum_kernel, dim3((unsigned)nq, (unsigned)((dim + 255) / 256)), dim3(256), 0, stream, parts, n_parts, part_stride,
                       q_stride, dim, out);
    return hipGetLastError();
}

hipError_t launch_combine_listed(const float* parts, const int64_t* ids, int64_t n, int n_shards, int64_t rows_per_shard, float* out,
                                 hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(combine_listed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, parts, ids, n, n_shards, rows_per_shard, out);
    return hipGetLastError();
}

hipError_t launch_select_listed(const float* scores, const int64_t* ids, int64_t nq, int64_t m, int k, int64_t id_base, float* out_scores,
                                int64_t* out_ids, hipStream_t stream) {
    if (nq <= 0) return hipSuccess;
    if (m < 1 || m > 8192 || nq > 0x7fffffffll) return hipErrorInvalidValue;
    int P = ST;
    while (P < m) P <<= 1;
    const int bytes = P * (int)sizeof(key_t64);
    if (hipError_t e = allow_dynamic_lds((const void*)select_listed_kernel, bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(select_listed_kernel, dim3((unsigned)nq), dim3(ST), bytes, stream, scores, ids, (int)m, P, k, id_base, out_scores, out_ids);
    return hipGetLastError();
}

}  // namespace vodhip
