// Sequence pooling of the encoder's last hidden state, with activation, norm and scale, forward and backward, on gfx950.
//
// Replaces the reference's src/vod_models/vod_encoder/modeling.py: VodPooler.forward :164-174, MeanAgg :76-82, ClsAgg :85-89
// (x.sum(-2) / mask.sum(), the activation, F.normalize, the multiplication by exp(0.5 * log_scaler)) and the autograd backward of those.
//
// hidden is [N, L, H] (1.6 GB in bf16 at 2112 x 512 x 768): a memory-bound stream.  Kernels:
//   pool_aggregate_kernel   one workgroup per (row n, chunk of L): its token rows are read ONCE; with one chunk per row it divides by
//                           the live count, writes a [N, H] and goes straight on to the finish (one launch); with several chunks it
//                           writes float32 partial sums [N, n_chunks, H]
//   pool_reduce_kernel      one workgroup per row: partials summed in chunk order, then the same tail
//   pool_finish_*_kernel    one workgroup per [N, P] row: activation, norm, scale (behind a projection) and their backward
//   pool_backward_kernel    one workgroup per (row n, chunk of L): da[n] recomputed from the saved a and the upstream gradient (H
//                           elements, two reductions), its chunk of d hidden written once, zeros included
// finish_row / finish_stats / finish_dz are the ONE finish routine of all of them: the fused and the split paths give the same bits.
// No atomics (bitwise reproducible), no device allocation, no host synchronisation (the scale is read from device memory).
#include "../../include/vodhip.h"
#include "vodhip_internal.h"
#include "row_reduce.h"

#include <algorithm>
#include <type_traits>

namespace vodhip {

constexpr int PL_THREADS = 256;
constexpr float PL_EPS = 1e-12f;  // F.normalize's default
constexpr int PL_INFLIGHT = 8;     // 16-byte loads a lane of the aggregate issues before it adds any

__device__ __forceinline__ float ld_any(const void* p, int dt, int64_t i) {
    switch (dt) {
        case 0: return ld_enc<0>(p, i);
        case 1: return ld_enc<1>(p, i);
        default: return ld_enc<2>(p, i);
    }
}
__device__ __forceinline__ void st_any(void* p, int dt, int64_t i, float v) {
    switch (dt) {
        case 0: st_enc<0>(p, i, v); break;
        case 1: st_enc<1>(p, i, v); break;
        default: st_enc<2>(p, i, v); break;
    }
}

__device__ __forceinline__ float pool_act(int act, float z) {
    switch (act) {
        case VODHIP_POOL_ACT_RELU: return z > 0.f ? z : 0.f;
        case VODHIP_POOL_ACT_TANH: return tanhf(z);
        case VODHIP_POOL_ACT_SIGMOID: return 1.f / (1.f + expf(-z));
        case VODHIP_POOL_ACT_GELU: return 0.5f * z * (1.f + erff(z * 0.70710678118654752f));  // nn.GELU(): the exact erf form
        default: return z;
    }
}
__device__ __forceinline__ float pool_act_grad(int act, float z) {
    switch (act) {
        case VODHIP_POOL_ACT_RELU: return z > 0.f ? 1.f : 0.f;
        case VODHIP_POOL_ACT_TANH: {
            const float t = tanhf(z);
            return 1.f - t * t;
        }
        case VODHIP_POOL_ACT_SIGMOID: {
            const float s = 1.f / (1.f + expf(-z));
            return s * (1.f - s);
        }
        case VODHIP_POOL_ACT_GELU:
            return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * expf(-0.5f * z * z);
        default: return 1.f;
    }
}

// ---- the finish: t = act(z); u = t / max(|t|_p, eps); y = c u -----------------------------------------------------------------
// forward of one row, by the whole workgroup.  z has `zdt`, y gets `ydt`; `off` is the row's first element.
__device__ __forceinline__ void finish_row(const void* z, int zdt, int64_t off, int P, int act, int norm, float c, void* y, int ydt,
                                           float* red) {
    float d = 1.f;
    if (norm != VODHIP_POOL_NORM_NONE) {
        float s = 0.f;
        for (int i = threadIdx.x; i < P; i += PL_THREADS) {
            const float t = pool_act(act, ld_any(z, zdt, off + i));
            s += norm == VODHIP_POOL_NORM_L2 ? t * t : fabsf(t);
        }
        s = block_sum(s, red);
        d = fmaxf(norm == VODHIP_POOL_NORM_L2 ? sqrtf(s) : s, PL_EPS);
    }
    for (int i = threadIdx.x; i < P; i += PL_THREADS) st_any(y, ydt, off + i, c * (pool_act(act, ld_any(z, zdt, off + i)) / d));
}

// backward, the row's two reductions: nrm = |t|_p (1 without a norm) and dot = sum u * (c g), which is also sum g * y
__device__ __forceinline__ void finish_stats(const void* z, int zdt, const void* g, int gdt, int64_t off, int P, int act, int norm,
                                             float c, float* red, float& nrm, float& dot) {
    nrm = 1.f;
    float d = 1.f;
    if (norm != VODHIP_POOL_NORM_NONE) {
        float s = 0.f;
        for (int i = threadIdx.x; i < P; i += PL_THREADS) {
            const float t = pool_act(act, ld_any(z, zdt, off + i));
            s += norm == VODHIP_POOL_NORM_L2 ? t * t : fabsf(t);
        }
        s = block_sum(s, red);
        nrm = norm == VODHIP_POOL_NORM_L2 ? sqrtf(s) : s;
        d = fmaxf(nrm, PL_EPS);
    }
    float acc = 0.f;
    for (int i = threadIdx.x; i < P; i += PL_THREADS)
        acc += (pool_act(act, ld_any(z, zdt, off + i)) / d) * (c * ld_any(g, gdt, off + i));
    dot = block_sum(acc, red);
}

// backward, one element: dL/dz from z, g = dL/dy and the row's (nrm, dot)
__device__ __forceinline__ float finish_dz(float z, float g, int act, int norm, float c, float nrm, float dot) {
    const float du = c * g;
    float dt = du;
    if (norm != VODHIP_POOL_NORM_NONE) {
        if (nrm > PL_EPS) {
            const float t = pool_act(act, z);
            const float dir = norm == VODHIP_POOL_NORM_L2 ? t / nrm : (t > 0.f ? 1.f : (t < 0.f ? -1.f : 0.f));
            dt = (du - dir * dot) / nrm;
        } else {
            dt = du / PL_EPS;  // the clamp is active: the norm carries no gradient
        }
    }
    return dt * pool_act_grad(act, z);
}

// live elements of mask row n, by the whole workgroup (exact in float32 below 2^24 tokens)
__device__ __forceinline__ float row_live_count(const void* mask, int mask_eb, int64_t row_off, int L, float* red) {
    float c = 0.f;
    for (int l = threadIdx.x; l < L; l += PL_THREADS) c += mask_live(mask, row_off + l, mask_eb) ? 1.f : 0.f;
    return block_sum(c, red);
}

// Work split of a [tokens, H] tile over 256 threads.  A "group" is what one lane moves at once: 16 bytes (VEC) or one element.
// With G groups per token row, CW = min(G, 256) lanes sit side by side on a row and R = 256 / CW token rows are in flight; lane
// (r, cl) owns the columns cl, cl + CW, ... ("sweeps", only when G > 256 and then R = 1) of the tokens r, r + R, ...
struct PoolSplit {
    int G, CW, R, r, cl;
    bool active;
};
template <int EPV>
__device__ __forceinline__ PoolSplit pool_split(int H) {
    PoolSplit s;
    s.G = H / EPV;
    s.CW = s.G < PL_THREADS ? s.G : PL_THREADS;
    s.R = PL_THREADS / s.CW;
    s.r = threadIdx.x / s.CW;
    s.cl = threadIdx.x - s.r * s.CW;
    s.active = s.r < s.R;
    return s;
}

// what one lane moves at once, as it comes from memory (unpacked only when it is added: 4 registers per load in flight, not 8)
template <int DT, bool VEC>
struct RawGroup {
    std::conditional_t<VEC, uint4, float> w;
    __device__ __forceinline__ void load(const char* p) {
        if constexpr (VEC) w = *(const uint4*)p;
        else w = ld_enc<DT>(p, 0);
    }
    __device__ __forceinline__ void add_to(float* acc) const {
        if constexpr (VEC) {
            float v[elems_per_vec<DT>()];
            unpack16<DT>(w, v);
#pragma unroll
            for (int u = 0; u < elems_per_vec<DT>(); ++u) acc[u] += v[u];
        } else {
            acc[0] += w;
        }
    }
};

// masked mode, backward: the liveness of tokens [t0, t1) of a mask row (at most PL_TILE of them) goes to LDS first, so that the
// store loop runs behind an LDS read and not behind a second trip to memory.  Barriers on both sides: call it workgroup-wide.
constexpr int PL_TILE = 2048;
__device__ __forceinline__ void stage_live(uint8_t* live_s, const void* mask, int mask_eb, int64_t mrow, int64_t t0, int64_t t1) {
    __syncthreads();
    for (int i = threadIdx.x; i < (int)(t1 - t0); i += PL_THREADS) live_s[i] = mask_live(mask, mrow + t0 + i, mask_eb) ? 1 : 0;
    __syncthreads();
}

// masked mode, forward: the LIVE tokens of [t0, t1) as an ordered list of offsets in LDS, so that the token loop is the same
// back-to-back batch of loads in both mask modes.  Each thread tests PL_TILE / 256 consecutive tokens, a workgroup scan places them.
// Returns the number of live tokens.  Workgroup-wide.
__device__ __forceinline__ int stage_live_list(uint16_t* idx_s, int* wave_sum, const void* mask, int mask_eb, int64_t mrow, int64_t t0,
                                               int64_t t1) {
    constexpr int PER = PL_TILE / PL_THREADS;
    const int n = (int)(t1 - t0), base = threadIdx.x * PER, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned bits = 0;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (base + u < n && mask_live(mask, mrow + t0 + base + u, mask_eb)) bits |= 1u << u;
    }
    const int mine = __popc(bits);
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    __syncthreads();  // the previous tile's list has been used up
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int off = incl - mine;
    for (int w = 0; w < wave; ++w) off += wave_sum[w];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (bits >> u & 1u) idx_s[off++] = (uint16_t)(base + u);
    }
    const int total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
    __syncthreads();
    return total;
}

// ------------------------------------------------------------------------------------------------
// 1. aggregate forward.  blockIdx.x = n * n_chunks + chunk; the chunk covers tokens [chunk * lc, min(L, (chunk + 1) * lc)).
//    cls: one chunk, the token range is [0, 1) and the count is 1.
//    n_chunks = 1: a[n,:] = sum / cnt (0 when cnt = 0), then the finish when `finish` is set.  n_chunks > 1: partials only.
// ------------------------------------------------------------------------------------------------
template <int DT, bool VEC>
__global__ __launch_bounds__(PL_THREADS) void pool_aggregate_kernel(
    const void* __restrict__ x, const void* __restrict__ mask, int mask_eb, int L, int H, int lc, int n_chunks, int agg, int masked,
    float* a, float* __restrict__ partials, int finish, int act, int norm, const float* __restrict__ log_scaler, void* y, int ydt) {
    constexpr int EPV = VEC ? elems_per_vec<DT>() : 1;
    constexpr int ES = DT == 2 ? 4 : 2;
    __shared__ float red[4];
    __shared__ float cross[PL_THREADS * EPV];  // cross-token-row sums, R > 1 only
    __shared__ uint16_t idx_s[PL_TILE];  // masked mode: the live tokens of the tile
    __shared__ int wave_sum[4];
    const int64_t n = blockIdx.x / n_chunks;
    const int chunk = (int)(blockIdx.x - n * n_chunks);
    const bool cls = agg == VODHIP_POOL_AGG_CLS;
    const int64_t l0 = cls ? 0 : (int64_t)chunk * lc;
    const int64_t l1 = cls ? 1 : (l0 + lc < L ? l0 + lc : L);
    const bool skip_pads = masked && !cls;
    const int64_t mrow = n * L;
    const int64_t xrow = n * (int64_t)L * H;
    const PoolSplit sp = pool_split<EPV>(H);
    float cnt = 1.f;
    if (n_chunks == 1 && !cls) cnt = row_live_count(mask, mask_eb, mrow, L, red);
    float* dst = n_chunks == 1 ? a + n * H : partials + (int64_t)blockIdx.x * H;

    for (int cb = 0; cb < sp.G; cb += sp.CW) {
        const int v = cb + sp.cl;
        const bool mine = sp.active && v < sp.G;
        float acc[EPV];
#pragma unroll
        for (int u = 0; u < EPV; ++u) acc[u] = 0.f;
        const int64_t col = xrow + (int64_t)v * EPV;
        for (int64_t t0 = l0; t0 < l1; t0 += PL_TILE) {
            const int64_t t1 = t0 + PL_TILE < l1 ? t0 + PL_TILE : l1;
            // the tokens to read: all of the tile, or the live ones through the list (a padded token row is not read)
            const int n_tok = skip_pads ? stage_live_list(idx_s, wave_sum, mask, mask_eb, mrow, t0, t1) : (int)(t1 - t0);
            if (!mine) continue;
            const char* tile = (const char*)x + (col + t0 * H) * ES;
            const int64_t pitch = (int64_t)H * ES;
            int j = sp.r;
#pragma nounroll
            for (; j + (PL_INFLIGHT - 1) * sp.R < n_tok; j += PL_INFLIGHT * sp.R) {  // PL_INFLIGHT loads go out back to back
                RawGroup<DT, VEC> raw[PL_INFLIGHT];
#pragma unroll
                for (int k = 0; k < PL_INFLIGHT; ++k) raw[k].load(tile + (skip_pads ? idx_s[j + k * sp.R] : j + k * sp.R) * pitch);
#pragma unroll
                for (int k = 0; k < PL_INFLIGHT; ++k) raw[k].add_to(acc);
            }
#pragma nounroll
            for (; j < n_tok; j += sp.R) {
                RawGroup<DT, VEC> raw;
                raw.load(tile + (skip_pads ? idx_s[j] : j) * pitch);
                raw.add_to(acc);
            }
        }
        if (sp.R > 1) {  // one sweep: token rows r = 0..R-1 meet in LDS, summed by row 0 in row order
            if (mine) {
#pragma unroll
                for (int u = 0; u < EPV; ++u) cross[(sp.r * sp.CW + sp.cl) * EPV + u] = acc[u];
            }
            __syncthreads();
            if (mine && sp.r == 0) {
                for (int rr = 1; rr < sp.R; ++rr) {
#pragma unroll
                    for (int u = 0; u < EPV; ++u) acc[u] += cross[(rr * sp.CW + sp.cl) * EPV + u];
                }
            }
        }
        if (mine && sp.r == 0) {
#pragma unroll
            for (int u = 0; u < EPV; ++u) dst[(int64_t)v * EPV + u] = n_chunks == 1 ? (cnt > 0.f ? acc[u] / cnt : 0.f) : acc[u];
        }
    }
    if (n_chunks == 1 && finish) {
        __syncthreads();  // a[n,:] was written by other lanes of this workgroup
        finish_row(a, 2, n * H, H, act, norm, expf(0.5f * log_scaler[0]), y, ydt, red);
    }
}

// ------------------------------------------------------------------------------------------------
// 2. several chunks per row: a[n,:] = (sum of the partials in chunk order) / cnt, then the same tail.  blockIdx.x = n.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PL_THREADS) void pool_reduce_kernel(const float* __restrict__ partials, const void* __restrict__ mask,
                                                                 int mask_eb, int L, int H, int n_chunks, float* a, int finish, int act,
                                                                 int norm, const float* __restrict__ log_scaler, void* y, int ydt) {
    __shared__ float red[4];
    const int64_t n = blockIdx.x;
    const float cnt = row_live_count(mask, mask_eb, n * L, L, red);
    const float* p = partials + n * n_chunks * H;
    for (int h = threadIdx.x; h < H; h += PL_THREADS) {
        float acc = p[h];
        for (int ch = 1; ch < n_chunks; ++ch) acc += p[(int64_t)ch * H + h];
        a[n * H + h] = cnt > 0.f ? acc / cnt : 0.f;
    }
    if (finish) {
        __syncthreads();
        finish_row(a, 2, n * H, H, act, norm, expf(0.5f * log_scaler[0]), y, ydt, red);
    }
}

// ------------------------------------------------------------------------------------------------
// 3. the finish on its own, behind a projection.  blockIdx.x = n.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PL_THREADS) void pool_finish_forward_kernel(const void* __restrict__ z, int zdt, int P, int act, int norm,
                                                                         const float* __restrict__ log_scaler, void* __restrict__ y,
                                                                         int ydt) {
    __shared__ float red[4];
    finish_row(z, zdt, (int64_t)blockIdx.x * P, P, act, norm, expf(0.5f * log_scaler[0]), y, ydt, red);
}

__global__ __launch_bounds__(PL_THREADS) void pool_finish_backward_kernel(const void* __restrict__ z, int zdt, const void* __restrict__ g,
                                                                          int gdt, int P, int act, int norm,
                                                                          const float* __restrict__ log_scaler, void* __restrict__ dz,
                                                                          int dzdt, float* __restrict__ gy) {
    __shared__ float red[4];
    const int64_t off = (int64_t)blockIdx.x * P;
    const float c = expf(0.5f * log_scaler[0]);
    float nrm, dot;
    finish_stats(z, zdt, g, gdt, off, P, act, norm, c, red, nrm, dot);
    if (threadIdx.x == 0) gy[blockIdx.x] = dot;
    for (int i = threadIdx.x; i < P; i += PL_THREADS)
        st_any(dz, dzdt, off + i, finish_dz(ld_any(z, zdt, off + i), ld_any(g, gdt, off + i), act, norm, c, nrm, dot));
}

// ------------------------------------------------------------------------------------------------
// 4. backward.  blockIdx.x = n * n_chunks + chunk.  da[n,:] = finish ? dL/da through the finish (from the saved a and g = dL/dy)
//    : g itself (float32 dL/da, the projection's input gradient).  d hidden[n,l,:] = da / cnt at the positions the aggregate read
//    (mean: all, or the live ones; cls: l = 0), exactly 0 elsewhere and in a row without a live token.
// ------------------------------------------------------------------------------------------------
template <int DT, bool VEC>
__global__ __launch_bounds__(PL_THREADS) void pool_backward_kernel(
    const void* __restrict__ g, int gdt, const float* __restrict__ a, const void* __restrict__ mask, int mask_eb, int L, int H, int lc,
    int n_chunks, int agg, int masked, int finish, int act, int norm, const float* __restrict__ log_scaler, void* __restrict__ dx,
    float* __restrict__ gy) {
    constexpr int EPV = VEC ? elems_per_vec<DT>() : 1;
    constexpr int ES = DT == 2 ? 4 : 2;
    __shared__ float red[4];
    const int64_t n = blockIdx.x / n_chunks;
    const int chunk = (int)(blockIdx.x - n * n_chunks);
    const bool cls = agg == VODHIP_POOL_AGG_CLS;
    const int64_t l0 = (int64_t)chunk * lc;
    const int64_t l1 = l0 + lc < L ? l0 + lc : L;
    const int64_t mrow = n * L;
    const int64_t xrow = n * (int64_t)L * H;
    const int64_t arow = n * H;
    const PoolSplit sp = pool_split<EPV>(H);
    const float cnt = cls ? 1.f : row_live_count(mask, mask_eb, mrow, L, red);
    float c = 1.f, nrm = 1.f, dot = 0.f;
    if (finish) {
        c = expf(0.5f * log_scaler[0]);
        finish_stats(a, 2, g, gdt, arow, H, act, norm, c, red, nrm, dot);
        if (chunk == 0 && threadIdx.x == 0) gy[n] = dot;
    }
    const bool dead_row = !(cnt > 0.f);
    const bool by_mask = masked && !cls;
    __shared__ uint8_t live_s[PL_TILE];
    for (int cb = 0; cb < sp.G; cb += sp.CW) {
        const int v = cb + sp.cl;
        const bool mine = sp.active && v < sp.G;
        float val[EPV];
#pragma unroll
        for (int u = 0; u < EPV; ++u) val[u] = 0.f;
        if (mine && !dead_row) {
#pragma unroll
            for (int u = 0; u < EPV; ++u) {
                const int64_t i = arow + (int64_t)v * EPV + u;
                const float gi = ld_any(g, gdt, i);
                val[u] = (finish ? finish_dz(a[i], gi, act, norm, c, nrm, dot) : gi) / cnt;
            }
        }
        const int64_t col = xrow + (int64_t)v * EPV;
        uint4 pv = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (VEC) pv = pack16<DT>(val);
        for (int64_t t0 = l0; t0 < l1; t0 += PL_TILE) {
            const int64_t t1 = t0 + PL_TILE < l1 ? t0 + PL_TILE : l1;
            if (by_mask) stage_live(live_s, mask, mask_eb, mrow, t0, t1);
            if (!mine) continue;
            for (int64_t l = t0 + sp.r; l < t1; l += sp.R) {
                const bool on = cls ? l == 0 : (!by_mask || live_s[l - t0]);
                // (selected word by word: `on ? pv : zero` on the struct is compiled into a select between two scratch copies)
                if constexpr (VEC) *(uint4*)((char*)dx + (col + l * H) * ES) = make_uint4(on ? pv.x : 0u, on ? pv.y : 0u, on ? pv.z : 0u, on ? pv.w : 0u);
                else st_enc<DT>(dx, col + l * H, on ? val[0] : 0.f);
            }
        }
    }
}

// 16-byte accesses need every token row on a 16-byte boundary: the tensor's base and the row pitch
static bool rows_aligned16(const void* p, int64_t H, int dtype) {
    const int64_t es = dtype == 2 ? 4 : 2;
    return ((uintptr_t)p % 16 == 0) && (H * es % 16 == 0);
}

// Chunking of L.  l_chunk > 0 is taken as it is (clamped to L).  Auto depends on (N, L, H) alone: one chunk per row - the
// single-launch path - unless N is small AND the rows are long: then L is cut so that about 1024 workgroups exist, but never below
// 64 Ki elements per workgroup.  Measured on an MI355X (profiles/pooler.json): at 64 x 64 x 768 one launch with 48 Ki elements per
// workgroup takes 25 us per eager forward against 30 us for three chunks + the reduce launch, and at 2112 x 512 x 768 one chunk per
// row (0.310 ms) beats chunks of 128 (0.325 ms) and 64 tokens (0.335 ms).
PoolPlan pool_plan(int64_t N, int64_t L, int64_t H, int64_t l_chunk) {
    PoolPlan p;
    if (l_chunk > 0) {
        p.l_chunk = std::min(l_chunk, L);
    } else {
        const int64_t want = (1024 + N - 1) / N;
        const int64_t min_tokens = std::max<int64_t>(1, (65536 + H - 1) / H);
        const int64_t chunks = std::max<int64_t>(1, std::min(want, L / min_tokens));
        p.l_chunk = (L + chunks - 1) / chunks;
    }
    p.n_chunks = (L + p.l_chunk - 1) / p.l_chunk;
    return p;
}

hipError_t launch_pool_forward(const void* hidden, int dtype, int64_t N, int64_t L, int64_t H, const void* mask, int mask_eb, int agg,
                               int masked, int finish, int act, int norm, const float* log_scaler, int64_t l_chunk, float* a, void* y,
                               int y_dtype, float* workspace, hipStream_t stream) {
    PoolPlan plan = pool_plan(N, L, H, l_chunk);
    if (agg == VODHIP_POOL_AGG_CLS) plan.l_chunk = L, plan.n_chunks = 1;
    const bool vec = rows_aligned16(hidden, H, dtype);
    const dim3 grid((unsigned)(N * plan.n_chunks));
#define VOD_PA(DT, VEC)                                                                                                         \
    if (dtype == DT && vec == VEC) {                                                                                            \
        hipLaunchKernelGGL((pool_aggregate_kernel<DT, VEC>), grid, dim3(PL_THREADS), 0, stream, hidden, mask, mask_eb, (int)L,  \
                           (int)H, (int)plan.l_chunk, (int)plan.n_chunks, agg, masked, a, workspace, finish, act, norm,         \
                           log_scaler, y, y_dtype);                                                                             \
    }
    VOD_PA(0, true) VOD_PA(0, false) VOD_PA(1, true) VOD_PA(1, false) VOD_PA(2, true) VOD_PA(2, false)
#undef VOD_PA
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || plan.n_chunks == 1) return e;
    hipLaunchKernelGGL(pool_reduce_kernel, dim3((unsigned)N), dim3(PL_THREADS), 0, stream, (const float*)workspace, mask, mask_eb,
                       (int)L, (int)H, (int)plan.n_chunks, a, finish, act, norm, log_scaler, y, y_dtype);
    return hipGetLastError();
}

hipError_t launch_pool_backward(const void* g, int g_dtype, const float* a, int64_t N, int64_t L, int64_t H, const void* mask,
                                int mask_eb, int agg, int masked, int finish, int act, int norm, const float* log_scaler,
                                int64_t l_chunk, void* d_hidden, int dtype, float* gy, hipStream_t stream) {
    const PoolPlan plan = pool_plan(N, L, H, l_chunk);
    const bool vec = rows_aligned16(d_hidden, H, dtype);
    const dim3 grid((unsigned)(N * plan.n_chunks));
#define VOD_PB(DT, VEC)                                                                                                            \
    if (dtype == DT && vec == VEC) {                                                                                               \
        hipLaunchKernelGGL((pool_backward_kernel<DT, VEC>), grid, dim3(PL_THREADS), 0, stream, g, g_dtype, a, mask, mask_eb,       \
                           (int)L, (int)H, (int)plan.l_chunk, (int)plan.n_chunks, agg, masked, finish, act, norm, log_scaler,      \
                           d_hidden, gy);                                                                                          \
    }
    VOD_PB(0, true) VOD_PB(0, false) VOD_PB(1, true) VOD_PB(1, false) VOD_PB(2, true) VOD_PB(2, false)
#undef VOD_PB
    return hipGetLastError();
}

hipError_t launch_pool_finish_forward(const void* z, int z_dtype, int64_t N, int64_t P, int act, int norm, const float* log_scaler,
                                      void* y, int y_dtype, hipStream_t stream) {
    hipLaunchKernelGGL(pool_finish_forward_kernel, dim3((unsigned)N), dim3(PL_THREADS), 0, stream, z, z_dtype, (int)P, act, norm,
                       log_scaler, y, y_dtype);
    return hipGetLastError();
}

hipError_t launch_pool_finish_backward(const void* z, int z_dtype, const void* g, int g_dtype, int64_t N, int64_t P, int act, int norm,
                                       const float* log_scaler, void* dz, int dz_dtype, float* gy, hipStream_t stream) {
    hipLaunchKernelGGL(pool_finish_backward_kernel, dim3((unsigned)N), dim3(PL_THREADS), 0, stream, z, z_dtype, g, g_dtype, (int)P, act,
                       norm, log_scaler, dz, dz_dtype, gy);
    return hipGetLastError();
}

}  // namespace vodhip
