// Marginal-likelihood objective of a retrieval-augmented LM (REALM), forward and backward, on gfx950.
//
// Replaces the reference's src/vod_models/vod_gradients/marginal_likelihood.py:
//   MarginalLikelihoodGradients.__call__ :12-48, _compute_lm_logprobs :51-66 (shift, masked_fill, log_softmax over V, gather,
//   masked_fill, masked mean over L) and the autograd backward of those.
//
// lm_logits is [B, D, L, V] (~1 GB in bf16 at 8 x 8 x 256 x 32128): the stage is a memory-bound stream, unlike the launch-bound
// retrieval loss next door.  Three kernels touch it as little as the arithmetic allows:
//   lm_token_forward_kernel   one workgroup per (b, d, t < L-1): live rows are read ONCE (online max / sum-exp), masked rows not at all;
//                             leaves the token log-prob and the row's (max, log sum-exp) = 3 floats per token
//   marginal_row_kernel       one workgroup per query row b: masked mean over L, the retriever scores, the marginal, dLoss/dScores
//                             and coef[b,d] = dLoss/d(sum of the live token log-probs of (b,d))
//   lm_token_backward_kernel  one workgroup per (b, d, t): one read and one write of the tensor, softmax recomputed from the saved
//                             (max, log sum-exp) - no max / sum pass
// No atomics (bitwise reproducible), no device allocation, no host synchronisation: one dependent chain on the caller's stream.
#include "vodhip_internal.h"
#include "row_reduce.h"

#include <algorithm>

namespace vodhip {

constexpr int ML_THREADS = 256;
// rows of at most this many 16-byte vectors (8 KiB) go to a one-wave workgroup: a 256-thread group would idle 3 of its 4 waves and
// pay two barriers for the cross-wave reduction
constexpr int ML_WAVE_ROW_VECS = 512;

// running (max, sum of exp(x - max)) of one lane, fed N values at a time: one rescale per group instead of one per value
template <int N>
__device__ __forceinline__ void online_absorb(float& m, float& s, const float* v) {
    float vm = v[0];
#pragma unroll
    for (int u = 1; u < N; ++u) vm = fmaxf(vm, v[u]);
    if (vm > m) {
        s *= __expf(m - vm);  // m = -inf: s is 0 and stays 0
        m = vm;
    }
    if (m > -__builtin_inff()) {  // a maximum that is still -inf: every value so far is -inf and adds nothing (-inf - -inf = NaN)
#pragma unroll
        for (int u = 0; u < N; ++u) s += __expf(v[u] - m);
    }
}

__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    const float sh = mn > -__builtin_inff() ? mn : 0.f;
    s = s * expf(m - sh) + s2 * expf(m2 - sh);
    m = mn;
}

// ------------------------------------------------------------------------------------------------
// 1. token forward.  blockIdx.x = bd * (L-1) + t.  tok_logp[pos] = logits[bd,t,ids[bd,t+1]] - logsumexp_v logits[bd,t,:]
//    tok_lse[pos] = (row max, log sum exp(x - max)): kept apart so that the backward's exp((x - max) - log sum) is as exact at
//    |logits| ~ 1e4 as at 1 (max + log sum in one float carries half an ulp of 1e4 = 5e-4 into every probability).
//    Masked positions write zeros and never touch the row.  A live target outside [0, V-2] gives NaN (it is never an index).
// ------------------------------------------------------------------------------------------------
template <int DT, int T>
__global__ __launch_bounds__(T) void lm_token_forward_kernel(const void* __restrict__ logits, int64_t L, int64_t V,
                                                             const int64_t* __restrict__ ids, const void* __restrict__ mask,
                                                             int mask_eb, int vec, float* __restrict__ tok_logp,
                                                             float* __restrict__ tok_lse) {
    constexpr int EPV = elems_per_vec<DT>();
    const int64_t pos = blockIdx.x;
    const int64_t bd = pos / (L - 1), t = pos - bd * (L - 1);
    const int64_t nxt = bd * L + t + 1;
    const int tid = threadIdx.x;
    if (!mask_live(mask, nxt, mask_eb)) {
        if (tid == 0) {
            tok_logp[pos] = 0.f;
            tok_lse[2 * pos] = 0.f;
            tok_lse[2 * pos + 1] = 0.f;
        }
        return;
    }
    const int64_t base = (bd * L + t) * V;  // in elements
    float m = -__builtin_inff(), s = 0.f;
    if (vec) {
        const uint4* __restrict__ r4 = (const uint4*)((const char*)logits + base * (DT == 2 ? 4 : 2));
        const int nvec = (int)(V / EPV);
        int i = tid;
        for (; i + 3 * T < nvec; i += 4 * T) {  // four loads in flight per lane
            const uint4 a = r4[i], b = r4[i + T], c = r4[i + 2 * T], d = r4[i + 3 * T];
            float v[EPV];
            unpack16<DT>(a, v);
            online_absorb<EPV>(m, s, v);
            unpack16<DT>(b, v);
            online_absorb<EPV>(m, s, v);
            unpack16<DT>(c, v);
            online_absorb<EPV>(m, s, v);
            unpack16<DT>(d, v);
            online_absorb<EPV>(m, s, v);
        }
        for (; i < nvec; i += T) {
            float v[EPV];
            unpack16<DT>(r4[i], v);
            online_absorb<EPV>(m, s, v);
        }
    } else {
        for (int64_t e = tid; e < V; e += T) {
            const float x = ld_enc<DT>(logits, base + e);
            online_absorb<1>(m, s, &x);
        }
    }
    // lanes -> wave (butterfly: every lane ends with the same pair), waves -> workgroup through LDS in wave order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        online_merge(m, s, m2, s2);
    }
    if constexpr (T > 64) {
        __shared__ float red_m[T / 64], red_s[T / 64];
        if ((tid & 63) == 0) {
            red_m[tid >> 6] = m;
            red_s[tid >> 6] = s;
        }
        __syncthreads();
        if (tid == 0) {
            m = red_m[0], s = red_s[0];
#pragma unroll
            for (int w = 1; w < T / 64; ++w) online_merge(m, s, red_m[w], red_s[w]);
        }
    }
    if (tid == 0) {
        const float lg = logf(s);
        const int64_t tgt = ids[nxt];
        const bool ok = tgt >= 0 && tgt < V - 1;  // the reference gathers from log_softmax(...)[..., :-1]
        tok_logp[pos] = ok ? (ld_enc<DT>(logits, base + tgt) - m) - lg : __builtin_nanf("");
        tok_lse[2 * pos] = m;
        tok_lse[2 * pos + 1] = lg;
    }
}

// ------------------------------------------------------------------------------------------------
// 3. logits backward.  blockIdx.x = bd * L + t.  d_logits[bd,t,v] = go * coef[bd] * (1[v == tgt] - exp((x_v - max) - log sum)) at
//    live positions, 0 at masked positions and at t = L-1.
// ------------------------------------------------------------------------------------------------
template <int DT, int T>
__global__ __launch_bounds__(T) void lm_token_backward_kernel(const void* __restrict__ logits, int64_t L, int64_t V,
                                                              const int64_t* __restrict__ ids, const void* __restrict__ mask,
                                                              int mask_eb, int vec, const float* __restrict__ tok_lse,
                                                              const float* __restrict__ coef, const float* __restrict__ grad_out,
                                                              void* __restrict__ d_logits) {
    constexpr int EPV = elems_per_vec<DT>();
    constexpr int ES = DT == 2 ? 4 : 2;
    const int64_t pos = blockIdx.x;
    const int64_t bd = pos / L, t = pos - bd * L;
    const int tid = threadIdx.x;
    const int64_t base = pos * V;
    const bool live = t < L - 1 && mask_live(mask, pos + 1, mask_eb);
    if (!live) {
        if (vec) {
            uint4* __restrict__ o4 = (uint4*)((char*)d_logits + base * ES);
            const int nvec = (int)(V / EPV);
            const uint4 z = make_uint4(0u, 0u, 0u, 0u);
            for (int i = tid; i < nvec; i += T) o4[i] = z;
        } else {
            for (int64_t e = tid; e < V; e += T) st_enc<DT>(d_logits, base + e, 0.f);
        }
        return;
    }
    const int64_t tgt64 = ids[pos + 1];
    const int tgt = (tgt64 >= 0 && tgt64 < V - 1) ? (int)tgt64 : -1;  // an invalid live target: coef is NaN already, nothing to mark
    const int64_t sp = bd * (L - 1) + t;
    const float m = tok_lse[2 * sp], lg = tok_lse[2 * sp + 1];
    const float c = grad_out[0] * coef[bd];
    if (vec) {
        const uint4* __restrict__ r4 = (const uint4*)((const char*)logits + base * ES);
        uint4* __restrict__ o4 = (uint4*)((char*)d_logits + base * ES);
        const int nvec = (int)(V / EPV);
        auto one = [&](const uint4& raw, int i) {
            float v[EPV];
            unpack16<DT>(raw, v);
#pragma unroll
            for (int u = 0; u < EPV; ++u) v[u] = c * ((i * EPV + u == tgt ? 1.f : 0.f) - __expf((v[u] - m) - lg));
            o4[i] = pack16<DT>(v);
        };
        int i = tid;
        for (; i + 3 * T < nvec; i += 4 * T) {
            const uint4 a = r4[i], b = r4[i + T], cc = r4[i + 2 * T], d = r4[i + 3 * T];
            one(a, i);
            one(b, i + T);
            one(cc, i + 2 * T);
            one(d, i + 3 * T);
        }
        for (; i < nvec; i += T) one(r4[i], i);
    } else {
        for (int64_t e = tid; e < V; e += T) {
            const float x = ld_enc<DT>(logits, base + e);
            st_enc<DT>(d_logits, base + e, c * ((e == tgt ? 1.f : 0.f) - __expf((x - m) - lg)));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 2. row kernel.  One 256-thread workgroup per query row b:
//      lp_xz[d] = sum_{live t} tok_logp[b,d,t] / n[d]           (n = 0: NaN, the reference's 0 / 0)
//      r[d]     = <q[b], s[(b,)d]>, -inf where section__score is -inf        -> retriever_scores
//      lp_r = log_softmax_d r ; a = lp_r + lp_xz ; lp_x = logsumexp_d a      -> row partial
//      post = exp(a - lp_x), p = exp(lp_r) ; d_scores = (p - post) / B (0 at padded sections) ; coef = -post / (B n)
// ------------------------------------------------------------------------------------------------
template <int DT, bool S3D, bool PRE>
__global__ __launch_bounds__(ML_THREADS) void marginal_row_kernel(
    const void* __restrict__ q, const void* __restrict__ s, int D, int H, const float* __restrict__ score,
    const float* __restrict__ tok_logp, const void* __restrict__ mask, int mask_eb, int64_t L,
    // no `restrict` on the two score outputs: with one slab the contraction was written INTO retriever_scores (read to LDS first)
    float* retriever_scores, float* d_scores, float* __restrict__ coef, float* __restrict__ row_lpx, float inv_B,
    const float* pre_slabs, int n_slabs, int64_t slab_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qrow = (float*)smem;  // [H]
    float* S = qrow + H;         // [D] scores -> a = lp_r + lp_xz
    float* X = S + D;            // [D] lp_xz
    float* Nn = X + D;           // [D] live tokens
    float* red = Nn + D;         // [4]
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float ninf = -__builtin_inff();

    if constexpr (PRE) {
        // the contraction was done by small_gemm_kernel (MFMA) in `n_slabs` split-K slabs: summed here in slab order
        for (int d = tid; d < D; d += ML_THREADS) {
            float acc = pre_slabs[b * D + d];
            for (int z = 1; z < n_slabs; ++z) acc += pre_slabs[(int64_t)z * slab_stride + b * D + d];
            S[d] = acc;
        }
    } else {
        for (int h = tid; h < H; h += ML_THREADS) qrow[h] = ld_enc<DT>(q, b * H + h);
        __syncthreads();
        // one wavefront per section, lanes split the hidden dimension (coalesced reads of s)
        const int64_t s_base = S3D ? b * (int64_t)D * H : 0;
        for (int d = wave; d < D; d += ML_THREADS / 64) {
            const int64_t off = s_base + (int64_t)d * H;
            float acc = 0.f;
            for (int h = lane; h < H; h += 64) acc = fmaf(qrow[h], ld_enc<DT>(s, off + h), acc);
            acc = wave_sum(acc);
            if (lane == 0) S[d] = acc;
        }
    }
    // masked mean of the token log-probs: one wavefront per section, lanes split L, fixed order
    for (int d = wave; d < D; d += ML_THREADS / 64) {
        const int64_t bd = b * D + d;
        float acc = 0.f, cnt = 0.f;
        for (int64_t t = lane; t < L - 1; t += 64) {
            if (mask_live(mask, bd * L + t + 1, mask_eb)) {
                acc += tok_logp[bd * (L - 1) + t];
                cnt += 1.f;
            }
        }
        acc = wave_sum(acc);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            X[d] = acc / cnt;
            Nn[d] = cnt;
        }
    }
    __syncthreads();

    const float* score_row = score + b * D;
    float mx = ninf;
    for (int d = tid; d < D; d += ML_THREADS) {
        const float sc = score_row[d];
        const bool pad = __builtin_isinf(sc) && sc < 0;
        const float v = pad ? ninf : S[d];
        S[d] = v;
        retriever_scores[b * D + d] = v;
        mx = fmaxf(mx, v);
    }
    mx = block_max(mx, red);
    float se = 0.f;
    for (int d = tid; d < D; d += ML_THREADS) se += expf(S[d] - mx);  // an all-padded row: NaN, exactly as torch
    se = block_sum(se, red);
    const float lse = logf(se);
    float amax = ninf;
    for (int d = tid; d < D; d += ML_THREADS) {
        const float lp_r = S[d] - mx - lse;
        d_scores[b * D + d] = lp_r;  // parked until the posterior is known
        const float a = lp_r + X[d];
        S[d] = a;
        amax = fmaxf(amax, a);  // (skips NaN: the sum below does not)
    }
    amax = block_max(amax, red);
    const float ash = amax > ninf ? amax : 0.f;  // every a = -inf: lp_x = -inf like torch.logsumexp, not NaN
    float ae = 0.f;
    for (int d = tid; d < D; d += ML_THREADS) ae += expf(S[d] - ash);
    ae = block_sum(ae, red);
    const float lp_x = ash + logf(ae);
    for (int d = tid; d < D; d += ML_THREADS) {
        const float sc = score_row[d];
        const bool pad = __builtin_isinf(sc) && sc < 0;
        const float post = expf(S[d] - lp_x);
        const float p = expf(d_scores[b * D + d]);
        d_scores[b * D + d] = pad ? 0.f : (p - post) * inv_B;
        coef[b * D + d] = -post * inv_B / Nn[d];
    }
    if (tid == 0) row_lpx[b] = lp_x;
}

__global__ __launch_bounds__(ML_THREADS) void marginal_finalize_kernel(const float* __restrict__ row_lpx, int B,
                                                                       float* __restrict__ loss) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int b = threadIdx.x; b < B; b += ML_THREADS) acc += row_lpx[b];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) loss[0] = -acc / (float)B;
}

// ------------------------------------------------------------------------------------------------
// The two stages that open vod_row_kernel, as functions: the contraction and the masked token reduction of marginal_row_kernel
// (which keeps its own inline copy: its code object stays the one its measurements were taken on); 256 threads, LDS rows of D floats.
// ------------------------------------------------------------------------------------------------
// S[d] = <q[b], s[(b,)d]>.  Ends without a barrier.
template <int DT, bool S3D, bool PRE>
__device__ __forceinline__ void row_scores(const void* __restrict__ q, const void* __restrict__ s, int64_t b, int D, int H, float* qrow,
                                           float* S, const float* pre_slabs, int n_slabs, int64_t slab_stride) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (PRE) {
        // the contraction was done by small_gemm_kernel (MFMA) in `n_slabs` split-K slabs: summed here in slab order
        for (int d = tid; d < D; d += ML_THREADS) {
            float acc = pre_slabs[b * D + d];
            for (int z = 1; z < n_slabs; ++z) acc += pre_slabs[(int64_t)z * slab_stride + b * D + d];
            S[d] = acc;
        }
    } else {
        for (int h = tid; h < H; h += ML_THREADS) qrow[h] = ld_enc<DT>(q, b * H + h);
        __syncthreads();
        // one wavefront per section, lanes split the hidden dimension (coalesced reads of s)
        const int64_t s_base = S3D ? b * (int64_t)D * H : 0;
        for (int d = wave; d < D; d += ML_THREADS / 64) {
            const int64_t off = s_base + (int64_t)d * H;
            float acc = 0.f;
            for (int h = lane; h < H; h += 64) acc = fmaf(qrow[h], ld_enc<DT>(s, off + h), acc);
            acc = wave_sum(acc);
            if (lane == 0) S[d] = acc;
        }
    }
}

// Nn[d] = live tokens of (b, d); X[d] = the sum of their log-probs, over Nn[d] when `mean` (0 / 0 = NaN), else NaN when there is none.
// One wavefront per section, lanes split L, fixed order.  Ends without a barrier.
__device__ __forceinline__ void row_token_reduce(const float* __restrict__ tok_logp, const void* __restrict__ mask, int mask_eb,
                                                 int64_t L, int64_t b, int D, float* X, float* Nn, bool mean) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = wave; d < D; d += ML_THREADS / 64) {
        const int64_t bd = b * D + d;
        float acc = 0.f, cnt = 0.f;
        for (int64_t t = lane; t < L - 1; t += 64) {
            if (mask_live(mask, bd * L + t + 1, mask_eb)) {
                acc += tok_logp[bd * (L - 1) + t];
                cnt += 1.f;
            }
        }
        acc = wave_sum(acc);
        cnt = wave_sum(cnt);
        if (lane == 0) {
            X[d] = mean ? acc / cnt : (cnt > 0.f ? acc : __builtin_nanf(""));
            Nn[d] = cnt;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 4. VOD row kernel: the Renyi bound over the priority-sampled sections of one query row (include/vodhip.h H5v has the formulas).
//    One 256-thread workgroup per row, the same opening as marginal_row_kernel.  A section is live when it is not padded and
//    neither its log-weight nor its log-proposal c is -inf; LS[d] = -inf marks every other section, which no sum visits.
//      LS: log_weight -> ls = log_weight - logsumexp   S: r -> g = r - c -> log pi = ls + g - lZ   X: l -> lw = l + g - lZ
//    A NaN log-weight or proposal of a live section needs no test: it reaches every sum of the row, the four row words and the
//    gradients of every live section of the row (fmaxf skips it, the sums do not).
//    `eps == 0` (alpha = 1) is the same for every lane: the ELBO, and omega = exp(ls) without the product 0 * lw (lw may be -inf).
//    row_words [4, B]: Lhat, Lhat at alpha = 0, Lhat at alpha = 1, 1 / sum omega^2.
// ------------------------------------------------------------------------------------------------
template <int DT, bool S3D, bool PRE>
__global__ __launch_bounds__(ML_THREADS) void vod_row_kernel(
    const void* __restrict__ q, const void* __restrict__ s, int D, int H, const float* __restrict__ score,
    const float* __restrict__ log_weight, const float* __restrict__ log_proposal, const float* __restrict__ tok_logp,
    const void* __restrict__ mask, int mask_eb, int64_t L, float eps, float temperature, int tok_mean,
    // no `restrict` on retriever_scores: with one slab the contraction was written INTO it (read to LDS first)
    float* retriever_scores, float* __restrict__ d_scores, float* __restrict__ coef, float* __restrict__ row_words, int B,
    float inv_B, const float* pre_slabs, int n_slabs, int64_t slab_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qrow = (float*)smem;  // [H]
    float* S = qrow + H;         // [D]
    float* X = S + D;            // [D]
    float* Nn = X + D;           // [D] live tokens
    float* LS = Nn + D;          // [D]
    float* red = LS + D;         // [4]
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float ninf = -__builtin_inff(), qnan = __builtin_nanf("");

    row_scores<DT, S3D, PRE>(q, s, b, D, H, qrow, S, pre_slabs, n_slabs, slab_stride);
    row_token_reduce(tok_logp, mask, mask_eb, L, b, D, X, Nn, tok_mean != 0);
    __syncthreads();

    const float* score_row = score + b * D;
    const float* logw_row = log_weight + b * D;
    float n_live = 0.f, mx = ninf;
    for (int d = tid; d < D; d += ML_THREADS) {
        const float sc = score_row[d];
        const bool pad = __builtin_isinf(sc) && sc < 0;
        const float r = pad ? ninf : S[d];
        retriever_scores[b * D + d] = r;
        // the three words are loaded side by side (one memory latency, not two); a padded section's log-weight and proposal are then
        // dropped unseen (temperature 0 would make 0 * -inf of its score).  The product is rounded on its own: r - c is the same
        // bits whether c was passed or formed here
        const float lw_in = logw_row[d];
        const float c = log_proposal ? log_proposal[b * D + d] : __fmul_rn(temperature, sc);
        float lw = ninf, g = 0.f;
        if (!pad) {
            lw = c == ninf ? ninf : lw_in;
            g = r - c;
        }
        const bool live = !(lw == ninf);
        LS[d] = lw;
        S[d] = live ? g : 0.f;
        if (live) n_live += 1.f;
        mx = fmaxf(mx, lw);
    }
    n_live = block_sum(n_live, red);
    if (n_live == 0.f) {  // (the same for every thread) no live section: a NaN row without gradients
        for (int d = tid; d < D; d += ML_THREADS) d_scores[b * D + d] = coef[b * D + d] = 0.f;
        if (tid < 4) row_words[(int64_t)tid * B + b] = qnan;
        return;
    }
    mx = block_max(mx, red);
    float se = 0.f;
    for (int d = tid; d < D; d += ML_THREADS)
        if (!(LS[d] == ninf)) se += expf(LS[d] - mx);
    se = block_sum(se, red);
    const float lse_w = mx + logf(se);
    float amax = ninf;
    for (int d = tid; d < D; d += ML_THREADS) {
        if (LS[d] == ninf) continue;
        const float ls = LS[d] - lse_w;
        LS[d] = ls;
        amax = fmaxf(amax, ls + S[d]);
    }
    amax = block_max(amax, red);
    float ae = 0.f;
    for (int d = tid; d < D; d += ML_THREADS)
        if (!(LS[d] == ninf)) ae += expf(LS[d] + S[d] - amax);
    ae = block_sum(ae, red);
    const float lZ = amax + logf(ae);
    // u = ls + eps lw (the logits of omega) and u1 = ls + lw, with their maxima
    float umax = ninf, u1max = ninf;
    for (int d = tid; d < D; d += ML_THREADS) {
        if (LS[d] == ninf) continue;
        const float g = S[d];
        const float lw = X[d] + g - lZ;
        X[d] = lw;
        S[d] = LS[d] + g - lZ;
        umax = fmaxf(umax, eps > 0.f ? fmaf(eps, lw, LS[d]) : LS[d]);  // (fmaxf skips NaN: the sums below do not)
        u1max = fmaxf(u1max, LS[d] + lw);
    }
    umax = block_max(umax, red);
    u1max = block_max(u1max, red);
    float t1 = 0.f, t2 = 0.f, t_iw = 0.f, s_elbo = 0.f;
    for (int d = tid; d < D; d += ML_THREADS) {
        if (LS[d] == ninf) continue;
        const float lw = X[d];
        const float e = expf((eps > 0.f ? fmaf(eps, lw, LS[d]) : LS[d]) - umax);
        t1 += e;
        t2 = fmaf(e, e, t2);
        t_iw += expf(LS[d] + lw - u1max);
        s_elbo = fmaf(expf(LS[d]), lw, s_elbo);
    }
    t1 = block_sum(t1, red);
    t2 = block_sum(t2, red);
    t_iw = block_sum(t_iw, red);
    s_elbo = block_sum(s_elbo, red);
    // Lhat = m + log1p(sum exp(ls) expm1(eps (lw - m))) / eps holds for EVERY shift m.  With m = max lw the sum can sit next to -1
    // (little weight on the best section) and log1p multiplies its rounding error by 1 / (1 + sum); with m = the plain
    // log-sum-exp value of the bound - exact to an ulp of u over eps - the sum is ~ 0 and what is left is the correction that the
    // plain form loses as eps -> 0.  exp(ls) expm1(x) is formed as exp(ls + x) - exp(ls) where |x| >= 1: no cancellation there, and
    // no overflow of exp(x) alone.
    const float l_iw = u1max + logf(t_iw);
    float l_hat = s_elbo;
    if (eps > 0.f) {
        const float m = (umax + logf(t1)) / eps;
        float s_eps = 0.f;
        for (int d = tid; d < D; d += ML_THREADS) {
            if (LS[d] == ninf) continue;
            const float x = eps * (X[d] - m);
            s_eps += fabsf(x) < 1.f ? expf(LS[d]) * expm1f(x) : expf(LS[d] + x) - expf(LS[d]);
        }
        s_eps = block_sum(s_eps, red);
        l_hat = m + log1pf(s_eps) / eps;
    }
    for (int d = tid; d < D; d += ML_THREADS) {
        float ds = 0.f, cf = 0.f;
        if (!(LS[d] == ninf)) {
            const float omega = expf((eps > 0.f ? fmaf(eps, X[d], LS[d]) : LS[d]) - umax) / t1;
            ds = -(omega - expf(S[d])) * inv_B;
            cf = -omega * inv_B;
            if (tok_mean) cf /= Nn[d];
        }
        d_scores[b * D + d] = ds;
        coef[b * D + d] = cf;
    }
    if (tid == 0) {
        row_words[b] = l_hat;
        row_words[(int64_t)B + b] = l_iw;
        row_words[2 * (int64_t)B + b] = s_elbo;
        row_words[3 * (int64_t)B + b] = t1 * t1 / t2;
    }
}

// loss = -mean Lhat ; diag = means of the other three row words
__global__ __launch_bounds__(ML_THREADS) void vod_finalize_kernel(const float* __restrict__ row_words, int B, float* __restrict__ loss,
                                                                  float* __restrict__ diag) {
    __shared__ float red[4];
    float part[4] = {0.f, 0.f, 0.f, 0.f};  // the four loads of a thread go out together
    for (int b = threadIdx.x; b < B; b += ML_THREADS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[k] += row_words[(int64_t)k * B + b];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float acc = block_sum(part[k], red);
        if (threadIdx.x == 0) {
            if (k == 0) loss[0] = -acc / (float)B;
            else diag[k - 1] = acc / (float)B;
        }
    }
}

// 16-byte accesses need every row base on a 16-byte boundary: the tensor's and a row's pitch
static bool rows_aligned(const void* p, int64_t V, int dtype) {
    const int64_t es = dtype == 2 ? 4 : 2;
    return ((uintptr_t)p % 16 == 0) && (V * es % 16 == 0);
}

hipError_t launch_lm_token_forward(const void* logits, int dtype, int64_t N, int64_t L, int64_t V, const int64_t* ids,
                                   const void* mask, int mask_eb, float* tok_logp, float* tok_lse, hipStream_t stream) {
    const int vec = rows_aligned(logits, V, dtype) ? 1 : 0;
    const int64_t row_vecs = (V * (dtype == 2 ? 4 : 2) + 15) / 16;
    const dim3 grid((unsigned)(N * (L - 1)));
#define VOD_TF(DT, T)                                                                                                    \
    if (dtype == DT && (row_vecs <= ML_WAVE_ROW_VECS) == (T == 64)) {                                                    \
        hipLaunchKernelGGL((lm_token_forward_kernel<DT, T>), grid, dim3(T), 0, stream, logits, L, V, ids, mask, mask_eb, \
                           vec, tok_logp, tok_lse);                                                                      \
        return hipGetLastError();                                                                                        \
    }
    VOD_TF(0, 64) VOD_TF(0, ML_THREADS) VOD_TF(1, 64) VOD_TF(1, ML_THREADS) VOD_TF(2, 64) VOD_TF(2, ML_THREADS)
#undef VOD_TF
    return hipErrorInvalidValue;
}

hipError_t launch_lm_token_backward(const void* logits, int dtype, int64_t N, int64_t L, int64_t V, const int64_t* ids,
                                    const void* mask, int mask_eb, const float* tok_lse, const float* coef, const float* grad_out,
                                    void* d_logits, hipStream_t stream) {
    const int vec = (rows_aligned(logits, V, dtype) && rows_aligned(d_logits, V, dtype)) ? 1 : 0;
    const int64_t row_vecs = (V * (dtype == 2 ? 4 : 2) + 15) / 16;
    const dim3 grid((unsigned)(N * L));
#define VOD_TB(DT, T)                                                                                                     \
    if (dtype == DT && (row_vecs <= ML_WAVE_ROW_VECS) == (T == 64)) {                                                     \
        hipLaunchKernelGGL((lm_token_backward_kernel<DT, T>), grid, dim3(T), 0, stream, logits, L, V, ids, mask, mask_eb, \
                           vec, tok_lse, coef, grad_out, d_logits);                                                       \
        return hipGetLastError();                                                                                         \
    }
    VOD_TB(0, 64) VOD_TB(0, ML_THREADS) VOD_TB(1, 64) VOD_TB(1, ML_THREADS) VOD_TB(2, 64) VOD_TB(2, ML_THREADS)
#undef VOD_TB
    return hipErrorInvalidValue;
}

hipError_t launch_marginal_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                                   const float* score, const float* tok_logp, const void* mask, int mask_eb, int64_t L,
                                   float* retriever_scores, float* d_scores, float* coef, float* loss, float* workspace,
                                   int64_t workspace_floats, hipStream_t stream) {
    const size_t lds = (size_t)(H + 3 * D + 4) * sizeof(float);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const float inv_B = 1.f / (float)B;
    float* row_lpx = workspace;  // [B]
    hipError_t e;
    if (!sections_3d) {
        // einsum("bh,dh->bd") on the MFMA GEMM of the retrieval loss; K split into 4 slabs behind the row words when the workspace
        // has room (launch_retrieval_forward explains the split), else one slab: retriever_scores itself
        int n_splits = 1;
        float* slabs = retriever_scores;
        if (H >= 512 && workspace_floats >= B + 4 * B * D) {
            n_splits = 4;
            slabs = workspace + B;
        }
        e = launch_small_gemm(enc_dtype, enc_dtype, q, H, 1, s, 1, H, slabs, D, (int)B, (int)D, (int)H, nullptr, stream, n_splits, B * D);
        if (e != hipSuccess) return e;
#define VOD_MRP(DT)                                                                                                          \
    if (enc_dtype == DT) {                                                                                                   \
        auto kern = marginal_row_kernel<DT, false, true>;                                                                    \
        e = allow_dynamic_lds((const void*)kern, 160 * 1024);                                                                \
        if (e != hipSuccess) return e;                                                                                       \
        hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(ML_THREADS), lds, stream, q, s, (int)D, (int)H, score, tok_logp,    \
                           mask, mask_eb, L, retriever_scores, d_scores, coef, row_lpx, inv_B, (const float*)slabs, n_splits, \
                           B * D);                                                                                           \
    }
        VOD_MRP(0) VOD_MRP(1) VOD_MRP(2)
#undef VOD_MRP
    } else {
#define VOD_MR(DT)                                                                                                        \
    if (enc_dtype == DT) {                                                                                                \
        auto kern = marginal_row_kernel<DT, true, false>;                                                                 \
        e = allow_dynamic_lds((const void*)kern, 160 * 1024);                                                             \
        if (e != hipSuccess) return e;                                                                                    \
        hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(ML_THREADS), lds, stream, q, s, (int)D, (int)H, score, tok_logp, \
                           mask, mask_eb, L, retriever_scores, d_scores, coef, row_lpx, inv_B, (const float*)nullptr, 0,  \
                           (int64_t)0);                                                                                   \
    }
        VOD_MR(0) VOD_MR(1) VOD_MR(2)
#undef VOD_MR
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(marginal_finalize_kernel, dim3(1), dim3(ML_THREADS), 0, stream, row_lpx, (int)B, loss);
    return hipGetLastError();
}

hipError_t launch_vod_forward(const void* q, const void* s, int enc_dtype, int sections_3d, int64_t B, int64_t D, int64_t H,
                              const float* score, const float* log_weight, const float* log_proposal, const float* tok_logp,
                              const void* mask, int mask_eb, int64_t L, float eps, float temperature, int tok_mean,
                              float* retriever_scores, float* d_scores, float* coef, float* loss, float* diag, float* workspace,
                              int64_t workspace_floats, hipStream_t stream) {
    const size_t lds = (size_t)(H + 4 * D + 4) * sizeof(float);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const float inv_B = 1.f / (float)B;
    float* row_words = workspace;  // [4, B]
    hipError_t e;
    // the contraction of 2-D sections as in launch_marginal_forward: four split-K slabs behind the row words, or retriever_scores
    int n_splits = 1;
    float* slabs = retriever_scores;
    if (!sections_3d) {
        if (H >= 512 && workspace_floats >= 4 * B + 4 * B * D) {
            n_splits = 4;
            slabs = workspace + 4 * B;
        }
        e = launch_small_gemm(enc_dtype, enc_dtype, q, H, 1, s, 1, H, slabs, D, (int)B, (int)D, (int)H, nullptr, stream, n_splits, B * D);
        if (e != hipSuccess) return e;
    }
#define VOD_VR(DT, S3D, PRE)                                                                                               \
    if (enc_dtype == DT && (sections_3d != 0) == S3D) {                                                                    \
        auto kern = vod_row_kernel<DT, S3D, PRE>;                                                                          \
        e = allow_dynamic_lds((const void*)kern, 160 * 1024);                                                              \
        if (e != hipSuccess) return e;                                                                                     \
        hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(ML_THREADS), lds, stream, q, s, (int)D, (int)H, score, log_weight, \
                           log_proposal, tok_logp, mask, mask_eb, L, eps, temperature, tok_mean, retriever_scores, d_scores, \
                           coef, row_words, (int)B, inv_B, (const float*)(PRE ? slabs : nullptr), PRE ? n_splits : 0,      \
                           PRE ? B * D : (int64_t)0);                                                                      \
    }
    VOD_VR(0, true, false) VOD_VR(1, true, false) VOD_VR(2, true, false)
    VOD_VR(0, false, true) VOD_VR(1, false, true) VOD_VR(2, false, true)
#undef VOD_VR
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vod_finalize_kernel, dim3(1), dim3(ML_THREADS), 0, stream, row_words, (int)B, loss, diag);
    return hipGetLastError();
}

}  // namespace vodhip
