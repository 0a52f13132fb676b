"""Float64 restatement of `HipFlatIndex.log_partition` (include/vodhip.h H2p, vod_amd/csrc/kernels_partition.hip):

1. rows and queries are rounded to the store dtype (`l2_ref.round_store`: round-to-nearest-even, finite values beyond its range saturate);
2. s = <q~, x~_z> in float64 for every row z;
3. a row counts when `eligible` allows it and its score is not NaN;
4. max = the largest score, log_rel = log sum exp(beta (s - max)); no row: (-inf, -inf); a +inf score: (+inf, +inf); scores that are
   all -inf count as no row.

`device_bound` is the derived bound on |device log_rel - float64 log_rel| ("Log-partition scan"), `max_bound` the one on
|device max_score - float64 max|; neither is fitted to what the device returns."""
import numpy as np

from l2_ref import round_store

U = 2.0 ** -24            # unit roundoff of float32
EXP_ULP = 1.0             # expf: 1 ulp (HIP math API accuracy table, single precision)
LOG_ULP = 1.0             # logf: 1 ulp (same table)
ARG_MAX = 104.0           # exp(t) is below the smallest float32 subnormal for t < -103.98: such terms are below 2^-149 on both sides


def scores(q, x, dtype) -> np.ndarray:
    """float64 [nq, n]: inner products of the rounded queries and rows"""
    qr, xr = round_store(q, dtype), round_store(x, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return qr @ xr.T


def from_scores(s, beta, eligible=None):
    """(max [nq], log_rel [nq]) in float64 from a score matrix"""
    s = np.asarray(s, dtype=np.float64)
    nq = s.shape[0]
    out_m = np.full(nq, -np.inf)
    out_r = np.full(nq, -np.inf)
    for a in range(nq):
        row = s[a]
        keep = ~np.isnan(row)
        if eligible is not None:
            keep &= eligible[a]
        v = row[keep]
        if v.size == 0 or v.max() == -np.inf:
            continue
        m = v.max()
        out_m[a] = m
        out_r[a] = np.inf if m == np.inf else np.log(np.exp(beta * (v - m)).sum())
    return out_m, out_r


def log_partition(q, x, dtype, beta, eligible=None):
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    if len(x) == 0:
        return np.full(len(q), -np.inf), np.full(len(q), -np.inf)
    return from_scores(scores(q, x, dtype), beta, eligible)


def dot_bound(q, x, dtype, eligible=None) -> np.ndarray:
    """[nq]: the any-order float32 bound of a dim_pad-term dot product (the products of two 16-bit values are exact in float32, the
    dim_pad - 1 additions round), gamma = k u / (1 - k u) with k = dim_pad, times the largest sum |q~_i x~_zi| over the query's rows"""
    qr, xr = round_store(q, dtype), round_store(x, dtype)
    k = (xr.shape[1] + 63) // 64 * 64
    absdot = np.abs(qr) @ np.abs(xr).T
    if eligible is not None:
        absdot = np.where(eligible, absdot, 0.0)
    return (k * U / (1 - k * U)) * absdot.max(axis=1)


def max_bound(q, x, dtype, eligible=None) -> np.ndarray:
    """[nq] bound on |device max_score - float64 max|: every device score is within `dot_bound` of its float64 value, so the maxima are"""
    return dot_bound(q, x, dtype, eligible)


def device_bound(q, x, dtype, beta, n_eligible, dot=True) -> np.ndarray:
    """[nq] bound on |device log_rel - float64 log_rel|, four parts (u = 2^-24, n = eligible rows, E = `dot_bound`):

    dot    every score moves by at most E and so does the maximum: log sum exp(beta s) moves by at most beta E, beta * max too: 2 beta E.
           `dot=False` (scores that are exact in float32) drops it.
    arg    t = fl(beta * fl(s - m)) has relative error 2 u + u^2; for |t| <= 104 the term exp(t) moves by a factor within
           exp(+-208.1 u); below -104 both the device's and the true term are under 2^-149 (n 2^-148 in all, against a sum >= 1).
           Twice: once in the tile (s - tile max), once in the finish (tile max - max).
    exp    expf is 1 ulp (relative 2 u) - twice, as above - and the product l_t * exp(..) rounds once (u).  logf is 1 ulp of the
           result: 2 u log n, since 0 <= log_rel <= log n.
    sum    the sum of n non-negative float32 terms in any order: relative (n - 1) u / (1 - (n - 1) u).  (Adding the +0 of an
           ineligible row or of an empty tile is exact, so only the n real terms count.)
    The relative error r of the sum becomes |log(1 + r)| <= r / (1 - r) in log_rel."""
    n = np.maximum(np.asarray(n_eligible, dtype=np.float64), 1.0)
    rel = 2 * (np.exp(2.0001 * ARG_MAX * U) - 1) + 2 * EXP_ULP * 2 * U + U + (n - 1) * U / (1 - (n - 1) * U)
    rel = rel * (1 + rel)  # the parts compound: (1 + a)(1 + b) - 1 <= (a + b)(1 + a + b)
    out = rel / (1 - rel) + LOG_ULP * 2 * U * np.log(n) * (1 + 2 * U) + n * 2.0 ** -148
    if dot:
        out = out + 2 * beta * dot_bound(q, x, dtype)
    return out + np.zeros(np.shape(q)[0])


def coverage(s, k, beta, eligible=None) -> np.ndarray:
    """float64 [nq]: log of the posterior mass of the k best eligible rows, logsumexp(beta * topk) - log Z"""
    s = np.asarray(s, dtype=np.float64)
    m, r = from_scores(s, beta, eligible)
    out = np.empty(s.shape[0])
    for a in range(s.shape[0]):
        v = s[a][~np.isnan(s[a]) if eligible is None else (~np.isnan(s[a]) & eligible[a])]
        top = np.sort(v)[::-1][:k]
        out[a] = np.log(np.exp(beta * (top - m[a])).sum()) - r[a]
    return out
