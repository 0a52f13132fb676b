"""Float64 restatement of `HipFlatIndex.posterior_mean` (include/vodhip.h H2m, vod_amd/csrc/kernels_posterior.hip):

1. rows and queries are rounded to the store dtype, scores and (max, log_rel) are those of `partition_ref`;
2. p(z | q) = exp(beta (s_z - max) - log_rel) over the eligible rows whose score is not NaN, 0 elsewhere;
3. mean = p @ x~; a query with no finite log Z gets the zero row.

`device_bound` is the derived bound on |device mean - float64 mean| per (query, column) ("Posterior mean"); it is not
fitted to what the device returns."""
import numpy as np

import partition_ref as P
from l2_ref import round_store

U = P.U
GROUP_ROWS = 16384                      # VODHIP_POSTERIOR_GROUP_ROWS: rows that share one reference maximum
EPS16 = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}   # unit roundoff of the store dtype: the one rounding of a weight
FP16_KEPT = 2.0 ** -29                  # fp16: a weight is a normal number down to this fraction of its group's largest


def weights(s, beta, eligible=None):
    """float64 [nq, n]: p(z | q); rows of queries without a finite log Z are zero.  Also returns (max, log_rel)."""
    s = np.asarray(s, dtype=np.float64)
    m, r = P.from_scores(s, beta, eligible)
    keep = ~np.isnan(s)
    if eligible is not None:
        keep &= eligible
    live = np.isfinite(m)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.exp(beta * (s - np.where(live, m, 0.0)[:, None]) - np.where(live, r, 0.0)[:, None])
    p = np.where(keep & live[:, None], p, 0.0)
    return p, m, r


def posterior_mean(q, x, dtype, beta, eligible=None):
    """(mean [nq, dim], max [nq], log_rel [nq]) in float64.  Rows that carry weight 0 do not enter (a non-finite value in such a row
    does not spread here: the device's NaN-column contract is tested on its own)."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    if len(x) == 0:
        return np.zeros((len(q), np.shape(x)[1])), np.full(len(q), -np.inf), np.full(len(q), -np.inf)
    p, m, r = weights(P.scores(q, x, dtype), beta, eligible)
    xr = round_store(x, dtype)
    used = (p > 0).any(axis=0)
    return p[:, used] @ xr[used], m, r


def rel_bound(q, x, dtype, beta, n_eligible, n_rows, eligible=None, dot=True) -> np.ndarray:
    """[nq]: (1 + eps16)(1 + delta) - 1 of `device_bound` for n_eligible rows in a store of n_rows"""
    nq = np.shape(q)[0]
    n = np.maximum(np.asarray(n_eligible, dtype=np.float64), 1.0) + np.zeros(nq)
    E = P.dot_bound(q, x, dtype, eligible) if dot else np.zeros(nq)
    PB = P.device_bound(q, x, dtype, beta, n, dot=dot)
    groups = (n_rows + GROUP_ROWS - 1) // GROUP_ROWS
    k = n + groups + 3
    arg = 2.0001 * P.ARG_MAX * U + (2.0001 * P.ARG_MAX + P.ARG_MAX + np.log(n)) * U
    delta = np.exp(2 * beta * E + PB + arg) * (1 + 2 * P.EXP_ULP * U) ** 2 * (1 + U) * (1 + k * U / (1 - k * U)) - 1
    return (1 + EPS16[dtype]) * (1 + delta) - 1


def device_bound(q, x, dtype, beta, eligible=None, dot=True) -> np.ndarray:
    """[nq, dim] bound on |device mean - float64 mean|:  ((1 + eps16)(1 + delta) - 1) * S + floor,  S = sum_z p_z |x~_zi|.

    The device's weight of row z of group g is c_g * P'_z with P'_z = round16(expf(fl(beta * fl(s_z - m_g)))) and
    c_g = expf(fl(fl(beta * fl(m_g - max)) - log_rel)); in exact arithmetic the two exponents add up to beta s_z - log Z.
    u = 2^-24, n = eligible rows, E = `partition_ref.dot_bound`, PB = `partition_ref.device_bound`.

    eps16  P' is rounded once to the store dtype: 2^-11 (fp16, a normal number: see floor) or 2^-8 (bf16), relative.
    score  s_z is within E of its float64 value, max_score too, and log_rel within PB (which holds its own 2 beta E):
           the exponent moves by at most 2 beta E + PB, the weight by a factor exp(+-(2 beta E + PB)).  `dot=False` drops E.
    arg    tile: t = fl(beta * fl(s - m_g)), relative 2 u + u^2, |t| <= 104 matters (below, both weights are under 2^-149: tiny).
           finish: fl(m_g - max) and its product with beta round (2 u + u^2 of at most 104), the subtraction of log_rel <= log n
           rounds once more (u of at most 104 + log n): the argument moves by at most (2.0001 * 104 + 104 + log n) u.
    exp    expf is 1 ulp = 2 u relative, in the tile and in the finish; the product c_g * acc_g rounds once (u).
    sum    the float32 sum of one column's terms in any order - n rows on the MFMA, 3 wave additions, one addition per group -
           is within gamma_k = k u / (1 - k u) of sum |terms|, k = n + groups + 3.
    floor  fp16: a weight below 2^-29 of its group's largest is subnormal after the 2^15 scale and may be rounded coarsely or flushed:
           at most 2^-29 per row in units of the group's largest weight (= 1), GROUP_ROWS rows per group, and the group weights c_g
           sum to at most 1 (+ their own rounding, 1.001): GROUP_ROWS * 2^-29 * max_z |x~_zi|.  bf16: zero.
    tiny   weights under 2^-126 (float32 / bf16 subnormals, arguments below -104): n * 2^-126 * max |x~_zi|, both dtypes."""
    qr, xr = round_store(q, dtype), round_store(x, dtype)
    nq, n_rows = qr.shape[0], xr.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = qr @ xr.T
    p, m, _ = weights(s, beta, eligible)
    keep = ~np.isnan(s) if eligible is None else (np.asarray(eligible) & ~np.isnan(s))
    n = np.maximum(keep.sum(axis=1), 1).astype(np.float64)
    absx = np.abs(np.where(np.isfinite(xr), xr, 0.0))
    S = p @ absx                                                    # [nq, dim]
    xmax = absx.max(axis=0) if n_rows else np.zeros(xr.shape[1])    # [dim]
    rel = rel_bound(q, x, dtype, beta, n, n_rows, eligible, dot)  # [nq]
    floor = (GROUP_ROWS * FP16_KEPT * 1.001 if dtype == "float16" else 0.0) * xmax + n.max() * 2.0 ** -126 * xmax
    return rel[:, None] * S + floor[None, :]
