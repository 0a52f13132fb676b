"""Float64 restatement of `HipFlatIndex.posterior_expectation` (include/vodhip.h H2e, vod_amd/csrc/kernels_readout.hip):

1. rows and queries are rounded to the store dtype, scores and (max, log_rel) are those of `partition_ref`;
2. the weights p(z | q) are `posterior_ref.weights`: exp(beta (s_z - max) - log_rel) over the eligible rows whose score is not NaN;
3. the value table is rounded to the store dtype with `l2_ref.round_store`; values = p @ v~; a query with no finite log Z gets the
   zero row.

`device_bound` is the derived bound on |device value - float64 value| per (query, column) ("Posterior read-out"); it is
not fitted to what the device returns."""
import numpy as np

import partition_ref as P
import posterior_ref as M
from l2_ref import round_store

U = P.U
GROUP_ROWS = 4096                       # VODHIP_READOUT_GROUP_ROWS: rows whose value accumulator shares one running maximum
TILE_ROWS = 256
GROUP_TILES = GROUP_ROWS // TILE_ROWS
EPS16 = M.EPS16
FP16_KEPT = M.FP16_KEPT


def posterior_expectation(q, x, v, dtype, beta, eligible=None):
    """(values [nq, n_cols], max [nq], log_rel [nq]) in float64.  Table rows that carry weight 0 do not enter (a non-finite value in
    such a row does not spread here: the device's NaN-column contract is tested on its own)."""
    v = np.asarray(v, dtype=np.float32)
    v = v.reshape(-1, 1) if v.ndim == 1 else v
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    if len(x) == 0:
        return np.zeros((len(q), v.shape[1])), np.full(len(q), -np.inf), np.full(len(q), -np.inf)
    p, m, r = M.weights(P.scores(q, x, dtype), beta, eligible)
    vr = round_store(v, dtype)
    used = (p > 0).any(axis=0)
    return p[:, used] @ vr[used], m, r


def rel_bound(q, x, dtype, beta, n_eligible, n_rows, eligible=None, dot=True) -> np.ndarray:
    """[nq]: (1 + eps16)(1 + delta) - 1 of `device_bound` for n_eligible rows in a store of n_rows"""
    nq = np.shape(q)[0]
    n = np.maximum(np.asarray(n_eligible, dtype=np.float64), 1.0) + np.zeros(nq)
    E = P.dot_bound(q, x, dtype, eligible) if dot else np.zeros(nq)
    PB = P.device_bound(q, x, dtype, beta, n, dot=dot)
    groups = (n_rows + GROUP_ROWS - 1) // GROUP_ROWS
    k = n + groups + 3
    resc = GROUP_TILES - 1                       # at most one rescale per tile of a group behind the tile that set the accumulator
    # the exponents of e, of gamma, of the rescales (they telescope: same sign, sum <= ARG_MAX where the weight matters) and of the finish
    arg = 3 * 2.0001 * P.ARG_MAX * U + (2.0001 * P.ARG_MAX + P.ARG_MAX + np.log(n)) * U
    expf = (1 + 2 * P.EXP_ULP * U) ** (3 + resc)  # e, gamma, the finish coefficient, the rescales
    prod = (1 + U) ** (2 + resc)                 # e * gamma, coefficient * accumulator, the rescales
    delta = np.exp(2 * beta * E + PB + arg) * expf * prod * (1 + k * U / (1 - k * U)) - 1
    return (1 + EPS16[dtype]) * (1 + delta) - 1


def device_bound(q, x, v, dtype, beta, eligible=None, dot=True) -> np.ndarray:
    """[nq, n_cols] bound on |device value - float64 value|:  ((1 + eps16)(1 + delta) - 1) * S + floor,  S = sum_z p_z |v~_zc|.

    `posterior_ref.device_bound` with the value table in place of the rows in S and in the floor, and the read-out's own weight:
    the device's weight of row z of tile t of group g is
        c_g * prod_k r_k * P'_z,   P'_z = round16(fl(e_z * gamma_t)),   e_z = expf(fl(beta * fl(s_z - m_t))),
        gamma_t = expf(fl(beta * fl(m_t - M))) (1 when the tile raised the running maximum M),
        r_k = expf(fl(beta * fl(M_old - M_new))) for every later tile of the group that raised M,
        c_g = expf(fl(fl(beta * fl(M_g - max)) - log_rel));
    in exact arithmetic the exponents add up to beta s_z - log Z.  u = 2^-24, n = eligible rows, E = `partition_ref.dot_bound`,
    PB = `partition_ref.device_bound`, T = GROUP_TILES.

    eps16  P' is rounded once to the store dtype: 2^-11 (fp16, a normal number: see floor) or 2^-8 (bf16), relative.
    score  as `posterior_ref`: the exponent moves by at most 2 beta E + PB.  `dot=False` drops E.
    arg    every argument is two roundings of a product, relative 2 u + u^2.  |beta (s - m_t)| <= 104 and |beta (m_t - M)| <= 104
           matter (below, the weight is under 2^-149 of its reference: tiny).  The rescale arguments all have the same sign and add up
           to beta (M_first - M_g): their rounding errors add up to 2.0001 * 104 u where the row matters (tiny otherwise).  The finish
           as `posterior_ref`: (2.0001 * 104 + 104 + log n) u.
    exp    expf is 1 ulp = 2 u relative: e, gamma, c_g and at most T - 1 rescales (one per tile behind the one that holds the row).
    prod   one rounding each (u): e * gamma, c_g * acc_g, and the T - 1 rescales of the accumulator.
    sum    the float32 sum of one column's terms - n rows on the MFMA, 3 wave additions, one addition per group - is within
           gamma_k = k u / (1 - k u) of sum |terms|, k = n + groups + 3.  (A rescale multiplies a partial sum: its rounding is in prod.)
    floor  fp16: a weight below 2^-29 of the running maximum's weight (= 1) is subnormal after the 2^15 scale and may be rounded
           coarsely or flushed: at most 2^-29 per row in units that later rescales (<= 1) only shrink, GROUP_ROWS rows per group, and
           the group weights c_g sum to at most 1 (+ rounding, 1.001): GROUP_ROWS * 2^-29 * max_z |v~_zc|.  bf16: zero.
    tiny   weights under 2^-126 (float32 / bf16 subnormals, arguments below -104): n * 2^-126 * max |v~_zc|, both dtypes."""
    v = np.asarray(v, dtype=np.float32)
    v = v.reshape(-1, 1) if v.ndim == 1 else v
    qr, xr, vr = round_store(q, dtype), round_store(x, dtype), round_store(v, dtype)
    n_rows = xr.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = qr @ xr.T
    p, m, _ = M.weights(s, beta, eligible)
    keep = ~np.isnan(s) if eligible is None else (np.asarray(eligible) & ~np.isnan(s))
    n = np.maximum(keep.sum(axis=1), 1).astype(np.float64)
    absv = np.abs(np.where(np.isfinite(vr), vr, 0.0))
    S = p @ absv                                                    # [nq, n_cols]
    vmax = absv.max(axis=0) if n_rows else np.zeros(vr.shape[1])    # [n_cols]
    rel = rel_bound(q, x, dtype, beta, n, n_rows, eligible, dot)    # [nq]
    floor = (GROUP_ROWS * FP16_KEPT * 1.001 if dtype == "float16" else 0.0) * vmax + n.max() * 2.0 ** -126 * vmax
    return rel[:, None] * S + floor[None, :]
