"""Float64 restatement of `HipFlatIndex.posterior_adjoint` (include/vodhip.h H2a, vod_amd/csrc/kernels_readout_adjoint.hip):

1. rows and queries are rounded to the store dtype, scores and (max, log_rel) are those of `partition_ref`;
2. the weights p(z | q) are `posterior_ref.weights`: exp(beta (s_z - max) - log_rel) over the eligible rows whose score is not NaN,
   zero for a query without a finite log Z;
3. out = p.T @ W with W as given (float32 values in float64): the device's one rounding of the normalised W is part of the bound.

`device_bound` is the derived bound on |device value - float64 value| per (row, column) ("Read-out adjoint"); it is not
fitted to what the device returns."""
import numpy as np

import partition_ref as P
import posterior_ref as M
import readout_ref as R
from l2_ref import round_store

U = P.U
EPS16 = M.EPS16
FP16_KEPT = M.FP16_KEPT
SLICE = 1024                            # queries of one scan launch: later slices add to the result


def _weights(w, nq):
    w = np.asarray(w, dtype=np.float32)
    w = w.reshape(-1, 1) if w.ndim == 1 else w
    assert w.shape[0] == nq
    return w


def posterior_adjoint(q, x, w, dtype, beta, eligible=None):
    """(out [n, n_cols], max [nq], log_rel [nq]) in float64; a dead query (no finite log Z) weighs 0"""
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    w = _weights(w, len(q))
    if len(x) == 0:
        return np.zeros((0, w.shape[1])), np.full(len(q), -np.inf), np.full(len(q), -np.inf)
    p, m, r = M.weights(P.scores(q, x, dtype), beta, eligible)
    used = (p > 0).any(axis=1)  # (a W row that weighs 0 does not enter: the NaN-column contract is tested on its own)
    return p[used].T @ w[used].astype(np.float64), m, r


def row_mass(q, x, dtype, beta, eligible=None, query_weights=None):
    w = np.ones(len(q), dtype=np.float32) if query_weights is None else query_weights
    return posterior_adjoint(q, x, w, dtype, beta, eligible)[0][:, 0]


def column_exponents(w) -> np.ndarray:
    """[n_cols] k_c = floor(log2 max_q |W[q, c]|) over the whole batch, 0 for an all-zero (or empty) column"""
    w = np.asarray(w, dtype=np.float32)
    w = w.reshape(-1, 1) if w.ndim == 1 else w
    amax = np.abs(w).max(axis=0) if w.shape[0] else np.zeros(w.shape[1], dtype=np.float32)
    _, e = np.frexp(amax.astype(np.float64))  # amax = f 2^e, 1/2 <= f < 1
    return np.where(amax > 0, e - 1, 0).astype(np.int64)


def staging(w, dtype):
    """(k [n_cols], W^ [nq, n_cols] float64 in units of 2^k_c after the one rounding, werr [nq, n_cols] the bound on that rounding)"""
    w = np.asarray(w, dtype=np.float32)
    w = w.reshape(-1, 1) if w.ndim == 1 else w
    k = column_exponents(w)
    wn = np.ldexp(w.astype(np.float64), -k[None, :])
    w_hat = round_store(wn.astype(np.float32), dtype).astype(np.float64)  # (|wn| < 2 and a float32 times a power of two: the cast is exact)
    least = 2.0 ** -25 if dtype == "float16" else 2.0 ** -134  # half the spacing of the 16-bit subnormals
    werr = np.where(w_hat == wn, 0.0, np.maximum(EPS16[dtype] * np.abs(wn), least))
    return k, w_hat, werr


def device_bound(q, x, w, dtype, beta, eligible=None, dot=True, rel_extra=0.0) -> np.ndarray:
    """[n, n_cols] bound on |device value - float64 value|, in units of 2^k_c per column (k_c = `column_exponents`, W' = W 2^-k_c):

        2^k_c * ( sum_q p_qz [ ((1 + rel_q)(1 + g) - 1) |W'_qc| + (1 + rel_q)(1 + g) werr_qc ] + floor_c + tiny_c )

    The device's weight of (query q, row z) is P' = round16(expf(fl(fl(min(0, fl(beta fl(s - max_q)))) - log_rel_q))), ONE exponential
    whose argument is in exact arithmetic beta s - log Z; (max_q, log_rel_q) are the device's forward words.

    rel_q  `readout_ref.rel_bound`: the one 16-bit rounding of the weight (eps16), the score and the two words (2 beta E + PB), the
           roundings of the argument, expf (the read-out has more of each: its bound holds here a fortiori), and a float32 sum over the
           query's eligible rows that does not happen here (slack).  `dot=False` drops E.  `rel_extra` (per query or scalar): what a node
           index's folded log_rel adds to the exponent, as a factor exp(rel_extra).
    g      the float32 sum of one element's terms - nq queries on the MFMA, 3 wave additions, one addition per further slice of 1024
           queries - is within gamma_k = k u / (1 - k u) of sum |terms|, k = nq + 3 + slices.  The final 2^k_c (and 2^-15) is exact.
    werr   the one rounding of W' to the store dtype: eps16 |W'_qc|; for fp16 at least 2^-25 (|W'| < 2^-14 is subnormal), i. e.
           2^(k_c - 25) in the output's units; ZERO when W' is exact in 16 bits.
    floor  fp16: a weight below 2^-29 is subnormal after the 2^15 scale and may be rounded coarsely or flushed: at most 2^-29 per query,
           FP16_KEPT * sum_q |W'_qc| (the read-out's nq * FP16_KEPT * max in its tighter form).  bf16: zero.
    tiny   weights under 2^-126 (float32 / bf16 subnormals, arguments below -104): nq * 2^-126 * max_q |W'_qc|, both dtypes."""
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    nq = len(q)
    w = _weights(w, nq)
    k, w_hat, werr = staging(w, dtype)
    n_rows = np.shape(x)[0]
    if n_rows == 0:
        return np.zeros((0, w.shape[1]))
    qr, xr = round_store(q, dtype), round_store(x, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        s = qr @ xr.T
    p, _, _ = M.weights(s, beta, eligible)
    keep = ~np.isnan(s) if eligible is None else (np.asarray(eligible) & ~np.isnan(s))
    n = np.maximum(keep.sum(axis=1), 1).astype(np.float64)
    rel = (1 + R.rel_bound(q, x, dtype, beta, n, n_rows, eligible, dot)) * np.exp(np.asarray(rel_extra, dtype=np.float64) + np.zeros(nq))  # [nq]
    kk = nq + 3 + (nq + SLICE - 1) // SLICE
    g = 1 + kk * U / (1 - kk * U)
    wn = np.abs(np.ldexp(np.where(np.isfinite(w), w, 0).astype(np.float64), -k[None, :]))
    per_q = (rel[:, None] * g - 1) * wn + rel[:, None] * g * werr   # [nq, n_cols]
    floor = (FP16_KEPT * wn.sum(axis=0) if dtype == "float16" else 0.0) + nq * 2.0 ** -126 * (wn.max(axis=0) if nq else 0.0)
    return np.ldexp(p.T @ per_q + floor[None, :], k[None, :])
