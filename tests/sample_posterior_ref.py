"""Float64 restatement of `HipFlatIndex.sample_posterior` (include/vodhip.h H2s, vod_amd/csrc/kernels_sample_posterior.hip).  This file
IS the noise contract:

1. rows and queries are rounded to the store dtype, s = <q~, x~_z> in float64 (`partition_ref.scores`), a row counts when `eligible`
   allows it and its score is not NaN;
2. Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter (low word of g >> 2, g >> 34, qs, j), g = id_base + row,
   qs = query_offset + query: output word g & 3 of the call with j = 0 is w_hi, with j = 1 it is w_lo;
3. v = (w_hi 2^32 + w_lo + 1/2) 2^-64, at most 1 - 2^-24;  E = -log1p(-v);  key = beta s - log E;
4. the k + 1 eligible rows with the largest finite keys by (key desc, id asc): the first k are the sample, key_{k+1} the threshold;
5. log_p = beta (s - max) - log_rel, log_tau = key_{k+1} - (beta max + log_rel) (-inf: fewer than k + 1 rows),
   log_weight = log_p - log(-expm1(-exp(log_p - log_tau))) (log_tau = -inf: log_p).  A query without a finite log Z: all pads.

`device_key_bound` is the derived bound on |device key - float64 key| per (query, row); it is not fitted to what the device returns."""
import numpy as np

import partition_ref as P
from l2_ref import round_store

U = P.U
LOG_ULP = 1.0      # logf: 1 ulp (HIP math API accuracy table, single precision)
LOG1P_ULP = 1.0    # log1pf: 1 ulp (same table)
V_MAX = 1.0 - 2.0 ** -24
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """four uint64 arrays holding 32-bit counter words (broadcast against each other), two key words -> four output word arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3))
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2  # (32 x 32 bits: no overflow in uint64)
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def words(seed: int, qs, g):
    """(w_hi, w_lo) uint64 arrays of the broadcast shape of `qs` (query stream indices) and `g` (global row ids)"""
    qs, g = np.broadcast_arrays(np.asarray(qs, dtype=np.uint64), np.asarray(g, dtype=np.uint64))
    ctr = g >> np.uint64(2)
    out = []
    for j in (0, 1):
        w = philox4x32_10(ctr & MASK, ctr >> np.uint64(32), qs, np.uint64(j), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        lane = (g & np.uint64(3)).astype(np.int64)
        out.append(np.choose(lane, w))
    return out[0], out[1]


def uniforms(seed: int, qs, g) -> np.ndarray:
    """float64 v in (0, 1 - 2^-24]"""
    hi, lo = words(seed, qs, g)
    v = (hi.astype(np.float64) * 2.0 ** 32 + lo.astype(np.float64) + 0.5) * 2.0 ** -64
    return np.minimum(v, V_MAX)


def neg_log_e(v) -> np.ndarray:
    """-log E, E = -log1p(-v): the Gumbel noise of the key"""
    return -np.log(-np.log1p(-v))


def keys_from_scores(s, beta, seed, query_offset=0, id_base=0, eligible=None):
    """float64 [nq, n] keys; -inf where the row is not eligible, its score NaN or the key not finite"""
    s = np.asarray(s, dtype=np.float64)
    nq, n = s.shape
    v = uniforms(seed, query_offset + np.arange(nq)[:, None], id_base + np.arange(n)[None, :])
    with np.errstate(invalid="ignore"):
        key = beta * s + neg_log_e(v)
    keep = ~np.isnan(s) & np.isfinite(key)
    if eligible is not None:
        keep &= eligible
    return np.where(keep, key, -np.inf), v


def weights(log_p, log_tau):
    """log_weight of rows with `log_p` under the threshold `log_tau` (broadcast); log_tau = -inf: log_p"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        d = log_p - log_tau
        return np.where(np.isneginf(log_tau) & np.isfinite(log_p), log_p, log_p - np.log(-np.expm1(-np.exp(d))))


def sample_from_scores(s, k, beta, seed, query_offset=0, id_base=0, eligible=None):
    """dict of float64 / int64 arrays: ids [nq, k] (global, pads -1), scores, log_p, log_weight [nq, k] (pads -inf), keys [nq, k + 1]
    (pads -inf), log_tau [nq], max, log_rel [nq], key_matrix [nq, n] (the keys of every row, -inf: cannot be drawn)"""
    s = np.asarray(s, dtype=np.float64)
    nq, n = s.shape
    m, r = P.from_scores(s, beta, eligible)
    key, _ = keys_from_scores(s, beta, seed, query_offset, id_base, eligible) if n else (np.zeros((nq, 0)), None)
    live = np.isfinite(m) & np.isfinite(r)
    key = np.where(live[:, None], key, -np.inf)
    ids = np.full((nq, k), -1, dtype=np.int64)
    sc, lp, lw = (np.full((nq, k), -np.inf) for _ in range(3))
    keys = np.full((nq, k + 1), -np.inf)
    log_tau = np.full(nq, -np.inf)
    for a in range(nq):
        order = np.lexsort((np.arange(n), -key[a]))[: k + 1]  # key desc, id asc
        order = order[key[a][order] > -np.inf]
        keys[a, : len(order)] = key[a][order]
        top = order[:k]
        ids[a, : len(top)] = id_base + top
        sc[a, : len(top)] = s[a][top]
        lp[a, : len(top)] = beta * (s[a][top] - m[a]) - r[a]
        if len(order) == k + 1:
            log_tau[a] = keys[a, k] - (beta * m[a] + r[a])
        lw[a, : len(top)] = weights(lp[a, : len(top)], log_tau[a])
    return dict(ids=ids, scores=sc, log_p=lp, log_weight=lw, keys=keys, log_tau=log_tau, max=m, log_rel=r, key_matrix=key)


def sample(q, x, dtype, k, beta, seed, query_offset=0, id_base=0, eligible=None):
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    s = P.scores(q, x, dtype) if len(x) else np.zeros((len(q), 0))
    return sample_from_scores(s, k, beta, seed, query_offset, id_base, eligible)


def device_key_bound(s, absdot, dim, beta, v, dot=True) -> np.ndarray:
    """[nq, n] bound on |device key - float64 key| for rows with float64 score `s`, sum |q~_i x~_zi| `absdot` and uniform `v`
    (u = 2^-24).  The device computes  key = fl(fl(beta * s_dev) - logf(-log1pf(-v_dev))).

    dot    s_dev is the MFMA's float32 dot product over dim_pad terms: within gamma_{dim_pad} * absdot of s (products of two 16-bit
           values are exact in float32, the additions round; `partition_ref.dot_bound`), so beta * s moves by beta times that.
           `dot=False` (scores that are exact in float32) drops it.
    v      v_dev = float32(double(w) + 1/2) 2^-64): the double sum is exact below 2^52 and rounds once above (2^-53 relative), the
           conversion to float32 rounds once (u relative; v >= 2^-65 is a normal float32): |v_dev - v| <= dv = v (u + 2^-52); the
           clamp at 1 - 2^-24 is applied on both sides and only shrinks the difference.  The float64 v of this file carries 2^-53.
    log1p  E_dev = -log1pf(-v_dev) is within LOG1P_ULP ulp (2 u relative each) of -log1p(-v_dev); -log1p is increasing, so E_dev lies in
           [E(v - dv) (1 - 2 u), E(v + dv) (1 + 2 u)] with the arguments clamped to (0, 1 - 2^-24] - evaluated, not linearised:
           near v = 1 the slope 1 / (1 - v) reaches 2^24.
    log    L = logf(E_dev) is within LOG_ULP ulp of log(E_dev): |log E_dev - log E| from the interval above, + 2 u |log E_dev|.
    round  fl(beta * s_dev): u |beta s_dev|;  the subtraction: u |key_dev|.  Both magnitudes are taken with their own error added."""
    s = np.asarray(s, dtype=np.float64)
    kpad = (dim + 63) // 64 * 64
    e_dot = beta * (kpad * U / (1 - kpad * U)) * np.asarray(absdot, dtype=np.float64) if dot else np.zeros_like(s)
    dv = v * (U + 2.0 ** -51)
    lo = np.maximum(v - dv, 2.0 ** -66)
    hi = np.minimum(v + dv, V_MAX)
    e = -np.log1p(-v)
    e_lo = -np.log1p(-lo) * (1 - 2 * U * LOG1P_ULP)
    e_hi = -np.log1p(-hi) * (1 + 2 * U * LOG1P_ULP)
    d_log = np.maximum(np.log(e_hi) - np.log(e), np.log(e) - np.log(e_lo))
    log_mag = np.maximum(np.abs(np.log(e_lo)), np.abs(np.log(e_hi)))
    e_log = d_log + 2 * U * LOG_ULP * log_mag * (1 + 2 * U)
    with np.errstate(invalid="ignore"):
        prod = np.abs(beta * s) + e_dot
        key_mag = prod * (1 + U) + log_mag * (1 + 4 * U)
        out = e_dot + U * prod + e_log + U * key_mag
    return np.where(np.isfinite(out), out, np.inf) * (1 + 1e-9) + 1e-300


def key_bound(q, x, dtype, beta, seed, query_offset=0, id_base=0, dot=True) -> np.ndarray:
    """[nq, n]: `device_key_bound` of every (query, row) of a store"""
    qr, xr = round_store(q, dtype), round_store(x, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        s = qr @ xr.T
        absdot = np.abs(qr) @ np.abs(xr).T
    v = uniforms(seed, query_offset + np.arange(len(qr))[:, None], id_base + np.arange(len(xr))[None, :])
    return device_key_bound(s, absdot, xr.shape[1], beta, v, dot)


def fold_sample(keys_g, ids_g, scores_g, k, beta, max_score, log_rel):
    """Python twin of `fold_sample_posterior` (vod_amd/csrc/sample_fold.h) for ONE query: per-shard lists `keys_g[g]` (k + 1 keys,
    descending, -inf padded), `ids_g[g]` / `scores_g[g]` (k entries, pads id -1) -> (ids, scores, log_p, log_weight, keys)."""
    ids = np.full(k, -1, dtype=np.int64)
    sc, lp, lw = (np.full(k, -np.inf, dtype=np.float32) for _ in range(3))
    keys = np.full(k + 1, -np.inf, dtype=np.float32)
    if not (np.isfinite(max_score) and np.isfinite(log_rel)):
        return ids, sc, lp, lw, keys
    entries = []
    for kg, ig, sg in zip(keys_g, ids_g, scores_g):
        for p in range(k + 1):
            if not kg[p] > -np.inf or (p < k and ig[p] < 0):
                break
            entries.append((float(kg[p]), int(ig[p]) if p < k else -1, float(sg[p]) if p < k else -np.inf))
    entries.sort(key=lambda e: (-e[0], e[1] < 0, e[1]))
    key_tau = entries[k][0] if len(entries) > k else -np.inf
    for p, e in enumerate(entries[: k + 1]):
        keys[p] = e[0]
    b, m, r = float(np.float32(beta)), float(max_score), float(log_rel)
    lt = -np.inf if np.isneginf(key_tau) else (key_tau - b * m) - r
    for p, e in enumerate(entries[:k]):
        ids[p], sc[p] = e[1], e[2]
        a = b * (e[2] - m) - r
        lp[p] = a
        lw[p] = weights(np.float64(a), np.float64(lt))
    return ids, sc, lp, lw, keys
