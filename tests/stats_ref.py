"""Float64 restatement of `HipFlatIndex.posterior_stats` (include/vodhip.h H2t, vod_amd/csrc/kernels_stats.hip):

1. scores, eligibility and the pair (max, log_rel) are `partition_ref`'s;
2. with p_z = exp(beta (s_z - max) - log_rel) over the eligible rows (a -inf score has p = 0 and adds nothing):
   mean_rel = sum p_z (s_z - max) <= 0,  var = sum p_z (s_z - max)^2 - mean_rel^2 >= 0;
3. no row (or scores that are all -inf): (-inf, -inf, NaN, NaN); a +inf score: (+inf, +inf, NaN, NaN).

`entropy = log_rel - beta * mean_rel`, `mean_score = max + mean_rel`.

`device_bound` is the derived bound on |device word - float64 word| for mean_rel and var ("Posterior statistics"); the
bounds of the first two words are `partition_ref.max_bound` / `partition_ref.device_bound`.  None is fitted to what the device returns."""
import numpy as np

import partition_ref as P
from partition_ref import ARG_MAX, EXP_ULP, U, dot_bound, scores  # noqa: F401  (the rounding helpers are partition_ref's)

UD = 2.0 ** -53           # unit roundoff of float64
LANE_ADDS = 36            # additions a term passes through inside a tile: 32 in the lane, 1 across the halves, 3 across the row waves


def from_scores(s, beta, eligible=None):
    """(max, log_rel, mean_rel, var), each float64 [nq], from a score matrix"""
    s = np.asarray(s, dtype=np.float64)
    nq = s.shape[0]
    out_m, out_r = P.from_scores(s, beta, eligible)
    out_mean = np.full(nq, np.nan)
    out_var = np.full(nq, np.nan)
    for a in range(nq):
        if not np.isfinite(out_m[a]):
            continue
        keep = ~np.isnan(s[a])
        if eligible is not None:
            keep &= eligible[a]
        v = s[a][keep]
        v = v[v > -np.inf]
        d = v - out_m[a]
        w = np.exp(beta * d)
        z = w.sum()
        mean = (w * d).sum() / z
        out_mean[a] = mean
        out_var[a] = max(0.0, (w * (d - mean) ** 2).sum() / z)  # (centred: no cancellation in the reference)
    return out_m, out_r, out_mean, out_var


def posterior_stats(q, x, dtype, beta, eligible=None):
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    if len(x) == 0:
        nq = len(q)
        return np.full(nq, -np.inf), np.full(nq, -np.inf), np.full(nq, np.nan), np.full(nq, np.nan)
    return from_scores(scores(q, x, dtype), beta, eligible)


def entropy(words, beta):
    """float64 [nq]: H(p) = log_rel - beta * mean_rel"""
    _, r, mean_rel, _ = words
    with np.errstate(invalid="ignore"):
        return r - beta * mean_rel


def mean_score(words):
    m, _, mean_rel, _ = words
    with np.errstate(invalid="ignore"):
        return m + mean_rel


def device_bound(q, x, dtype, beta, n_eligible, mean_rel, var, dot=True, node=False):
    """(bound on |device mean_rel - float64 mean_rel|, bound on |device var - float64 var|), each [nq].  `mean_rel`, `var`: the float64
    words (the bound is relative to them); u = 2^-24, n = eligible rows, E = `partition_ref.dot_bound`, sigma = sqrt(var).

    dot    (`dot=False`, scores that are exact in float32, drops it.)  Every device score is within E of its float64 value and so is the
           maximum.  The device posterior p^ then has p^_z / p_z within exp(+-2 beta E), so for any c
               |E_p^[s^] - E_p[s]| <= E + sum |p^_z - p_z| |s_z - mu| <= E + (exp(2 beta E) - 1) sigma   (Cauchy-Schwarz),
           and mean_rel also carries the maximum's E:  dm = 2 E + (exp(2 beta E) - 1) sigma.
           Var_p^[s] <= E_p^[(s - mu)^2] <= exp(2 beta E) Var_p[s] and the other way round, and sqrt Var_p^[s + delta] is within E of
           sqrt Var_p^[s] (Minkowski): |sigma^ - sigma| <= ds = sigma (exp(beta E) - 1) + E,  |var^ - var| <= ds (2 sigma + ds).
    e      (H2p (2).)  t = fl(beta fl(s - m)) has relative error 2 u + u^2, so for |t| <= 104 exp(t) moves by a factor within
           exp(+-208.1 u), and expf is 1 ulp (relative 2 u):  rho_e.  Below -104 the term, times |d| or d^2 at d = 104 / beta (both
           x exp(beta x) and x^2 exp(beta x) fall beyond it), and a result flushed or rounded in the subnormal range stay below
           2^-125 max(1, 104 / beta)^2 per row, against L >= 1: the absolute part.
    tile   a's term is fl(e fl(s - m)): rho_e and two more roundings; b's term one product and one fl(s - m) more: four.  The sums
           are same-sign float32 sums in which a term passes through at most 36 additions (32 in the lane, 1 across the halves, 3
           across the waves): relative gamma_36 = 36 u / (1 - 36 u), no cancellation.
    finish c_t = expf(fl(beta fl(m_t - M))): rho_e again.  A = sum c_t (a_t + D_t l_t) <= 0 and B = sum c_t (b_t + 2 D_t a_t +
           D_t^2 l_t) >= 0 are same-sign too (a_t, D_t <= 0 <= l_t, b_t), formed and added in double: (tiles + 8) 2^-53 relative.
           So A^ = A (1 + rA), B^ = B (1 + rB), L'^ = L' (1 + rL) with the relative parts compounded.
    var    mean_rel = A / L':  |err| <= |mean_rel| (rA + rL) / (1 - rL) = em.  S2 = B / L' = var + mean_rel^2:  |err| <= S2 (rB + rL) /
           (1 - rL).  var = S2 - mean_rel^2:  the absolute errors add, 2 |mean_rel| em + em^2 for the square: this is where a posterior
           far below its maximum (|mean_rel| >> sigma) costs digits.  The clamp at 0 only moves towards the true var >= 0.
    Each word is rounded to float32 once (u relative).  The arithmetic parts are taken at the device's own magnitudes, the float64
    ones plus the dot part.
    node   (`node=True`: the words of a node index, whatever the split into shards.)  A shard's words carry the errors above, relative
           to the shard's own maximum m_g <= M, so sum_g w_g S2_g <= S2 and mean_rel_g^2 <= S2_g.  Its weight exp(log_rel_g) is off by
           a factor exp(+-PB), PB = `partition_ref.device_bound` without its dot part (log_rel_g is the log of the float32 sum L, not of
           L'), and by the word's rounding (u log n): rw, in the numerator and in the sum of the weights.  u_g = mean_rel_g + (m_g - M) <= 0 is a same-sign sum and sum_g w_g u_g too: mean_rel's relative error is the flat
           one, u, and rw twice.  The second moment sum_g w_g (var_g + u_g^2) carries var_g's own error (the flat one: its S2 part and
           2 rm + rm^2 for its square, rm = the flat relative error of mean_rel), u for the word, 2 rm + rm^2 for u_g^2, and rw twice.
           The fold itself runs in double."""
    nq = np.shape(q)[0]
    n = np.maximum(np.asarray(n_eligible, dtype=np.float64), 1.0)
    tiles = np.ceil(n / 256.0)
    mean_rel = np.abs(np.asarray(mean_rel, dtype=np.float64))
    var = np.asarray(var, dtype=np.float64)
    sigma = np.sqrt(var)
    if dot:
        e_dot = dot_bound(q, x, dtype)
        dm = 2 * e_dot + np.expm1(2 * beta * e_dot) * sigma
        ds = sigma * np.expm1(beta * e_dot) + e_dot
        dv = ds * (2 * sigma + ds)
    else:
        dm = dv = ds = np.zeros(nq)
    # the device's own magnitudes
    mr = mean_rel + dm
    s2 = (var + dv) + mr * mr
    rho_e = np.expm1(2.0001 * ARG_MAX * U) + 2 * EXP_ULP * U
    gamma = LANE_ADDS * U / (1 - LANE_ADDS * U)
    dbl = (tiles + 8) * UD

    def compound(*parts):
        out = 0.0
        for p in parts:
            out = out + p + out * p
        return out

    r_l = compound(rho_e, gamma, rho_e, dbl)
    r_a = compound(rho_e, 2 * U, gamma, rho_e, dbl)
    r_b = compound(rho_e, 4 * U, gamma, rho_e, dbl)
    tiny = n * 2.0 ** -125 * max(1.0, ARG_MAX / beta) ** 2
    rel_m = (r_a + r_l) / (1 - r_l)
    rel_2 = (r_b + r_l) / (1 - r_l)
    if node:
        r_w = compound(np.expm1(P.device_bound(np.zeros((nq, 1)), None, None, beta, n, dot=False)), U * np.log(n))
        square = 2 * rel_m + rel_m * rel_m
        rel_2 = compound(rel_2 + 2 * square + U, r_w, r_w / (1 - r_w), 8 * UD)
        rel_m = compound(rel_m, U, r_w, r_w / (1 - r_w), 8 * UD)
    em = mr * rel_m + tiny
    e2 = s2 * rel_2 + tiny
    b_mean = dm + em + U * (mr + em)
    ev = e2 + 2 * mr * em + em * em + UD * s2
    b_var = dv + ev + U * (var + dv + ev)
    return b_mean + np.zeros(nq), b_var + np.zeros(nq)


def bounds(q, x, dtype, beta, n_eligible, words, dot=True, node=False):
    """the four per-word bounds (max_score, log_rel, mean_rel, var) against the float64 `words`; `node`: of a node index - log_rel
    with the float32 rounding of the fold's result and of the shards' words on top of the shards' own (the sum runs in double)"""
    nq = np.shape(q)[0]
    b_max = P.max_bound(q, x, dtype) if dot else np.zeros(nq)
    b_rel = P.device_bound(q, x, dtype, beta, n_eligible, dot=dot)
    if node:
        b_rel = b_rel + 4 * U * (1 + np.log(np.maximum(np.asarray(n_eligible, dtype=np.float64), 1.0)))
    b_mean, b_var = device_bound(q, x, dtype, beta, n_eligible, words[2], words[3], dot=dot, node=node)
    return b_max, b_rel, b_mean, b_var


def entropy_bound(beta, words, b_rel, b_mean):
    """|float32 (log_rel - beta mean_rel) - float64 entropy|: the two words' bounds, the rounding of beta to float32 and of the
    product and the difference (3 u of the larger magnitudes)"""
    _, r, mean_rel, _ = words
    return b_rel + beta * b_mean + 3 * U * (np.abs(r) + b_rel + 2 * beta * (np.abs(mean_rel) + b_mean))


def mean_score_bound(words, b_max, b_mean):
    """|float32 (max + mean_rel) - float64 mean score|: the two words' bounds and the rounding of the sum"""
    m, _, mean_rel, _ = words
    return b_max + b_mean + U * (np.abs(m) + np.abs(mean_rel) + b_max + b_mean)
