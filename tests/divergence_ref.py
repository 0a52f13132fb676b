"""Float64 restatement of `HipFlatIndex.posterior_divergence` (include/vodhip.h H2d, vod_amd/csrc/kernels_divergence.hip):

1. scores are `partition_ref.scores` of each side; a row is eligible for the PAIR when neither score is NaN and the pair's labels allow
   it; each side's (max, log_rel, mean_rel) are `stats_ref.from_scores` over those rows;
2. with p_z = exp(beta_a (s_a - max_a) - log_rel_a):  cross_rel_ab = sum p_z (s_b - max_b) <= 0 (a row with p_z > 0 and s_b = -inf
   makes it -inf; a row with s_a = -inf has p_z = 0 and adds nothing), and the mirror;
3. a side with no row (or scores all -inf): (-inf, -inf, NaN); with a +inf score: (+inf, +inf, NaN); both cross words are NaN then.

entropy_a = log_rel_a - beta_a mean_rel_a,  cross_entropy_ab = log_rel_b - beta_b cross_rel_ab,
kl_ab = max(0, (log_rel_b - log_rel_a) + (beta_a mean_rel_a - beta_b cross_rel_ab)).

`bounds` gives the derived bound on |device word - float64 word| for each of the eight library words and `derived_bounds` for the six
derived ones ("Posterior divergence").  None is fitted to what the device returns."""
from typing import NamedTuple

import numpy as np

import partition_ref as P
import stats_ref as S
from partition_ref import ARG_MAX, EXP_ULP, U, dot_bound, scores  # noqa: F401
from stats_ref import LANE_ADDS, UD

WORDS = ("max_a", "log_rel_a", "mean_rel_a", "cross_rel_ab", "max_b", "log_rel_b", "mean_rel_b", "cross_rel_ba")
DERIVED = ("entropy_a", "entropy_b", "cross_entropy_ab", "cross_entropy_ba", "kl_ab", "kl_ba")


class Ref(NamedTuple):
    words: tuple          # the eight float64 [nq] words, in the order of WORDS
    var_a: np.ndarray     # Var_p[s_a], Var_r[s_b]: what the per-side bounds are relative to
    var_b: np.ndarray
    cvar_ab: np.ndarray   # Var_p[s_b], Var_r[s_a]: the spread the dot-product part of the cross words multiplies
    cvar_ba: np.ndarray
    spread_a: np.ndarray  # max_a - the smallest finite eligible s_a (and b): the magnitude of a cross term whose weight underflows
    spread_b: np.ndarray
    n: np.ndarray         # rows eligible for the pair


def pair_eligible(sa, sb, eligible=None):
    keep = ~np.isnan(sa) & ~np.isnan(sb)
    if eligible is not None:
        keep &= eligible
    return keep


def _cross(s_own, s_other, m_own, m_other, beta, keep):
    """(E_p[s_other] - m_other, Var_p[s_other]) under p = softmax(beta s_own) over `keep`"""
    v, o = s_own[keep], s_other[keep]
    live = v > -np.inf
    v, o = v[live], o[live]
    w = np.exp(beta * (v - m_own))
    z = w.sum()
    if (o[w > 0] == -np.inf).any():
        return -np.inf, np.nan
    use = w > 0
    d = o[use] - m_other
    mean = (w[use] * d).sum() / z
    return mean, (w[use] * (d - mean) ** 2).sum() / z


def from_scores(sa, sb, beta_a, beta_b, eligible=None) -> Ref:
    sa, sb = np.asarray(sa, dtype=np.float64), np.asarray(sb, dtype=np.float64)
    nq = sa.shape[0]
    keep = pair_eligible(sa, sb, eligible)
    ma, ra, aa, va = S.from_scores(sa, beta_a, keep)
    mb, rb, ab, vb = S.from_scores(sb, beta_b, keep)
    cab, cba, vab, vba = (np.full(nq, np.nan) for _ in range(4))
    spa, spb = np.zeros(nq), np.zeros(nq)
    for i in range(nq):
        if not (np.isfinite(ma[i]) and np.isfinite(mb[i])):
            continue
        cab[i], vab[i] = _cross(sa[i], sb[i], ma[i], mb[i], beta_a, keep[i])
        cba[i], vba[i] = _cross(sb[i], sa[i], mb[i], ma[i], beta_b, keep[i])
        fa, fb = sa[i][keep[i]], sb[i][keep[i]]
        spa[i] = ma[i] - fa[fa > -np.inf].min()
        spb[i] = mb[i] - fb[fb > -np.inf].min()
    return Ref((ma, ra, aa, cab, mb, rb, ab, cba), va, vb, vab, vba, spa, spb, keep.sum(axis=1))


def posterior_divergence(qa, qb, x, dtype, beta_a, beta_b, eligible=None) -> Ref:
    qa = np.asarray(qa, dtype=np.float32).reshape(-1, np.shape(x)[1])
    qb = np.asarray(qb, dtype=np.float32).reshape(-1, np.shape(x)[1])
    if len(x) == 0:
        nq = len(qa)
        ninf, nan = np.full(nq, -np.inf), np.full(nq, np.nan)
        return Ref((ninf, ninf, nan, nan, ninf, ninf, nan, nan), nan, nan, nan, nan, np.zeros(nq), np.zeros(nq), np.zeros(nq, dtype=np.int64))
    return from_scores(scores(qa, x, dtype), scores(qb, x, dtype), beta_a, beta_b, eligible)


def derived(words, beta_a, beta_b):
    """the six float64 derived words, in the order of DERIVED"""
    ma, ra, aa, cab, mb, rb, ab, cba = words
    with np.errstate(invalid="ignore"):
        kl_ab = (rb - ra) + (beta_a * aa - beta_b * cab)
        kl_ba = (ra - rb) + (beta_b * ab - beta_a * cba)
        return (ra - beta_a * aa, rb - beta_b * ab, rb - beta_b * cab, ra - beta_a * cba,
                np.where(kl_ab < 0, 0.0, kl_ab), np.where(kl_ba < 0, 0.0, kl_ba))


def naive_kl(sa, sb, beta_a, beta_b):
    """sum p (log p - log r) in float64 from finite score matrices, every row eligible"""
    la = beta_a * sa - np.log(np.exp(beta_a * sa).sum(axis=1, keepdims=True))
    lb = beta_b * sb - np.log(np.exp(beta_b * sb).sum(axis=1, keepdims=True))
    return (np.exp(la) * (la - lb)).sum(axis=1)


def _compound(*parts):
    out = 0.0
    for p in parts:
        out = out + p + out * p
    return out


def cross_bound(beta_own, n_eligible, cross_rel, spread_other, e_own=None, e_other=None, sigma_cross=None, node=False):
    """[nq] bound on |device cross_rel - float64 cross_rel| for cross_rel = E_p[s_other] - max_other, p the posterior of the OWN side
    (beta_own).  u = 2^-24, n = rows eligible for the pair.

    dot    (`e_own is None`, scores exact in float32, drops it.)  Every device score of the own side is within E_own = `dot_bound` of its
           float64 value, of the other side within E_other, and so are the maxima.  The device posterior p^ has p^_z / p_z within
           exp(+-2 beta_own E_own), so
               |E_p^[s^_other] - E_p[s_other]| <= E_other + sum |p^_z - p_z| |s_other,z - mu| <= E_other + (exp(2 beta_own E_own) - 1) sigma
           with sigma = sqrt(Var_p[s_other]) (Cauchy-Schwarz; `sigma_cross`, computed by the restatement in float64), and the word also
           carries the other maximum's E_other:  dm = 2 E_other + (exp(2 beta_own E_own) - 1) sigma.
    tile   the term is fl(e fl(s_other - m_other)) with e = expf(fl(beta fl(s_own - m_own))): rho_e (stats_ref: the argument's two
           roundings through exp, expf's 1 ulp) and two more roundings - the arithmetic of posterior_stats' accumulator a.  Every term
           is <= 0: a same-sign float32 sum in which a term passes through at most 36 additions, relative gamma_36.
    finish c_t = expf(fl(beta fl(m_t - M))): rho_e again.  C = sum_t c_t (c_ab_t + (m_other_t - M_other) l_t) is same-sign too (every
           part <= 0), formed and added in double from float32 words that are exact in double: (tiles + 8) 2^-53 relative.  l_t has
           the relative error of the log-partition sum (rho_e, gamma_36), below c_ab_t's.  So C^ = C (1 + rC), L'^ = L' (1 + rL):
               |err| <= |cross_rel| (rC + rL) / (1 - rL).
    tiny   a weight below 2^-126 (flushed, rounded in the subnormal range, or dropped by the `e > 0` rule) is off by at most 2^-125
           absolutely, times |s_other - m_other| <= the other side's spread (`spread_other` = max - smallest finite eligible score;
           unlike mean_rel's own d it is not tied to the weight), per row, against L' >= 1.
    The word is rounded to float32 once.  The arithmetic part is taken at the device's own magnitude, the float64 one plus the dot part.
    node   (`node=True`.)  As stats_ref: the own side's weights exp(log_rel_g) are off by rw in the numerator and in the sum, a shard's
           word by its own flat error and its rounding u, u_g = cross_g + (m_other_g - M_other) <= 0 and sum_g w_g u_g are same-sign."""
    n = np.maximum(np.asarray(n_eligible, dtype=np.float64), 1.0)
    nq = np.shape(cross_rel)[0]
    tiles = np.ceil(n / 256.0)
    mag = np.abs(np.asarray(cross_rel, dtype=np.float64))
    if e_own is not None:
        dm = 2 * e_other + np.expm1(2 * beta_own * e_own) * np.asarray(sigma_cross, dtype=np.float64)
    else:
        dm = np.zeros(nq)
    mr = mag + dm
    rho_e = np.expm1(2.0001 * ARG_MAX * U) + 2 * EXP_ULP * U
    gamma = LANE_ADDS * U / (1 - LANE_ADDS * U)
    dbl = (tiles + 8) * UD
    r_l = _compound(rho_e, gamma, rho_e, dbl)
    r_c = _compound(rho_e, 2 * U, gamma, rho_e, dbl)
    rel = (r_c + r_l) / (1 - r_l)
    if node:
        r_w = _compound(np.expm1(P.device_bound(np.zeros((nq, 1)), None, None, beta_own, n, dot=False)), U * np.log(n))
        rel = _compound(rel, U, r_w, r_w / (1 - r_w), 8 * UD)
    tiny = n * 2.0 ** -125 * np.maximum(1.0, np.asarray(spread_other, dtype=np.float64) + dm)
    em = mr * rel + tiny
    return dm + em + U * (mr + em) + np.zeros(nq)


def bounds(qa, qb, x, dtype, beta_a, beta_b, ref: Ref, dot=True, node=False):
    """the eight per-word bounds, in the order of WORDS, against the float64 words of `ref`.  (max, log_rel, mean_rel) of a side are
    `stats_ref.bounds` of that side over the pair's eligible rows; the cross words `cross_bound`."""
    w = ref.words
    nq = len(w[0])
    za = np.zeros((nq, 1)) if not dot else qa
    zb = np.zeros((nq, 1)) if not dot else qb
    # NaN words (a dead side) get NaN bounds: the checks look at live pairs only
    with np.errstate(invalid="ignore"):
        ba = S.bounds(za, x, dtype, beta_a, ref.n, (w[0], w[1], w[2], ref.var_a), dot=dot, node=node)
        bb = S.bounds(zb, x, dtype, beta_b, ref.n, (w[4], w[5], w[6], ref.var_b), dot=dot, node=node)
        if dot:
            ea, eb = dot_bound(qa, x, dtype), dot_bound(qb, x, dtype)
            cab = cross_bound(beta_a, ref.n, w[3], ref.spread_b, ea, eb, np.sqrt(ref.cvar_ab), node=node)
            cba = cross_bound(beta_b, ref.n, w[7], ref.spread_a, eb, ea, np.sqrt(ref.cvar_ba), node=node)
        else:
            cab = cross_bound(beta_a, ref.n, w[3], ref.spread_b, node=node)
            cba = cross_bound(beta_b, ref.n, w[7], ref.spread_a, node=node)
    return ba[0], ba[1], ba[2], cab, bb[0], bb[1], bb[2], cba


def derived_bounds(beta_a, beta_b, words, b):
    """the six bounds of the derived words, in the order of DERIVED: the sums of the parts' bounds, and one float32 rounding of the
    result (the words are combined in float64: 2^-50 of the magnitudes covers it)"""
    ma, ra, aa, cab, mb, rb, ab, cba = (np.abs(t) for t in words)

    def total(err, *mags):
        size = sum(mags) + err
        return err + U * size + 8 * UD * size

    return (total(b[1] + beta_a * b[2], ra, beta_a * aa), total(b[5] + beta_b * b[6], rb, beta_b * ab),
            total(b[5] + beta_b * b[3], rb, beta_b * cab), total(b[1] + beta_a * b[7], ra, beta_a * cba),
            total(b[1] + b[5] + beta_a * b[2] + beta_b * b[3], ra, rb, beta_a * aa, beta_b * cab),
            total(b[1] + b[5] + beta_b * b[6] + beta_a * b[7], ra, rb, beta_b * ab, beta_a * cba))
