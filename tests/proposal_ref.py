"""Restatement of the labeled priority sampler WITH its proposal (include/vodhip.h H7, `vodhip_priority_sample_proposal`) in NumPy.

Written for this repository: the formulas below are the specification of `priority_sample_kernel` (vod_amd/csrc/kernels_sample.hip)
and of the four quantities it emits next to the reference's outputs.  Evaluated in float64 it is the oracle of
tests/test_proposal_cpu.py and tests/test_proposal_gpu.py; evaluated in float32 (`dtype=np.float32`, the same arithmetic on float32
arrays) it measures what a float32 pipeline of the same formulas costs, the unit of the GPU tests' tolerance (the scheme of
tests/vod_ref.py).

Per query row; a stratum S is the positives (label > 0) or the negatives, each in column order:
  t_inv      = temperature if temperature > 0 else 1
  k_total    = min(k_total, width) ; k_pos = min(k_positive, k_total given) ; n_neg_finite = #negatives whose score is not +-inf
  k_pos      = k_total - n_neg_finite                     if n_neg_finite < k_total - k_pos
  a_i        = t_inv * score_i                            then, when max_support > 0 and |S| > max_support, with thr = the
               max_support-th largest a of S: a_i = -inf where a_i >= thr ("reference": it REMOVES the best) | a_i < thr ("keep_top")
  NaN -> -inf ; mx = max_S a (0 when that is -inf) ; log_mass_S = mx + log sum_S exp(a_i - mx)            [-inf: empty / all -inf]
  log_p_i    = (a_i - mx) - log sum_S exp(a_i - mx)       [= a_i - log_mass_S; NaN in a stratum whose members are all -inf]
  lse_S      = log sum_S exp(log_p_i)                     [the reference's log_norm_const: ~0]
  key_i      = log_p_i - log(noise_i) if temperature > 0 else log_p_i ; members by key descending (NaN keys last, ties and NaNs by
               the smaller column) ; k = k_pos for the positives, k_total - #selected positives for the negatives
  selected   = the first min(max(k, 0), |S|) members ; log_tau = key of member number k (0-based) if 0 <= k < |S| else -inf
  w_j        = log_p_j - log1p(-exp(-exp(log_p_j - log_tau))) if log_tau > -inf else log_p_j
  log_weight = log_softmax over the selected w of S (NaN -> -inf, max 0 when -inf) when `normalized`, else w
  joint_j    = log_weight_j + log_mass_S(j) - logaddexp(log_mass_pos, log_mass_neg)   ; -inf when log_mass_S(j) is -inf: a member of
               a stratum without mass has probability 0 under one softmax over the row (its log_weight is NaN) - which covers
               "both masses are -inf"
Outputs [k_total given]: positives first, then negatives; pad slots carry sample -1, label 0 and -inf in log_weight, log_p, joint.

The selection is a discrete decision on float32 keys: in BOTH modes the keys are formed and ordered in float32 (what the kernel sorts),
so a float64 evaluation cannot pick another member through a last-bit difference; every value is then computed in `dtype`.
"""
from __future__ import annotations

import numpy as np


def _log_softmax(x, dt):
    """(log_softmax(x), log-sum-exp(x)) with the kernel's conventions: NaN -> -inf, a -inf maximum is replaced by 0."""
    ninf = dt(-np.inf)
    x = np.where(np.isnan(x), ninf, x).astype(dt)
    mx = x.max() if len(x) else ninf
    if np.isneginf(mx):
        mx = dt(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = x - mx
        lse = np.log(np.exp(v).sum(dtype=dt))
        return (v - lse).astype(dt), dt(mx + lse)


def _scaled(score, temperature, max_support, keep_top, dt):
    """a = t_inv * score of one stratum after the support truncation."""
    a = (score.astype(dt) * dt(temperature if temperature > 0 else 1.0)).astype(dt)
    if max_support > 0 and len(a) > max_support:
        thr = np.sort(a)[-max_support]
        a = np.where((a < thr) if keep_top else (a >= thr), dt(-np.inf), a).astype(dt)
    return a


def _stratum(score, noise, k, temperature, max_support, keep_top, normalized, dt):
    """One stratum: (selected member numbers, log_weight, lse, log_p of the selected, log_mass)."""
    m = len(score)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        log_p, log_mass = _log_softmax(_scaled(score, temperature, max_support, keep_top, dt), dt)
        lse = np.log(np.exp(log_p).sum(dtype=dt))
        # float32 keys, float32 order (see the module docstring)
        lp32 = log_p if dt is np.float32 else _log_softmax(_scaled(score, temperature, max_support, keep_top, np.float32), np.float32)[0]
        key32 = (lp32 - np.log(noise.astype(np.float32))) if temperature > 0 else lp32.copy()
        order = np.argsort(-key32, kind="stable")  # NaN last, ties by the smaller member number
        n_sel = min(max(k, 0), m)
        sel = order[:n_sel]
        if 0 <= k < m:
            tau_i = order[k]
            log_tau = (log_p[tau_i] - np.log(noise[tau_i].astype(dt))) if temperature > 0 else log_p[tau_i]
        else:
            log_tau = dt(-np.inf)
        lp_sel = log_p[sel]
        if log_tau > -np.inf:
            w = lp_sel - np.log1p(-np.exp(-np.exp(lp_sel - log_tau)))
        else:
            w = lp_sel.copy()
        w = w.astype(dt)
        if normalized and n_sel > 0:
            w = _log_softmax(w, dt)[0]
    return sel, w, dt(lse), lp_sel.astype(dt), log_mass


def sample_row(score, label, noise, k_positive, k_total, *, temperature=1.0, max_support=-1, keep_top=False, normalized=True,
               dtype=np.float64) -> dict[str, np.ndarray]:
    """One row.  `score` / `noise` float32 [width], `label` [width] (> 0 = positive); `max_support` as the C-ABI takes it (<= 0: none)."""
    dt = np.float32 if dtype in (np.float32, "float32") else np.float64
    score = np.asarray(score, np.float32)
    noise = np.asarray(noise, np.float32)
    pos = np.asarray(label) > 0
    n = len(score)
    k_out = int(k_total)
    k_tot = min(k_out, n)
    k_pos = min(int(k_positive), k_out)
    n_neg_finite = int((~pos & ~np.isinf(score)).sum())
    if n_neg_finite < k_tot - k_pos:
        k_pos = k_tot - n_neg_finite
    cols = np.arange(n)
    out = {"samples": np.full(k_out, -1, np.int64), "labels": np.zeros(k_out, bool), "log_weights": np.full(k_out, -np.inf, dt),
           "log_p": np.full(k_out, -np.inf, dt), "joint": np.full(k_out, -np.inf, dt), "lse": np.zeros(2, dt), "log_mass": np.zeros(2, dt)}
    cursor = n_pos_sel = 0
    cls_of = np.zeros(k_out, np.int64)
    for cls, members in enumerate((cols[pos], cols[~pos])):
        k = k_pos if cls == 0 else k_tot - n_pos_sel
        sel, w, lse, lp_sel, log_mass = _stratum(score[members], noise[members], k, temperature, max_support, keep_top, normalized, dt)
        j = slice(cursor, cursor + len(sel))
        out["samples"][j], out["labels"][j], out["log_weights"][j], out["log_p"][j] = members[sel], cls == 0, w, lp_sel
        cls_of[j] = cls
        out["lse"][cls], out["log_mass"][cls] = lse, log_mass
        cursor += len(sel)
        if cls == 0:
            n_pos_sel = len(sel)
    mp, mn = out["log_mass"]
    with np.errstate(invalid="ignore"):
        hi, lo = max(mp, mn), min(mp, mn)
        tot = hi + np.log1p(np.exp(dt(lo - hi))) if hi > -np.inf else dt(-np.inf)
        for j in range(cursor):
            mc = out["log_mass"][cls_of[j]]
            out["joint"][j] = out["log_weights"][j] + (mc - tot) if mc > -np.inf else -np.inf
    return out


def sample(scores, labels, noise, k_positive, k_total, **kw) -> dict[str, np.ndarray]:
    """Rows stacked: samples / labels / log_weights / log_p / joint [nq, k_total], lse / log_mass [nq, 2]."""
    rows = [sample_row(s, l, z, k_positive, k_total, **kw) for s, l, z in zip(scores, labels, noise)]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def flatten(ids, values, fill=-np.inf):
    """`flatten_samples(padding=True)` of one value array: (sorted distinct ids padded with 1 to B * n, values [B, B * n] by first
    occurrence, `fill` where the row does not hold the id)."""
    ids = np.asarray(ids)
    B, n = ids.shape
    uq = np.unique(ids)
    uq = np.concatenate([uq, np.ones(B * n - len(uq), ids.dtype)])
    out = np.full((B, B * n), fill, dtype=np.asarray(values).dtype)
    for b in range(B):
        for u, want in enumerate(uq):
            hit = np.flatnonzero(ids[b] == want)
            if len(hit):
                out[b, u] = values[b, hit[0]]
    return uq, out


def scaled_error(got, want) -> float:
    """max |got - want| / max(1, max |want|) over the entries finite in `want`, which must carry the same non-finite pattern (every
    output is a logarithm; `lse` is ~0, so below 1 the error is absolute)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), "non-finite entries differ"
    if not fin.any():
        return 0.0
    return float(np.abs(got[fin] - want[fin]).max() / max(1.0, np.abs(want[fin]).max()))
