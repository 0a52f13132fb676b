"""Float64 NumPy restatement of the marginal-likelihood objective (forward and its three gradients).

The formulas of `MarginalLikelihoodGradients` (the reference's src/vod_models/vod_gradients/marginal_likelihood.py:9-66), written
out with their analytic gradients; no reference code is imported.  Shared by tests/test_marginal_cpu.py, tests/test_marginal_gpu.py
and tests/golden/make_golden_marginal.py.

  live[b,d,t] = mask[b,d,t+1] != 0, tgt = ids[b,d,t+1]                       t = 0..L-2
  tok         = logits[b,d,t,tgt] - logsumexp_v logits[b,d,t,:]
  n, lp_xz    = sum_t live, (sum_t live * tok) / n
  r           = <q, s>, -inf where section__score is -inf ; lp_r = log_softmax_d r
  a = lp_r + lp_xz ; lp_x = logsumexp_d a ; loss = -mean_b lp_x
  post = exp(a - lp_x), p = exp(lp_r)
  dloss/dr = -(post - p) / B (0 at padded sections) ; dloss/dlogits = -post / (B n) * (1[v = tgt] - softmax_v) at live positions
A live target outside [0, V-2] makes lp_xz (and the loss) NaN; ids at masked positions are not looked at.
"""
from __future__ import annotations

import numpy as np


def _lse(x: np.ndarray, axis: int) -> np.ndarray:
    """logsumexp with -inf for an all -inf slice (torch.logsumexp)."""
    m = np.max(x, axis=axis, keepdims=True)
    sh = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.squeeze(sh, axis) + np.log(np.sum(np.exp(x - sh), axis=axis))


def marginal(q, s, score, logits, ids, mask, grad_out: float = 1.0) -> dict[str, np.ndarray]:
    """All outputs in float64: loss, retriever_scores, lp_xz, dq, ds, dlogits (the gradients scaled by `grad_out`)."""
    q, s, logits = np.asarray(q, np.float64), np.asarray(s, np.float64), np.asarray(logits, np.float64)
    score, ids, mask = np.asarray(score), np.asarray(ids).astype(np.int64), np.asarray(mask)
    B, D, L, V = logits.shape
    if L < 2:
        raise ValueError("L < 2")
    live = mask[..., 1:] != 0                      # [B,D,L-1]
    tgt = ids[..., 1:]
    x = logits[..., :-1, :]                        # [B,D,L-1,V]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lse = _lse(x, -1)                          # [B,D,L-1]
        valid = (tgt >= 0) & (tgt < V - 1)
        safe = np.where(valid & live, tgt, 0)
        x_t = np.take_along_axis(x, safe[..., None], axis=-1)[..., 0]
        tok = np.where(live, np.where(valid, x_t - lse, np.nan), 0.0)
        n = live.sum(-1).astype(np.float64)        # [B,D]
        lp_xz = tok.sum(-1) / n
        pad = np.isinf(score) & (score < 0)
        r = np.einsum("bh,bdh->bd", q, s) if s.ndim == 3 else np.einsum("bh,dh->bd", q, s)
        r = np.where(pad, -np.inf, r)
        lp_r = r - _lse(r, -1)[:, None]
        lp_r = np.where(np.all(pad, axis=-1, keepdims=True), np.nan, lp_r)   # log_softmax of an all -inf row
        a = lp_r + lp_xz
        lp_x = _lse(a, -1)
        loss = -lp_x.mean()
        post = np.exp(a - lp_x[:, None])
        p = np.exp(lp_r)
        dr = np.where(pad, 0.0, -(post - p) / B) * grad_out
        if s.ndim == 3:
            dq, ds = np.einsum("bd,bdh->bh", dr, s), dr[..., None] * q[:, None, :]
        else:
            dq, ds = dr @ s, dr.T @ q
        coef = -post / (B * n) * grad_out          # [B,D]
        soft = np.exp(x - lse[..., None])          # [B,D,L-1,V]
        onehot = np.zeros_like(soft)
        np.put_along_axis(onehot, safe[..., None], 1.0, axis=-1)
        g = coef[..., None, None] * (onehot - soft)
        g = np.where(live[..., None], g, 0.0)
        dlogits = np.zeros_like(logits)
        dlogits[..., :-1, :] = g
    return {"loss": np.float64(loss), "retriever_scores": r, "lp_xz": lp_xz, "dq": dq, "ds": ds, "dlogits": dlogits}


def scaled_error(got, want) -> float:
    """max |got - want| / max |want| over the entries finite in `want` (which must carry the same non-finite pattern)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), "non-finite entries differ"
    if not fin.any():
        return 0.0
    scale = np.abs(want[fin]).max()
    return float(np.abs(got[fin] - want[fin]).max() / (scale if scale > 0 else 1.0))
