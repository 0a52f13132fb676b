"""Restatement of the Renyi VOD objective (`vod_amd.gradients.VodGradients`, include/vodhip.h H5v) in torch on the CPU.

No reference code exists (the reference's vod_gradients/vod.py raises NotImplementedError): the formulas below ARE the specification
(Lievin et al., "Variational Open-Domain Question Answering", arXiv 2210.06345: the self-normalised importance-sampling estimate of
the Renyi bound, differentiated with respect to the model with the sampler held constant).  Evaluated in float64 it is the oracle of
tests/test_vod_cpu.py and tests/test_vod_gpu.py; evaluated in float32 (`dtype=torch.float32`) it measures what a float32 pipeline of
the same formulas costs, the unit of the GPU tests' tolerance.  The gradients dq / ds / dlogits come from autograd; `d_scores` and
`coef` are the closed forms the kernel uses.

  live[b,d,t] = mask[b,d,t+1] != 0, tgt = ids[b,d,t+1]                    t = 0..L-2
  tok         = logits[b,d,t,tgt] - logsumexp_v logits[b,d,t,:]           (a live target outside [0, V-2]: NaN)
  n_d, l_d    = sum_t live, (sum_t live * tok) / n_d ("mean") | sum_t live * tok ("sum"; n_d = 0: NaN in both)
  r_d         = <q_b, s_(b,)d> ; retriever_scores = r, -inf where section__score is -inf (a PADDED section)
  c_d         = log_proposal, or temperature * score ; neither it nor logw is looked at on a padded section
  Lambda_b    = { d : not padded, logw_d != -inf, c_d != -inf }
  ls = logw - logsumexp_Lambda logw ; g = r - c ; lZ = logsumexp_Lambda (ls + g) ; lw = l + g - lZ ; eps = 1 - alpha
  Lhat_b = sum_Lambda exp(ls) lw                                           (eps == 0)
         = m + log1p( sum_Lambda exp(ls) expm1(eps (lw - m)) ) / eps , m = max_Lambda lw
  loss = -mean_b Lhat_b
  omega = softmax_Lambda(ls + eps lw), pi = softmax_Lambda(ls + g)
  d_scores = -(omega - pi) / B ; coef = -omega / (B n) ("mean") | -omega / B ("sum") ; both 0 outside Lambda
  iw_bound, elbo = mean_b Lhat_b at alpha = 0, 1 ; ess = mean_b 1 / sum_Lambda omega^2
An empty Lambda_b makes Lhat_b (and the loss) NaN, with no gradient from that row.  NaN is not -inf: a NaN in logw or c of a live
section goes through the formulas as written, into Lhat_b, the diagnostics and the gradients of every live section of the row.
"""
from __future__ import annotations

import numpy as np
import torch


def _bound(ls, lw, eps):
    if eps == 0:
        return (ls.exp() * lw).sum()
    m = lw.max().detach()  # the value does not depend on m: no gradient through it
    return m + torch.log1p((ls.exp() * torch.expm1(eps * (lw - m))).sum()) / eps


def vod(q, s, score, logw, logits, ids, mask, *, alpha=0.0, temperature=1.0, token_reduction="mean", log_proposal=None,
        grad_out=1.0, dtype=torch.float64) -> dict[str, np.ndarray]:
    """Every output as a float64 array: loss, retriever_scores, dq, ds, dlogits, d_scores, coef, iw_bound, elbo, ess, and per row /
    section Lhat [B], ls, lw [B, D] (NaN outside the live set).  Gradients are scaled by `grad_out`."""
    assert token_reduction in ("mean", "sum")
    q = torch.tensor(np.asarray(q, np.float64), dtype=dtype, requires_grad=True)
    s = torch.tensor(np.asarray(s, np.float64), dtype=dtype, requires_grad=True)
    logits = torch.tensor(np.asarray(logits, np.float64), dtype=dtype, requires_grad=True)
    score_t = torch.tensor(np.asarray(score, np.float64), dtype=dtype)
    logw_t = torch.tensor(np.asarray(logw, np.float64), dtype=dtype)
    ids_t = torch.tensor(np.asarray(ids).astype(np.int64))
    mask_t = torch.tensor(np.asarray(mask) != 0)
    B, D, L, V = logits.shape
    if L < 2:
        raise ValueError("L < 2")
    eps = 1.0 - float(alpha)
    pad = torch.isinf(score_t) & (score_t < 0)
    if log_proposal is None:
        c = temperature * torch.where(pad, torch.zeros_like(score_t), score_t)
    else:
        c = torch.tensor(np.asarray(log_proposal, np.float64), dtype=dtype)
    ninf = float("-inf")
    live_sec = ~pad & ~(logw_t == ninf) & ~(c == ninf)

    live = mask_t[..., 1:]
    tgt = ids_t[..., 1:]
    x = logits[..., :-1, :]
    valid = (tgt >= 0) & (tgt < V - 1)
    safe = torch.where(valid & live, tgt, torch.zeros_like(tgt))
    tok = x.gather(-1, safe[..., None])[..., 0] - torch.logsumexp(x, -1)
    tok = torch.where(live, torch.where(valid, tok, torch.full_like(tok, float("nan"))), torch.zeros_like(tok))
    n = live.sum(-1).to(dtype)
    l_sum = tok.sum(-1)
    if token_reduction == "mean":  # (no 0 / 0 in the graph: its backward would put NaN into sections that take no part)
        l_sum = l_sum / torch.where(n > 0, n, torch.ones_like(n))
    l_all = torch.where(n > 0, l_sum, torch.full_like(l_sum, float("nan")))

    r = torch.einsum("bh,bdh->bd", q, s) if s.dim() == 3 else torch.einsum("bh,dh->bd", q, s)
    nan = torch.tensor(float("nan"), dtype=dtype)
    rows = {k: [] for k in ("lhat", "iw", "elbo", "ess")}
    d_scores, coef = torch.zeros((B, D), dtype=dtype), torch.zeros((B, D), dtype=dtype)
    ls_all, lw_all = torch.full((B, D), float("nan"), dtype=dtype), torch.full((B, D), float("nan"), dtype=dtype)
    for b in range(B):
        idx = torch.nonzero(live_sec[b])[:, 0]
        if len(idx) == 0:
            for k in rows:
                rows[k].append(nan)
            continue
        ls = logw_t[b, idx] - torch.logsumexp(logw_t[b, idx], 0)
        g = r[b, idx] - c[b, idx]
        lZ = torch.logsumexp(ls + g, 0)
        lw = l_all[b, idx] + g - lZ
        rows["lhat"].append(_bound(ls, lw, eps))
        with torch.no_grad():
            rows["iw"].append(_bound(ls, lw, 1.0))
            rows["elbo"].append(_bound(ls, lw, 0.0))
            omega = torch.softmax(ls + eps * lw if eps != 0 else ls, 0)
            pi = torch.softmax(ls + g, 0)
            rows["ess"].append(1.0 / (omega * omega).sum())
            d_scores[b, idx] = -(omega - pi) / B * grad_out
            coef[b, idx] = -omega / B / (n[b, idx] if token_reduction == "mean" else 1.0) * grad_out
            ls_all[b, idx], lw_all[b, idx] = ls, lw
    lhat = torch.stack(rows["lhat"])
    loss = -lhat.mean()
    if loss.requires_grad:  # (not when every row is NaN)
        (loss * grad_out).backward()
    for x in (q, s, logits):
        if x.grad is None:
            x.grad = torch.full_like(x, float("nan"))
    out = {"loss": loss.detach(), "retriever_scores": torch.where(pad, torch.full_like(score_t, ninf), r.detach()),
           "dq": q.grad, "ds": s.grad, "dlogits": logits.grad, "d_scores": d_scores, "coef": coef,
           "iw_bound": torch.stack(rows["iw"]).mean(), "elbo": torch.stack(rows["elbo"]).mean(), "ess": torch.stack(rows["ess"]).mean(),
           "Lhat": lhat.detach(), "ls": ls_all, "lw": lw_all}
    return {k: v.double().numpy() for k, v in out.items()}


def log_softmax_live(c, score, logw=None) -> np.ndarray:
    """float32 `log_softmax` of `c` over the sections of each row that are not padded (and, with `logw`, not excluded by it): the
    exact self-normalised weights of a single-softmax sampler; -inf elsewhere."""
    c, score = np.asarray(c, np.float64), np.asarray(score, np.float64)
    keep = ~(np.isinf(score) & (score < 0))
    if logw is not None:
        keep &= ~(np.isinf(logw) & (np.asarray(logw) < 0))
    z = np.where(keep, c, -np.inf)
    m = z.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return (z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))).astype(np.float32)
