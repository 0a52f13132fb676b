"""Float64 NumPy restatement of the encoder's pooling head (forward and analytic backward), in both mask modes.

The formulas of `VodPooler`, `MeanAgg` and `ClsAgg` (the reference's src/vod_models/vod_encoder/modeling.py:76-89,164-174), written out
with their gradients; no reference code is imported.  Shared by tests/test_pooler_cpu.py, tests/test_pooler_gpu.py and
tests/golden/make_golden_pooler.py.

  cnt[n] = live mask elements of row n ; c = exp(0.5 * log_scaler) ; eps = 1e-12
  a      = mean, mode "reference": (sum over ALL positions of x[n,l,:]) / cnt   (the reference sums the padded positions too)
           mean, mode "masked":    (sum over the live positions) / cnt
           cls:                    x[n,0,:]                                      (the mask is ignored)
           a mean row with cnt = 0 is 0
  z      = a, or a @ W.T + b with a projection
  t = act(z) ; u = t | t / max(|t|_2, eps) | t / max(|t|_1, eps) ; y = c u
  g = dL/dy, du = c g ; d log_scaler = 0.5 sum g y
  l2, |t|_2 > eps: dt = (du - u (u.du)) / |t|_2 ; l1, |t|_1 > eps: dt = (du - sign(t) (u.du)) / |t|_1 ; below eps: dt = du / eps
  dz = dt act'(z) ; dW = dz.T a, db = sum_n dz, da = dz W (da = dz without a projection)
  d hidden[n,l,:] = da / cnt at every position ("reference") or at the live ones ("masked", 0 elsewhere) ; cls: da at l = 0, 0 elsewhere
A FULLY MASKED mean row has a zero gradient by definition here (the reference's autograd gives 0 / 0 there).
"""
from __future__ import annotations

import math

import numpy as np

EPS = 1e-12
ACTIVATIONS = (None, "relu", "tanh", "sigmoid", "gelu")
NORMS = (None, "l2", "l1")
_erf = np.vectorize(math.erf, otypes=[np.float64])


def act(name, z):
    if name is None:
        return z
    if name == "relu":
        return np.where(z > 0, z, 0.0)
    if name == "tanh":
        return np.tanh(z)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    if name == "gelu":
        return 0.5 * z * (1.0 + _erf(z / math.sqrt(2.0)))
    raise ValueError(name)


def act_grad(name, z):
    if name is None:
        return np.ones_like(z)
    if name == "relu":
        return np.where(z > 0, 1.0, 0.0)
    if name == "tanh":
        return 1.0 - np.tanh(z) ** 2
    if name == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-z))
        return s * (1.0 - s)
    if name == "gelu":
        return 0.5 * (1.0 + _erf(z / math.sqrt(2.0))) + z * np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    raise ValueError(name)


def aggregate(hidden, mask, agg: str, mode: str):
    """(a [N,H], cnt [N], the positions [N,L] the aggregate read): float64."""
    x = np.asarray(hidden, np.float64)
    live = np.asarray(mask) != 0
    N, L, _ = x.shape
    if agg == "cls":
        used = np.zeros((N, L), bool)
        used[:, 0] = True
        return x[:, 0, :].copy(), np.ones(N), used
    if agg != "mean":
        raise ValueError(agg)
    cnt = live.sum(-1).astype(np.float64)
    used = live if mode == "masked" else np.ones((N, L), bool)
    if mode not in ("reference", "masked"):
        raise ValueError(mode)
    s = np.where(used[..., None], x, 0.0).sum(1)  # a selection: what sits at an unread position does not matter
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(cnt[:, None] > 0, s / cnt[:, None], 0.0)
    return a, cnt, used


def finish(z, log_scaler, activation, norm):
    """(y, t, raw norm [N] or None): float64."""
    c = math.exp(0.5 * float(log_scaler))
    t = act(activation, np.asarray(z, np.float64))
    if norm is None:
        return c * t, t, None
    nrm = np.sqrt((t * t).sum(-1)) if norm == "l2" else np.abs(t).sum(-1)
    return c * (t / np.maximum(nrm, EPS)[:, None]), t, nrm


def finish_backward(z, g, log_scaler, activation, norm):
    """(dz, d log_scaler) for g = dL/dy."""
    z, g = np.asarray(z, np.float64), np.asarray(g, np.float64)
    c = math.exp(0.5 * float(log_scaler))
    y, t, nrm = finish(z, log_scaler, activation, norm)
    dls = 0.5 * float((g * y).sum())
    du = c * g
    if norm is None:
        dt = du
    else:
        u = t / np.maximum(nrm, EPS)[:, None]
        dot = (u * du).sum(-1, keepdims=True)
        direction = u if norm == "l2" else np.sign(t)
        big = (nrm > EPS)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            dt = np.where(big, (du - direction * dot) / np.where(big, nrm[:, None], 1.0), du / EPS)
    return dt * act_grad(activation, z), dls


def pool(hidden, mask, *, agg="mean", mode="reference", activation=None, norm=None, log_scaler=0.0, weight=None, bias=None,
         grad=None) -> dict[str, np.ndarray]:
    """Forward (`a`, `z`, `y`) and, with `grad` = dL/dy, the backward (`d_hidden`, `d_log_scaler`, `dz`, and `dW` / `db` with a
    projection), all float64."""
    x = np.asarray(hidden, np.float64)
    a, cnt, used = aggregate(x, mask, agg, mode)
    z = a if weight is None else a @ np.asarray(weight, np.float64).T + np.asarray(bias, np.float64)
    y, _, _ = finish(z, log_scaler, activation, norm)
    out = {"a": a, "z": z, "y": y}
    if grad is None:
        return out
    dz, dls = finish_backward(z, grad, log_scaler, activation, norm)
    out["dz"], out["d_log_scaler"] = dz, np.float64(dls)
    if weight is None:
        da = dz
    else:
        out["dW"], out["db"] = dz.T @ a, dz.sum(0)
        da = dz @ np.asarray(weight, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_tok = np.where(cnt[:, None] > 0, da / cnt[:, None], 0.0)   # a fully masked row: zero gradient
    out["d_hidden"] = np.where(used[..., None], per_tok[:, None, :], 0.0)
    return out


def scaled_error(got, want) -> float:
    """max |got - want| / max |want| (both finite)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(want).all() and np.isfinite(got).all(), "non-finite entries"
    scale = float(np.abs(want).max()) if want.size else 0.0
    return float(np.abs(got - want).max() / (scale if scale > 0 else 1.0)) if want.size else 0.0
