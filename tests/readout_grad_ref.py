"""Float64 restatement of `HipFlatIndex.posterior_expectation_backward` (include/vodhip.h H2b, vod_amd/csrc/kernels_readout_grad.hip):

    grad = beta * ((p * (g @ v~.T - ubar)) @ x~),   ubar = sum_c g[q, c] y[q, c],   y = p @ v~

with p of `posterior_ref.weights` (rows and queries rounded to the store dtype, the eligible rows whose score is not NaN), v~ the
table rounded to the store dtype with `l2_ref.round_store`, and `g` as given (float32 -> float64: the device's one rounding of the
normalised g to the store dtype is an error term of the bound, zero when g is exact in 16 bits).  A query with no finite log Z gets
the zero row.

`device_bound` is the derived bound on |device gradient - float64 gradient| per (query, column) ("Read-out gradient"); it
is not fitted to what the device returns."""
import numpy as np

import partition_ref as P
import posterior_ref as M
import readout_ref as R
from l2_ref import round_store

U = P.U
GROUP_ROWS = R.GROUP_ROWS
EPS16 = M.EPS16
FP16_KEPT = M.FP16_KEPT
C_SLICE = 64                            # the table's columns are padded to whole slices: the K loop of u sums c_pad terms


def _table(v):
    v = np.asarray(v, dtype=np.float32)
    return v.reshape(-1, 1) if v.ndim == 1 else v


def expected_values_grad(q, x, v, g, dtype, beta, eligible=None):
    """(grad [nq, dim], values y [nq, n_cols], max [nq], log_rel [nq]) in float64.  Rows that carry weight 0 do not enter."""
    v = _table(v)
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    g = np.asarray(g, dtype=np.float64).reshape(len(q), v.shape[1])
    if len(x) == 0:
        return np.zeros((len(q), np.shape(x)[1])), np.zeros((len(q), v.shape[1])), np.full(len(q), -np.inf), np.full(len(q), -np.inf)
    p, m, r = M.weights(P.scores(q, x, dtype), beta, eligible)
    vr, xr = round_store(v, dtype), round_store(x, dtype)
    used = (p > 0).any(axis=0)
    pu, vu, xu = p[:, used], vr[used], xr[used]
    y = pu @ vu
    w = g @ vu.T - (g * y).sum(axis=1)[:, None]        # u_z - ubar_q
    return beta * ((pu * w) @ xu), y, m, r


def staging(g, y, vmax, dtype):
    """What the device's stage kernel forms per query, in float64: (k [nq], g^ 2^k [nq, n_cols] = the rounded g back in g's units,
    R_hi [nq] = the largest R_q the device may choose).  The device takes R_q = the power of two above A = (sum_c |g^_c| vmax_c +
    |ubar|)(1 + 2^-10) with ITS ubar (from its own y); the forward's error in y moves A by far less than 2^-8 of itself, so the power
    of two above A (1 + 2^-8) is at least the device's.  Rows with g = 0: k = 0, R = 1."""
    g = np.asarray(g, dtype=np.float64)
    amax = np.abs(g).max(axis=1) if g.shape[1] else np.zeros(len(g))
    k = np.where(amax > 0, np.floor(np.log2(np.where(amax > 0, amax, 1.0))), 0.0)
    gs = round_store((g * 2.0 ** -k[:, None]).astype(np.float32), dtype)
    ubar = np.abs((gs * y).sum(axis=1))
    A = ((np.abs(gs) * vmax[None, :]).sum(axis=1) + ubar) * (1 + 2.0 ** -8)
    R_hi = np.where(A > 0, 2.0 ** np.ceil(np.log2(np.where(A > 0, A, 1.0)) + 1e-12), 1.0)
    return k, gs * 2.0 ** k[:, None], R_hi


def device_bound(q, x, v, g, dtype, beta, eligible=None, dot=True, values_bound=None, rel_extra=0.0) -> np.ndarray:
    """[nq, dim] bound on |device gradient - float64 gradient|.  `values_bound` [nq, n_cols]: the bound on the error of the forward
    values the call was given, when they are not the flat index's (a node index folds them: its caller states that bound);
    `rel_extra` [nq]: a further relative error of every weight (the folded log_rel of a node index).

    The device returns  beta 2^k R * sum_g c_g prod_k r_k sum_z W'_z x~_zd,   W'_z = round16(fl(fl(e_z gamma_t) * t'_z)),
    t'_z = fl(u'_z - ubar') / R (an exact scale), with e, gamma, r_k, c_g of `readout_ref.device_bound`, u'_z the float32 MFMA sum
    of g^_c v~_zc over c_pad columns, g^ = round16(g 2^-k) and ubar' = float32 of sum_c g^_c y'_c summed in double, y' the DEVICE's
    forward values.  In exact arithmetic with the true g and y this is the reference.  u = 2^-24; E_p|.| = sum_z p_z |.|.

    rel     everything the read-out's weight carries (`readout_ref.rel_bound`: eps16 of the ONE rounding to the store dtype, the
            scores, the arguments, the expf's, the products, the float32 sum), and three more float32 roundings: the product with
            t', the product of the row's sum with beta (the power of two is exact) and one of slack.  Relative, on
            S = E_p[|u_z - ubar| |x~_zd|].
    g       the one rounding of the normalised g: |g^_c 2^k - g_c| <= dg_c = eps16 |g_c| (fp16: at least 2^(k - 25), an entry below
            2^-14 of the row's largest is an fp16 subnormal).  The same g^ enters u_z and ubar, so u_z - ubar moves by
            (g^ 2^k - g) . (v~_z - y), at most sum_c dg_c |v~_zc - y_c|:  beta sum_c dg_c E_p[|v~_zc - y_c| |x~_zd|]
            (<= eps16 beta sum_c |g_c| E_p[(|v~_zc| + |y_c|) |x~_zd|]; a column of ones cancels here too).  Zero when g 2^-k is
            exact in 16 bits.
    centre  ubar' uses the device's y': |y'_c - y_c| <= `readout_ref.device_bound`[q, c] = RB_c, so ubar moves by at most
            sum_c |g^_c 2^k| RB_c: beta sum_c |g_c| (1 + eps16) RB_c E_p|x~_zd|.
    f32     u'_z is a float32 sum of c_pad exact products in the MFMA's order: gamma_{c_pad} sum_c |g^_c 2^k| |v~_zc|; ubar' is
            rounded once (u |ubar|) and so is the difference (u |u_z - ubar|):
            beta ((1 + eps16) gamma_{c_pad} sum_c |g_c| E_p[|v~_zc| |x~_zd|] + u (|ubar| E_p|x~_zd| + S)).
    floor   fp16: a weight below 2^-29 of the running maximum's (|t'| <= 1, so no weight exceeds it) is subnormal after the 2^15 scale:
            as in the read-out, GROUP_ROWS * 2^-29 * 1.001 * max_z |x~_zd|, here in units of beta 2^k R.  bf16: zero.
    tiny    weights under 2^-126 (either factor): 2 n * 2^-126 * max_z |x~_zd| in the same units.
    The absolute terms (g, centre, f32) pass through the same relative errors: they are multiplied by 1 + rel."""
    v = _table(v)
    qr, xr, vr = round_store(q, dtype), round_store(x, dtype), round_store(v, dtype)
    nq, n_rows = qr.shape[0], xr.shape[0]
    g = np.asarray(g, dtype=np.float64).reshape(nq, v.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        s = qr @ xr.T
    p, m, _ = M.weights(s, beta, eligible)
    keep = ~np.isnan(s) if eligible is None else (np.asarray(eligible) & ~np.isnan(s))
    n = np.maximum(keep.sum(axis=1), 1).astype(np.float64)
    absx = np.abs(np.where(np.isfinite(xr), xr, 0.0))
    absv = np.abs(np.where(np.isfinite(vr), vr, 0.0))
    vfin = np.where(np.isfinite(vr), vr, 0.0)
    xmax = absx.max(axis=0) if n_rows else np.zeros(xr.shape[1])
    vmax = absv.max(axis=0) if n_rows else np.zeros(vr.shape[1])
    y = p @ vfin
    k, g_hat, R_hi = staging(g, y, vmax, dtype)
    absg = np.abs(g)
    dg = np.abs(g_hat - g)
    eps = EPS16[dtype]
    dg_bound = eps * absg
    if dtype == "float16":
        dg_bound = np.where(dg > 0, np.maximum(dg_bound, 2.0 ** (k[:, None] - 25)), 0.0)
    dg_bound = np.where(dg > 0, dg_bound, 0.0)                      # exact in 16 bits: no term
    ubar = (g * y).sum(axis=1)
    w = np.abs(g @ vfin.T - ubar[:, None])                           # |u_z - ubar| [nq, n]
    S = (p * w) @ absx                                              # [nq, dim]
    Ex = p @ absx                                                   # E_p |x_d|
    c_pad = (v.shape[1] + C_SLICE - 1) // C_SLICE * C_SLICE
    gam_c = c_pad * U / (1 - c_pad * U)
    rel = (1 + R.rel_bound(q, x, dtype, beta, n, n_rows, eligible, dot)) * (1 + U) ** 3 * (1 + np.asarray(rel_extra, dtype=np.float64)) - 1   # [nq]
    RB = R.device_bound(q, x, v, dtype, beta, eligible, dot=dot) if values_bound is None else np.asarray(values_bound, dtype=np.float64)
    # E_p[|v_c| |x_d|] weighted by a per-(q, c) coefficient: sum_c a_qc sum_z p_qz |v_zc| |x_zd| = ((p * (a @ |v|.T)) @ |x|)
    t_g = np.zeros_like(S)
    for i in np.flatnonzero(dg_bound.any(axis=1)):                  # (one query at a time: |v~_zc - y_c| depends on the query)
        t_g[i] = beta * ((p[i] * (np.abs(vfin - y[i][None, :]) @ dg_bound[i])) @ absx)
    t_centre = beta * (1 + eps) * (absg * RB).sum(axis=1)[:, None] * Ex
    t_f32 = beta * ((1 + eps) * gam_c * ((p * (absg @ absv.T)) @ absx) + U * (np.abs(ubar)[:, None] * Ex + S))
    unit = beta * 2.0 ** k * R_hi                                   # [nq]
    floor = unit[:, None] * ((GROUP_ROWS * FP16_KEPT * 1.001 if dtype == "float16" else 0.0) + 2 * n.max() * 2.0 ** -126) * xmax[None, :]
    return rel[:, None] * beta * S + (1 + rel[:, None]) * (t_g + t_centre + t_f32) + floor
