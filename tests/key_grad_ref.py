"""Float64 restatement of `HipFlatIndex.key_gradient` (include/vodhip.h H2k, vod_amd/csrc/kernels_key_grad.hip):

    out = beta * (p * c).T @ q~,   c_qz = a_q + (u_qz - ubar_q),   u = G @ v~.T,   ubar_q = sum_c G[q, c] y[q, c],   y = p @ v~

with p of `posterior_ref.weights` (rows and queries rounded to the store dtype, scores and (max, log_rel) those of `partition_ref`), v~
the table rounded with `l2_ref.round_store`, and a, G as given (float32 -> float64: the device's one rounding of the normalised G is an
error term of the bound, zero when G 2^-k is exact in 16 bits).  A query without a finite log Z weighs nothing.  It is the gradient of
sum_q a_q log Z_q + sum_qc G_qc y_qc in x~ (tests/test_key_gradient_cpu.py checks that by central differences).

`staging` restates the device's batch-wide scales; `device_bound` is the derived bound on |device value - float64 value| per (row,
column) ("Key gradient"); it is not fitted to what the device returns."""
import numpy as np

import partition_ref as P
import posterior_ref as M
import readout_ref as R
from l2_ref import round_store

U = P.U
EPS16 = M.EPS16
FP16_KEPT = M.FP16_KEPT
SLICE = 1024                            # queries of one scan launch: later slices add to the result
C_SLICE = 64                            # the table's columns are padded to whole slices: the K loop of u sums c_pad terms


def _args(q, x, a, G, v):
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1])
    nq = len(q)
    a = np.zeros(nq) if a is None else np.asarray(a, dtype=np.float64).reshape(nq)
    if G is None:
        v = np.zeros((np.shape(x)[0], 0), dtype=np.float32)
        G = np.zeros((nq, 0))
    else:
        v = np.asarray(v, dtype=np.float32)
        v = v.reshape(-1, 1) if v.ndim == 1 else v
        G = np.asarray(G, dtype=np.float64).reshape(nq, v.shape[1])
    return q, a, G, v


def key_gradient(q, x, dtype, beta, a=None, G=None, v=None, eligible=None):
    """(out [n, dim], y [nq, n_cols], max [nq], log_rel [nq]) in float64.  Queries that weigh 0 do not enter."""
    q, a, G, v = _args(q, x, a, G, v)
    dim = np.shape(x)[1]
    if len(x) == 0:
        return np.zeros((0, dim)), np.zeros((len(q), v.shape[1])), np.full(len(q), -np.inf), np.full(len(q), -np.inf)
    p, m, r = M.weights(P.scores(q, x, dtype), beta, eligible)
    qr, vr = round_store(q, dtype).astype(np.float64), round_store(v, dtype).astype(np.float64)
    rows = (p > 0).any(axis=0)
    y = p[:, rows] @ vr[rows]
    used = (p > 0).any(axis=1)
    with np.errstate(invalid="ignore"):
        c = a[used, None] + (G[used] @ vr.T - (G[used] * y[used]).sum(axis=1)[:, None])
    pc = np.where(p[used] > 0, p[used] * c, 0.0)                    # (a row that weighs 0 spreads nothing, whatever its u)
    return beta * (pc.T @ qr[used]), y, m, r


def batch_exponent(a, G, live=None) -> int:
    """k = floor(log2 of the largest finite |G|) over the live queries, of the largest finite |a| when there is no G or G is all
    zero, else 0"""
    for t in (G, a):
        if t is None:
            continue
        t = np.abs(np.asarray(t, dtype=np.float32))
        t = (t if live is None else t[np.asarray(live, dtype=bool)]).reshape(-1)
        t = t[np.isfinite(t)]
        if t.size and t.max() > 0:
            return int(np.frexp(np.float64(t.max()))[1] - 1)  # amax = f 2^e, 1/2 <= f < 1
    return 0


def staging(a, G, y, vmax, dtype, live=None):
    """What the device's staging forms, with the device's arithmetic (`live` [nq]: the queries with finite forward words, all by
    default; a dead query enters no scale and gets flag 1 unless its gradient is not finite): dict of k, a' [nq] float32, g_hat [nq, n_cols] float32 (in units of
    2^k), ubar [nq] float32, B [nq] float64, flag [nq] (0 scan, 1 the zero row, 2 the NaN row), nan (bool), e (R = 2^e), shift = k + e"""
    nq = len(y) if a is None else len(np.asarray(a).reshape(-1))
    a32 = np.zeros(nq, dtype=np.float32) if a is None else np.asarray(a, dtype=np.float32).reshape(nq)
    G32 = np.zeros((nq, 0), dtype=np.float32) if G is None else np.asarray(G, dtype=np.float32).reshape(nq, -1)
    y = np.zeros((nq, 0)) if G is None else np.asarray(y, dtype=np.float32).reshape(nq, -1)
    vmax = np.zeros(G32.shape[1]) if G is None else np.asarray(vmax, dtype=np.float32)[:G32.shape[1]]
    k = batch_exponent(a, G, live)
    dead = np.zeros(nq, dtype=bool) if live is None else ~np.asarray(live, dtype=bool)
    bad = ~np.isfinite(a32) | ~np.isfinite(G32).all(axis=1)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        ap = np.ldexp(a32, -k).astype(np.float32)
        gn = np.ldexp(np.where(bad[:, None], 0, G32), -k).astype(np.float32)
        g_hat = round_store(gn, dtype).astype(np.float32)
        nz = g_hat != 0
        ubar = np.where(nz, g_hat.astype(np.float64) * y.astype(np.float64), 0.0).sum(axis=1).astype(np.float32)  # (exact products, summed in double)
        sa = np.where(nz, np.abs(g_hat).astype(np.float64) * vmax.astype(np.float64)[None, :], 0.0).sum(axis=1)
        B = np.abs(ap).astype(np.float64) + sa + np.abs(ubar).astype(np.float64)
        bf = B.astype(np.float32)
        bf = np.where(bf.astype(np.float64) < B, np.nextafter(bf, np.float32(np.inf)), bf)
    flag = np.where(bad, 2, np.where(dead, 1, np.where(~(bf < np.inf), 2, np.where(B == 0, 1, 0))))
    live = flag == 0
    ap, ubar, g_hat = np.where(live, ap, 0).astype(np.float32), np.where(live, ubar, 0).astype(np.float32), np.where(live[:, None], g_hat, 0).astype(np.float32)
    bmax = float(bf[live].max()) if live.any() else 0.0
    A = bmax * (1.0 + 1.0 / 1024.0)
    e, nan = 0, bool((flag == 2).any())
    if A > 0:
        e = max(int(np.frexp(A)[1]), -120)
        if e > 120:
            e, nan = 0, True
    return dict(k=k, a=ap, g_hat=g_hat, ubar=ubar, B=np.where(live, B, 0.0), flag=flag, nan=nan, e=e, shift=k + e)


def device_bound(q, x, dtype, beta, a=None, G=None, v=None, eligible=None, dot=True, values_bound=None, rel_extra=0.0) -> np.ndarray:
    """[n, dim] bound on |device value - float64 value|.  `values_bound` [nq, n_cols]: the bound on the error of the forward values the
    call was given, when they are not the flat index's (a node index folds them); `rel_extra` (per query or scalar): what a node index's
    folded log_rel adds to the exponent, as a factor exp(rel_extra).

    The device returns  beta 2^k R sum_q W'_qz q~_qd,   W'_qz = round16(fl(e_qz * t'_qz)),   t'_qz = fl(a'_q + fl(u'_qz - ubar'_q)) / R
    (an exact scale), e_qz = expf(fl(fl(min(0, fl(beta fl(s - max_q)))) - log_rel_q)) (the adjoint's weight), u'_qz the float32 MFMA sum
    of g^_c v~_zc over c_pad columns, g^ = round16(G 2^-k), a' = fl(a 2^-k), ubar' = float32 of sum_c g^_c y'_c summed in double, y' the
    device's forward values; k and R = 2^e are ONE pair for the batch (`staging`).  In exact arithmetic with the true a, G, y this is the
    reference.  u = 2^-24.  Per (query, row) the error of p c is bounded, then contracted with |q~_qd| over the queries:

        beta sum_q [ (rel_q gam - 1) p |c| + rel_q gam p (t_a + t_g + t_centre + t_f32) ] |q~_qd| + floor_d + tiny_d

    rel_q   1 + `readout_ref.rel_bound` - the ONE 16-bit rounding of the weight (eps16), the score and the two words, the argument's
            roundings and expf, as the adjoint's bound takes it - times (1 + u)^4 for the float32 sum with a', the product with e, the
            product with beta and one of slack, times exp(rel_extra).
    gam     the float32 sum of one element's terms - nq queries on the MFMA, 3 wave additions, one addition per further slice of 1024
            queries - is within gamma_kk of sum |terms|, kk = nq + 3 + slices; gam = 1 + gamma_kk.  The final power of two is exact.
    t_a     the rounding of a' = a 2^-k: exact unless it is a float32 subnormal, then at most 2^(k - 150).
    t_g     the one rounding of the normalised G: |g^_c 2^k - g_c| <= dg_c = eps16 |g_c| (fp16: at least 2^(k - 25), an entry below 2^-14
            of the BATCH's largest is an fp16 subnormal: the batch-wide scale costs a small query relative, not absolute, precision).
            The same g^ enters u and ubar, so c moves by at most sum_c dg_c |v~_zc - y_c| (a column of ones cancels here too).  Zero
            when G 2^-k is exact in 16 bits.
    centre  ubar' uses the device's y': |y'_c - y_c| <= `readout_ref.device_bound` (or `values_bound`): sum_c |g_c| (1 + eps16) RB_c.
    f32     `readout_grad_ref`'s treatment of u - ubar: u' is a float32 sum of c_pad exact products, gamma_{c_pad} sum_c |g^_c 2^k|
            |v~_zc|; ubar' is rounded once (u |ubar|) and so is the difference (u |u - ubar|).
    floor   fp16: |t'| <= 1 (R > max_q B_q >= |c| with 2^-10 to spare for the float32 error of u'), so |W'| <= 1; a weight below 2^-29
            is subnormal after the 2^15 scale and may be rounded coarsely or flushed: at most 2^-29 per query in units of the batch
            scale, beta 2^k R_hi * FP16_KEPT * sum_q |q~_qd|.  R_hi = the power of two above max_q B_q (1 + 2^-8) >= the device's (its
            ubar' comes from its own y').  bf16: zero.
    tiny    weights under 2^-126 (float32 / bf16 subnormals): nq * 2^-126 * max_q |q~_qd| in the same units, both dtypes."""
    q, a, G, v = _args(q, x, a, G, v)
    nq, n_rows, dim = len(q), np.shape(x)[0], np.shape(x)[1]
    if n_rows == 0:
        return np.zeros((0, dim))
    qr, xr, vr = round_store(q, dtype).astype(np.float64), round_store(x, dtype), round_store(v, dtype).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = round_store(q, dtype) @ xr.T
    p, _, _ = M.weights(s, beta, eligible)
    keep = ~np.isnan(s) if eligible is None else (np.asarray(eligible) & ~np.isnan(s))
    n = np.maximum(keep.sum(axis=1), 1).astype(np.float64)
    eps = EPS16[dtype]
    vfin = np.where(np.isfinite(vr), vr, 0.0)
    absv = np.abs(vfin)
    vmax = absv.max(axis=0) if v.shape[1] else np.zeros(0)
    y = p @ vfin
    afin, gfin = np.where(np.isfinite(a), a, 0.0), np.where(np.isfinite(G), G, 0.0)
    alive = (p > 0).any(axis=1)                                     # (a dead query enters no scale)
    k = batch_exponent(afin, gfin if G.shape[1] else None, alive)
    ubar = (gfin * y).sum(axis=1)
    uc = gfin @ vfin.T - ubar[:, None]                              # u - ubar [nq, n]
    c = np.abs(afin[:, None] + uc)
    # the roundings of the staging
    with np.errstate(under="ignore"):
        a_p = np.ldexp(afin.astype(np.float32), -k).astype(np.float64)
    t_a = np.where(np.ldexp(a_p, k) != afin, 2.0 ** (k - 150), 0.0)  # [nq]
    gn = np.ldexp(gfin, -k)
    g_hat = round_store(gn.astype(np.float32), dtype).astype(np.float64)
    absg = np.abs(gfin)
    dg = eps * absg
    if dtype == "float16":
        dg = np.maximum(dg, 2.0 ** (k - 25))
    dg = np.where(g_hat != gn, dg, 0.0)                             # exact in 16 bits: no term
    t_g = np.zeros_like(c)
    for i in np.flatnonzero(dg.any(axis=1)):                        # (one query at a time: |v~_zc - y_c| depends on the query)
        t_g[i] = np.abs(vfin - y[i][None, :]) @ dg[i]
    if G.shape[1]:
        RB = R.device_bound(q, x, v, dtype, beta, eligible, dot=dot) if values_bound is None else np.asarray(values_bound, dtype=np.float64)
    else:
        RB = np.zeros((nq, 0))
    t_centre = (1 + eps) * (absg * RB).sum(axis=1)                  # [nq]
    c_pad = (v.shape[1] + C_SLICE - 1) // C_SLICE * C_SLICE
    gam_c = c_pad * U / (1 - c_pad * U)
    t_f32 = (1 + eps) * gam_c * (absg @ absv.T) + U * (np.abs(ubar)[:, None] + np.abs(uc))
    rel = (1 + R.rel_bound(q, x, dtype, beta, n, n_rows, eligible, dot)) * (1 + U) ** 4 * np.exp(np.asarray(rel_extra, dtype=np.float64) + np.zeros(nq))
    kk = nq + 3 + (nq + SLICE - 1) // SLICE
    gam = 1 + kk * U / (1 - kk * U)
    rg = (rel * gam)[:, None]
    err = (rg - 1) * p * c + rg * p * (t_a[:, None] + t_g + t_centre[:, None] + t_f32)   # [nq, n]
    absq = np.abs(np.where(np.isfinite(qr), qr, 0.0))
    # the batch scale: B_q in units of 2^k, R_hi the largest R the device may choose
    B = np.abs(a_p) + (np.abs(g_hat) * vmax[None, :]).sum(axis=1) + np.abs((g_hat * y).sum(axis=1))
    A = (B[alive].max() if alive.any() else 0.0) * (1 + 2.0 ** -8)
    R_hi = 2.0 ** max(np.ceil(np.log2(A) + 1e-12), -120) if A > 0 else 1.0
    unit = beta * 2.0 ** k * R_hi
    floor = unit * ((FP16_KEPT * absq.sum(axis=0) if dtype == "float16" else 0.0) + nq * 2.0 ** -126 * (absq.max(axis=0) if nq else 0.0))
    return beta * (err.T @ absq) + floor[None, :]
