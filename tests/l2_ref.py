"""Float64 restatement of the L2 search contract of `HipFlatIndex(metric="l2")` (include/vodhip.h, VODHIP_L2):

1. rows and queries are rounded to the store dtype (round-to-nearest-even, finite values beyond its range saturate);
2. d = sum_i (q~_i - x~_i)^2 in float64;
3. the k best by (d ascending, id ascending) - one `lexsort`;
4. missing entries are (+inf, -1).

Also the bias split's description in NumPy terms (`term_value`, `is_subnormal`, `RESIDUAL`, `LIMIT`) for tests/test_l2_cpu.py, and the derived error
bound of the device's float32 arithmetic (`device_bound`) for the Gaussian cases of tests/test_l2_gpu.py.
"""
import numpy as np

F16, BF16 = 0, 1
RESIDUAL = {F16: 2.0 ** -28, BF16: 2.0 ** -126}      # |c - sum_i const_i * term_i| within the limit (vod_amd/csrc/l2_bias.h)
LIMIT = {F16: 65504.0 * 256.0, BF16: 2.0 ** 120}     # largest |c| = |x~|^2 / 2 the split represents
MIN_NORMAL = {F16: 2.0 ** -14, BF16: 2.0 ** -126}


def round_store(a, dtype) -> np.ndarray:
    """`a` rounded to the store dtype (0 / "float16", 1 / "bfloat16"), as float64."""
    a = np.asarray(a, dtype=np.float32)
    if dtype in (F16, "float16", "f16"):
        with np.errstate(over="ignore"):
            return np.clip(a, -65504.0, 65504.0).astype(np.float16).astype(np.float64)
    u = np.ascontiguousarray(a).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)  # (finite inputs below the bf16 maximum: no carry into inf)
    return r.view(np.float32).astype(np.float64)


def distances(q, x, dtype) -> np.ndarray:
    """float64 [nq, n]: squared L2 distances of the rounded queries and rows, summed as (q - x)^2."""
    qr, xr = round_store(q, dtype), round_store(x, dtype)
    out = np.empty((qr.shape[0], xr.shape[0]), dtype=np.float64)
    buf = np.empty_like(xr)
    step = max(1, (1 << 21) // max(1, xr.shape[1]))  # row blocks of ~16 MB: the three passes stay in cache
    for a in range(qr.shape[0]):
        for lo in range(0, xr.shape[0], step):
            b = buf[lo : lo + step]
            np.subtract(xr[lo : lo + step], qr[a], out=b)
            np.square(b, out=b)
            out[a, lo : lo + step] = b.sum(axis=1)
    return out


def topk_from(d, k, id_base=0, eligible=None):
    """(float64 [nq, k], int64 [nq, k]) from a distance matrix: (d asc, id asc), pads (+inf, -1).  `eligible`: bool [nq, n] or None."""
    nq, n = d.shape
    out_d = np.full((nq, k), np.inf, dtype=np.float64)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    ids = np.arange(n)
    for a in range(nq):
        keep = ids if eligible is None else ids[eligible[a]]
        if len(keep) > 4 * k:  # only rows no farther than the k-th smallest distance can be among the k best
            keep = keep[d[a, keep] <= np.partition(d[a, keep], k - 1)[k - 1]]
        order = keep[np.lexsort((keep, d[a, keep]))][:k]
        out_d[a, : len(order)] = d[a, order]
        out_i[a, : len(order)] = order + id_base
    return out_d, out_i


def l2_topk(q, x, k, dtype, id_base=0, eligible=None):
    q = np.asarray(q, dtype=np.float32).reshape(-1, np.shape(x)[1]) if np.size(q) else np.zeros((0, np.shape(x)[1]), np.float32)
    if len(x) == 0:
        return np.full((len(q), k), np.inf), np.full((len(q), k), -1, dtype=np.int64)
    return topk_from(distances(q, x, dtype), k, id_base, eligible)


def term_value(bits, dtype) -> np.ndarray:
    """float64 values of store-dtype bit patterns"""
    b = np.asarray(bits, dtype=np.uint16)
    if dtype == F16:
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def is_subnormal(bits, dtype) -> np.ndarray:
    """a non-zero store-dtype pattern with a zero exponent field"""
    b = np.asarray(bits, dtype=np.uint16)
    exp_mask, frac_mask = (0x7C00, 0x03FF) if dtype == F16 else (0x7F80, 0x007F)
    return ((b & exp_mask) == 0) & ((b & frac_mask) != 0)


def device_bound(q, x, dtype, d64) -> np.ndarray:
    """[nq, n] bound on |device distance - float64 distance| for ANY float32 summation order of the three sums involved (the row's
    |x~|^2 at ingest, the query's |q~|^2 at staging, the D + 3 products of the contraction), u = 2^-24:
        u [2 (D + 3) (sum |q~_i x~_i| + |x~|^2 / 2) + D |x~|^2 + D |q~|^2] + 2 r(c) + 4 ulp(d)."""
    qr, xr = round_store(q, dtype), round_store(x, dtype)
    D = xr.shape[1]
    u = 2.0 ** -24
    absdot = np.abs(qr) @ np.abs(xr).T
    xn = (xr * xr).sum(axis=1)[None, :]
    qn = (qr * qr).sum(axis=1)[:, None]
    r = RESIDUAL[F16 if dtype in (F16, "float16", "f16") else BF16]
    return u * (2 * (D + 3) * (absdot + 0.5 * xn) + D * xn + D * qn) + 2 * r + 4 * np.spacing(d64.astype(np.float32)).astype(np.float64)


def float32_emulation(q, x, dtype):
    """[nq, n] float32: the device's FORM of the distance - max(0, |q~|^2 - 2 (q~.x~ - |x~|^2 / 2)) - evaluated by NumPy in float32."""
    qr, xr = round_store(q, dtype).astype(np.float32), round_store(x, dtype).astype(np.float32)
    s = qr @ xr.T - np.float32(0.5) * (xr * xr).sum(axis=1, dtype=np.float32)[None, :]
    return np.maximum(np.float32(0), (qr * qr).sum(axis=1, dtype=np.float32)[:, None] - np.float32(2) * s)
