"""Float64 restatement (test infrastructure) of the weighted sum of LISTED rows: `HipFlatIndex.sum_ids`, include/vodhip.h H2w,
`sum_listed_kernel` of vod_amd/csrc/kernels_listed.hip - the backward of `score_ids` with respect to the queries.

  out[q, d] = sum over the slots j that are PRESENT and whose weight is not 0.0 of  w[q, j] * x[ids[q, j] - id_base, d]

Presence is the rule of `score_ids_ref` (empty: id < 0; out of range: id - id_base outside [0, ntotal); ineligible: `eligible`).  An
absent slot contributes nothing whatever its weight (NaN, +-inf); a present slot with weight 0.0 (either sign) is skipped and its row
is not read; all slots skipped: the zero row; a duplicate id contributes once per slot.  `x` holds the plane the device sums: the rows
as rounded to the store dtype, or the float32 rows of an `exact_f32` store.

THE BOUND (derived, not fitted; it holds for any chunking of the kernel, so it does not move when the kernel is retuned).  Take the n
contributing slots of one (query, column).  The device widens x exactly to float32 and fuses every product into its add (one rounding
per slot); partial sums meet in further float32 additions.  Adding a zero is exact, so however the n terms are associated no term
passes through more than n roundings, and by the standard argument (Higham, Accuracy and Stability, 4.2: any summation order)

  |device - float64| <= gamma_n * sum_j |w_j x_jd|,    gamma_n = n u / (1 - n u),  u = 2^-24.

Underflow: the library is built WITHOUT flushing subnormals (hipcc's default for gfx950: the kernels' descriptors carry
float_denorm_mode_32 = 3, and fp16 subnormals widen exactly), so an fma whose result is subnormal is rounded to a multiple of 2^-149:
an absolute error of at most 2^-150 per slot, n * 2^-150 in all.  (Additions never underflow inexactly.)  `TINY` = 2^-149 per slot is
used: twice what is needed, nothing next to any value a test holds.

`listed_scores` casts the gradient to the dtype of the queries: one more rounding of that dtype, `cast_bound`.
"""
from __future__ import annotations

import numpy as np

from score_ids_ref import eligible

U = 2.0 ** -24
TINY = 2.0 ** -149
EPS = {"float32": 0.0, "float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}   # unit roundoff of a query dtype
CAST_TINY = {"float32": 0.0, "float16": 2.0 ** -25, "bfloat16": 2.0 ** -134}  # half the smallest subnormal of that dtype


def contributing(ids, w, ntotal: int, id_base: int = 0, row_labels=None, q_labels=None) -> np.ndarray:
    """bool [nq, m]: the slots that enter the sum"""
    ids, w = np.asarray(ids, dtype=np.int64), np.asarray(w)
    local = ids - id_base
    keep = (ids >= 0) & (local >= 0) & (local < ntotal)
    for i in range(ids.shape[0]):
        slots = np.flatnonzero(keep[i])
        if len(slots):
            keep[i, slots] = eligible(row_labels, q_labels, i, local[i, slots])
    return keep & ~(w == 0)  # (a NaN weight is not 0: it stays)


def sum_ids(x, ids, w, id_base: int = 0, row_labels=None, q_labels=None) -> tuple[np.ndarray, np.ndarray]:
    """(out, bound), float64 [nq, dim] each: the sum and the bound on |device - out| per element.  Where `out` is not finite the bound
    is NaN or inf (compare such elements by class, not by distance)."""
    x64 = np.asarray(x, dtype=np.float64)
    ids, w64 = np.asarray(ids, dtype=np.int64), np.asarray(w, dtype=np.float64)
    keep = contributing(ids, w64, len(x64), id_base, row_labels, q_labels)
    out = np.zeros((ids.shape[0], x64.shape[1]))
    bound = np.zeros_like(out)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(ids.shape[0]):
            slots = np.flatnonzero(keep[i])
            n = len(slots)
            if n == 0:
                continue
            rows = ids[i, slots] - id_base
            terms = w64[i, slots, None] * x64[rows]
            out[i] = terms.sum(axis=0)
            bound[i] = n * U / (1 - n * U) * np.abs(terms).sum(axis=0) + n * TINY
    return out, bound


def cast_bound(out, bound, dtype: str) -> np.ndarray:
    """the bound after the device's float32 result was rounded once to `dtype` (a gradient cast to the dtype of the queries)"""
    return bound + EPS[dtype] * (np.abs(out) + bound) + CAST_TINY[dtype]
