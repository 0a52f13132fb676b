"""Restatement (test infrastructure) of scoring LISTED sections on the dense engine: `HipFlatIndex.score_ids`, include/vodhip.h H2i.

PARITY UNPINNED.  The reference has NO dense implementation of `ids`: its faiss client drops the argument
(/root/reference/src/vod_search/faiss_search/client.py:70, `# noqa: ARG002`).  What is restated here is the contract of the one engine
of the reference that honours it, the Elasticsearch client (src/vod_search/es_search/client.py:145,177-183): a `terms` filter on the
section id, so that only listed sections can be hits and a listed section counts once; an empty list gives no hit; the result's labels
are `scores > -inf`.  The score itself is the dense engine's own (oracle/flat_ip.py): the inner product of the query and the row AS
ROUNDED to the store dtype, accumulated in float64.

  aligned form   out[q, j] = float64(q~) . float64(x~[ids[q, j] - id_base]); -inf where the slot is absent: empty (id < 0), out of
                 range (id - id_base outside [0, ntotal)) or ineligible (the row's label is not among the query's labels; all -1 =
                 unrestricted - the rule of the subset filter).  A duplicate id is scored once per slot.
  top-k form     the distinct present ids of a row, NaN and -inf scores dropped, ordered by (score desc, id asc), the first k; pads
                 (-inf, -1).

For fp16 / bf16 inputs the float64 sum is the correctly rounded reference the GPU's fp32 accumulation is compared against; on the
small-integer fixtures every partial sum is exact in fp32, so the GPU and this file agree bit for bit.
"""
from __future__ import annotations

import numpy as np


def eligible(row_labels, q_labels, q: int, rows: np.ndarray) -> np.ndarray:
    """Which of `rows` query q may see: everything without labels or with all slots -1, else the rows whose label is listed."""
    if row_labels is None or q_labels is None:
        return np.ones(len(rows), dtype=bool)
    allowed = np.asarray(q_labels[q])
    if (allowed == -1).all():
        return np.ones(len(rows), dtype=bool)
    return np.isin(np.asarray(row_labels)[rows], allowed[allowed != -1])


def score_ids_aligned(q: np.ndarray, x: np.ndarray, ids: np.ndarray, id_base: int = 0, row_labels=None, q_labels=None) -> np.ndarray:
    """float64 [nq, m]: the aligned form.  `q` / `x` hold the values as rounded to the store dtype (any float dtype); `x` = the ntotal rows."""
    q64, x64 = np.asarray(q, dtype=np.float64), np.asarray(x, dtype=np.float64)
    ids = np.asarray(ids, dtype=np.int64)
    out = np.full(ids.shape, -np.inf, dtype=np.float64)
    for i in range(ids.shape[0]):
        local = ids[i] - id_base
        present = (ids[i] >= 0) & (local >= 0) & (local < len(x64))
        slots = np.flatnonzero(present)
        if len(slots) == 0:
            continue
        rows = local[slots]
        ok = eligible(row_labels, q_labels, i, rows)
        with np.errstate(invalid="ignore", over="ignore"):
            out[i, slots[ok]] = x64[rows[ok]] @ q64[i]
    return out


def score_ids_topk(aligned: np.ndarray, ids: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """(scores [nq, k] in the dtype of `aligned`, ids int64 [nq, k]) from the aligned scores: dedupe, drop NaN / -inf, lexsort by
    (-score, id), pads.  Taking the aligned scores as input lets a test order the DEVICE's own scores as well."""
    aligned, ids = np.asarray(aligned), np.asarray(ids, dtype=np.int64)
    out_s = np.full((ids.shape[0], k), -np.inf, dtype=aligned.dtype)
    out_i = np.full((ids.shape[0], k), -1, dtype=np.int64)
    for i in range(ids.shape[0]):
        keep = ~np.isnan(aligned[i]) & (aligned[i] > -np.inf)
        uid, first = np.unique(ids[i][keep], return_index=True)
        s = aligned[i][keep][first] + 0.0  # (-0.0 orders as +0.0)
        order = np.lexsort((uid, -s))[:k]
        out_s[i, : len(order)] = s[order]
        out_i[i, : len(order)] = uid[order]
    return out_s, out_i


def es_labels(scores: np.ndarray) -> np.ndarray:
    """`labels = scores > -inf` as the Elasticsearch client returns them (es_search/client.py:145), int64."""
    return (np.asarray(scores) > -np.inf).astype(np.int64)
