"""NumPy restatement of the rank calls (vod_amd/csrc/kernels_rank.hip) over a GIVEN float32 score matrix `s` `[nq, n]`:

    C(q; t, r) = #{ eligible rows z : key(s[q, z]) > key(t)  or  (key(s[q, z]) == key(t) and id_base + z < r) }

`key` is the search's result key (`flip_f32`): an order-preserving map of float32 to uint32 after `-0.0 -> +0.0`, so the two zeros are
equal.  A row is eligible when its score is not NaN and `eligible[q, z]` (subset labels; rows past ntotal are simply not in `s`).
"""
import numpy as np


def key(s):
    """flip_f32 of mips_common.h as uint32 (int64-held so that comparisons and `- 1` cannot wrap)"""
    u = (np.asarray(s, dtype=np.float32) + np.float32(0.0)).view(np.uint32).astype(np.int64)
    neg = (u & 0x80000000) != 0
    return np.where(neg, (~u) & 0xFFFFFFFF, u | 0x80000000)


def _eligible(s, eligible):
    ok = ~np.isnan(s)
    return ok if eligible is None else ok & eligible


def count(s, thresholds, tie_ids=None, eligible=None, id_base=0):
    """`count_above`: int64 `[nq, m]`; NaN thresholds give -1; `tie_ids=None` is the strict count"""
    s = np.asarray(s, dtype=np.float32)
    t = np.asarray(thresholds, dtype=np.float32)
    nq, n = s.shape
    ok = _eligible(s, eligible)
    ks, kt = key(s), key(t)
    ids = id_base + np.arange(n, dtype=np.int64)
    out = np.empty(t.shape, dtype=np.int64)
    for q in range(nq):  # one [m, n] comparison per query
        above = ks[q][None, :] > kt[q][:, None]
        if tie_ids is not None:
            above |= (ks[q][None, :] == kt[q][:, None]) & (ids[None, :] < np.asarray(tie_ids[q], dtype=np.int64)[:, None])
        out[q] = (above & ok[q][None, :]).sum(axis=1)
    out[np.isnan(t)] = -1
    return out


def rank_ids(s, ids, eligible=None, id_base=0):
    """`rank_ids`: (rank int64 `[nq, m]`, score float32 `[nq, m]`); absent slots (-1, -inf), NaN scores rank -1"""
    s = np.asarray(s, dtype=np.float32)
    ids = np.asarray(ids, dtype=np.int64)
    nq, n = s.shape
    local = ids - id_base
    present = (ids >= 0) & (local >= 0) & (local < n)
    safe = np.where(present, local, 0)
    if eligible is not None:
        present &= np.take_along_axis(eligible, safe, axis=1)
    score = np.where(present, np.take_along_axis(s, safe, axis=1), np.float32(-np.inf)).astype(np.float32)
    thr = np.where(present, score, np.float32(np.nan)).astype(np.float32)
    return count(s, thr, ids, eligible, id_base), score


def ranks_by_argsort(s, eligible=None):
    """rank of every row `[nq, n]` by a plain stable sort on (score desc, id asc); -1 for ineligible rows.  Independent of `key`."""
    s = np.asarray(s, dtype=np.float32)
    nq, n = s.shape
    ok = _eligible(s, eligible)
    out = np.full((nq, n), -1, dtype=np.int64)
    for q in range(nq):
        rows = np.nonzero(ok[q])[0]
        order = rows[np.argsort(-(s[q, rows].astype(np.float64) + 0.0), kind="stable")]  # stable: ties keep increasing id
        out[q, order] = np.arange(len(order))
    return out
