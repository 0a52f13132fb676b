"""NumPy restatement of `range_search` (vod_amd/csrc/kernels_range.hip) over a GIVEN float32 score matrix `s` `[nq, n]`:

    R(q) = { eligible rows z : key(s[q, z]) > key(t[q])  or  (key(s[q, z]) == key(t[q]) and id_base + z < r[q]) }

as CSR `(lims, scores, ids)` with ascending ids within a query.  `key` and eligibility are `rank_ref`'s, so `diff(lims)` is
`rank_ref.count` with one slot per query (0 where that says -1: a NaN threshold selects nothing).
"""
import numpy as np

import rank_ref as R

TIE_PAST_EVERY_ROW = np.iinfo(np.int64).max  # `inclusive=True`


def member(s, thresholds, tie_ids=None, eligible=None, id_base=0):
    """bool `[nq, n]`: row z is in R(q)"""
    s = np.asarray(s, dtype=np.float32)
    t = np.asarray(thresholds, dtype=np.float32)
    nq, n = s.shape
    ks, kt = R.key(s), R.key(t)
    inn = ks > kt[:, None]
    if tie_ids is not None:
        ids = id_base + np.arange(n, dtype=np.int64)
        # (compare as Python-free int64: the largest tie id is above every row)
        inn |= (ks == kt[:, None]) & (ids[None, :] < np.asarray(tie_ids, dtype=np.int64)[:, None])
    inn &= R._eligible(s, eligible)
    inn &= ~np.isnan(t)[:, None]
    return inn


def range_search(s, thresholds, tie_ids=None, eligible=None, id_base=0, inclusive=False):
    """(lims int64 `[nq + 1]`, scores float32 `[total]`, ids int64 `[total]`)"""
    s = np.asarray(s, dtype=np.float32)
    if inclusive:
        assert tie_ids is None
        tie_ids = np.full((s.shape[0],), TIE_PAST_EVERY_ROW, dtype=np.int64)
    inn = member(s, thresholds, tie_ids, eligible, id_base)
    lims = np.zeros((s.shape[0] + 1,), dtype=np.int64)
    np.cumsum(inn.sum(axis=1), out=lims[1:])
    qs, zs = np.nonzero(inn)  # row-major: queries in order, ascending rows within a query
    return lims, s[qs, zs], (id_base + zs).astype(np.int64)


def sort_by_score(lims, scores, ids):
    """every list re-sorted by (score desc, id asc), zeros of both signs equal - a plain Python sort, independent of `key`"""
    scores, ids = scores.copy(), ids.copy()
    for q in range(len(lims) - 1):
        b, e = int(lims[q]), int(lims[q + 1])
        order = sorted(range(b, e), key=lambda i: (-(float(scores[i]) + 0.0), int(ids[i])))
        scores[b:e], ids[b:e] = scores[order], ids[order]
    return scores, ids
