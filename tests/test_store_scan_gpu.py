"""The whole-store scans agree on score bits: `log_partition`, `posterior_mean`, `sample_posterior`, `rank_ids` and `search` of one
`HipFlatIndex` give a (query, row) pair ONE float32 score.  The scans share one K loop and one eligibility rule
(vod_amd/csrc/store_scan.h); each operation's own tests compare it with its restatement, this file compares the operations with
each other, as `uint32` views.

Gaussian rows and queries, seeded.  Stores of 257 rows (two tiles, the second holding one live row) and 300 rows; widths 64, 129 and
256 (dim_pad / 64 = 1, 3, 4 K-loop steps: the prologue alone, the first pass through the steady loop, steady loop and full drain);
batches of 3 and 65 queries (the 64-query and the 128-query instantiation); both store dtypes; and all of it once more with subset
labels that exclude about half the rows.  `S[q, z]`, the yardstick, is the score `rank_ids` returns when every row is listed, 64 per
call.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
BATCHES = [3, 65]
K = 8


@functools.lru_cache(maxsize=None)
def _case(dim):
    rng = np.random.default_rng(9100 + dim)
    x = rng.standard_normal((300, dim)).astype(np.float32)
    q = rng.standard_normal((max(BATCHES), dim)).astype(np.float32)
    labels = rng.integers(0, 2, size=300).astype(np.int32)  # a query allows label q % 2: about half the rows
    for a in (x, q, labels):
        a.setflags(write=False)
    return x, q, labels


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _all_scores(ix, qd, n):
    """S [nq, n]: rank_ids over every row, 64 listed rows per call (the last call is shorter)"""
    cols = []
    for c0 in range(0, n, 64):
        ids = torch.arange(c0, min(c0 + 64, n), dtype=torch.int64, device="cuda").repeat(qd.shape[0], 1)
        cols.append(ix.rank_ids(qd, ids).score.cpu().numpy())
    return np.concatenate(cols, axis=1)


@pytest.mark.parametrize("labelled", [False, True], ids=["all_rows", "subset"])
@pytest.mark.parametrize("n", [257, 300])
@pytest.mark.parametrize("dim", [64, 129, 256])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_every_scan_and_the_search_give_a_pair_the_same_score_bits(dtype, dim, n, labelled):
    from vod_amd.index import HipFlatIndex

    x, q, labels = _case(dim)
    with HipFlatIndex(dim, n, dtype=TDT[dtype], device=0) as ix:
        ix.add(x[:n])
        if labelled:
            ix.set_row_labels(labels[:n])
        for nq in BATCHES:
            qd = torch.from_numpy(np.array(q[:nq])).cuda()
            S = _all_scores(ix, qd, n)  # (no query labels: every row is present)
            assert S.shape == (nq, n) and np.isfinite(S).all()
            sub = (np.arange(nq, dtype=np.int32) % 2)[:, None] if labelled else None
            elig = labels[None, :n] == sub if labelled else np.ones((nq, n), dtype=bool)
            assert elig.sum(axis=1).min() > K
            kw = {"subset": sub} if labelled else {}

            lp = ix.log_partition(qd, **kw)
            want_max = np.where(elig, S, -np.inf).max(axis=1)
            np.testing.assert_array_equal(_bits(lp.max_score), _bits(want_max))

            pm = ix.posterior_mean(qd, **kw)
            sp = ix.sample_posterior(qd, K, seed=1234 + nq, **kw)
            for other in (pm.log_partition, sp.log_partition):
                np.testing.assert_array_equal(_bits(other.max_score), _bits(lp.max_score))
                np.testing.assert_array_equal(_bits(other.log_rel), _bits(lp.log_rel))

            ids = sp.ids.cpu().numpy()
            assert (ids >= 0).all() and (ids < n).all()
            np.testing.assert_array_equal(_bits(sp.scores), _bits(np.take_along_axis(S, ids, axis=1)))
            assert np.take_along_axis(elig, ids, axis=1).all()  # with labels: only allowed rows are drawn

            ss, si = ix.search(qd, n, **kw)
            ss, si = ss.cpu().numpy(), si.cpu().numpy()
            hit = si >= 0
            np.testing.assert_array_equal(hit.sum(axis=1), elig.sum(axis=1))  # k = ntotal: the whole eligible order
            np.testing.assert_array_equal(_bits(ss[hit]), _bits(np.take_along_axis(S, np.where(hit, si, 0), axis=1)[hit]))
            assert np.take_along_axis(elig, np.where(hit, si, 0), axis=1)[hit].all()
