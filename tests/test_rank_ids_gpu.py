"""`rank_ids` / `count_above` of `HipFlatIndex` and `HipNodeIndex` on the GPU against the NumPy restatement (tests/rank_ref.py).

Everything here is EXACT: ranks and counts are integers, scores are compared as bits.  Integer data (values in [-8, 8]: exact in fp16
and bf16, every score an exact integer in float32, so the restatement's score matrix IS the scan's): stores of 1, 255, 256, 257 (one
tile, the tile edge, two tiles), 1500 and 3000 rows, widths 1 (scores in [-64, 64]: hundreds of ties per score, the id rule decides
almost every rank), 64, 65, 768, batches 1, 64 (the 64-query kernel), 65, 129, 300 (the 128-query kernel, one to three query tiles),
1, 2, 8, 9 and 64 slots; the 300 x 64 call lists every row of the store.  One data set per width (300 queries, 3000 rows): a smaller
store or batch is its first rows; the reference ranks of every (query, row) are computed once per (width, store).

Gaussian data: `rank_ids(q, ids of search(q, ntotal))` must be `arange(ntotal)` with the bits of the search's scores - the listed pairs'
scores come from a gathered mini-store, not from the scan, and this is what proves them equal.  Then: absent slots, duplicates,
`id_base`, stale rows, NaN / +-inf scores, subset labels, a batch of two slices (1100 queries), thresholds on and between the scores, batch independence, a call beside a
search in flight, the node index on 1, 2 and 3 shards of device 0, refusals and empty cases.
"""
import ctypes
import functools

import numpy as np
import pytest

import rank_ref as R
from test_l2_cpu import GAUSS_CASES, gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
STORES = [1, 255, 256, 257, 1500, 3000]
WIDTHS = [1, 64, 65, 768]
BATCHES = [1, 64, 65, 129, 300]
SLOTS = [1, 2, 8, 9, 64]


def _index(x, dtype="float16", capacity=None, dim=None, **kw):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, **kw)
    if len(x):
        ix.add(x)
    return ix


@functools.lru_cache(maxsize=None)
def _int_case(d, n=3000, nq=300):
    """integer rows / queries and their exact float32 scores; the same for both store dtypes (both hold the values exactly)"""
    rng = np.random.default_rng(4000 + d)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    s64 = q.astype(np.float64) @ x.astype(np.float64).T
    s = s64.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), s64)  # every score is exact in float32
    for a in (q, x, s):
        a.setflags(write=False)
    return q, x, s


@functools.lru_cache(maxsize=None)
def _all_ranks(d, n):
    """the reference rank of every row of the first n rows for every query: [300, n], computed once per (width, store)"""
    _, _, s = _int_case(d)
    rank = R.ranks_by_argsort(s[:, :n])  # the sort form of the restatement (n log n per query); the counting form on three queries
    some = [0, 150, s.shape[0] - 1]
    by_count, score = R.rank_ids(s[some, :n], np.broadcast_to(np.arange(n, dtype=np.int64), (len(some), n)))
    assert np.array_equal(by_count, rank[some]) and np.array_equal(score, s[some, :n])
    for q in some:
        assert np.array_equal(np.sort(rank[q]), np.arange(n))  # a permutation
    rank.setflags(write=False)
    return rank


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _rank(ix, q, ids, **kw):
    r = ix.rank_ids(_cuda(q), _cuda(ids), **kw)
    assert r.rank.dtype == torch.int64 and r.score.dtype == torch.float32 and r.rank.shape == r.score.shape == tuple(np.shape(ids))
    return r.rank.cpu().numpy(), r.score.cpu().numpy()


def _count(ix, q, thr, tie=None, **kw):
    c = ix.count_above(_cuda(q), _cuda(thr), tie_ids=None if tie is None else _cuda(tie), **kw)
    assert c.dtype == torch.int64 and c.shape == tuple(np.shape(thr))
    return c.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


# ---- integer data: every store, width, batch and list length, every row of the store --------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", STORES)
def test_ranks_are_exact_for_every_row(n, d, dtype):
    q, x, s = _int_case(d)
    want = _all_ranks(d, n)
    seen = np.zeros(n, dtype=bool)
    with _index(x[:n], dtype) as ix:
        for nq in BATCHES:
            for m in SLOTS:
                ids = ((7 * nq + 13 * m + np.arange(nq * m, dtype=np.int64)) % n).reshape(nq, m)  # consecutive rows: 300 x 64 lists all
                rank, score = _rank(ix, q[:nq], ids)
                np.testing.assert_array_equal(rank, np.take_along_axis(want[:nq], ids, axis=1), err_msg=f"nq {nq} m {m}")
                assert _same_bits(score, np.take_along_axis(s[:nq, :n], ids, axis=1)), (nq, m)
                if nq * m >= n:
                    seen[:] = True
                else:
                    seen[ids.ravel()] = True
        assert seen.all()
        # the contract: the hits of a search come back at their own positions with their own bits
        k = min(n, 64)
        ss, si = ix.search(_cuda(q[:129]), k)
        rank, score = _rank(ix, q[:129], si.cpu().numpy())
        np.testing.assert_array_equal(rank, np.broadcast_to(np.arange(k), (129, k)))
        assert _same_bits(score, ss.cpu().numpy())


# ---- Gaussian data: the pick reproduces the scan's bits ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1500, 2048])
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_search_hits_come_back_at_their_positions_with_their_bits(dim, dtype, seed, n):
    q, x = gauss_case(dim, seed)
    x = x[:n]
    qd = _cuda(q)
    with _index(x, dtype) as ix:
        ss, si = ix.search(qd, n)  # k = ntotal: the whole order
        assert bool(torch.isfinite(ss).all()) and bool((si >= 0).all())
        for c0 in range(0, n, 64):
            r = ix.rank_ids(qd, si[:, c0:c0 + 64].contiguous())
            w = min(64, n - c0)
            assert torch.equal(r.rank, torch.arange(c0, c0 + w, device="cuda").expand(len(q), w)), c0
            assert torch.equal(r.score.view(torch.int32), ss[:, c0:c0 + w].contiguous().view(torch.int32)), c0


# ---- slots -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_absent_slots_duplicates_the_last_tile_and_id_base(dtype):
    q, x, s = _int_case(65)
    n, nq, base = 300, 70, 1000  # two tiles, the second holds 44 rows
    ids = np.empty((nq, 9), dtype=np.int64)
    ids[:, 0] = 299                      # the gold row is the last row of the partly filled tile
    ids[:, 1] = -1                       # empty
    ids[:, 2] = 300                      # the first row past ntotal
    ids[:, 3] = np.arange(nq) % 256      # anything
    ids[:, 4] = ids[:, 3]                # a duplicate: an independent slot
    ids[:, 5] = 2 ** 40                  # far out of range
    ids[:, 6] = 256                      # the first row of the last tile
    ids[:, 7] = -(2 ** 40)
    ids[:, 8] = 255
    want_rank, want_score = R.rank_ids(s[:nq, :n], ids)
    assert (want_rank[:, [1, 2, 5, 7]] == -1).all() and np.isneginf(want_score[:, [1, 2, 5, 7]]).all()
    with _index(x[:n], dtype) as ix:
        rank, score = _rank(ix, q[:nq], ids)
        np.testing.assert_array_equal(rank, want_rank)
        assert _same_bits(score, want_score)
        np.testing.assert_array_equal(rank[:, 3], rank[:, 4])
        # id_base: the same rows under global ids; an id below the base is absent
        shifted = np.where(ids >= 0, ids + base, ids)
        shifted[:, 7] = base - 1
        rank2, score2 = _rank(ix, q[:nq], shifted, id_base=base)
        np.testing.assert_array_equal(rank2, want_rank)
        assert _same_bits(score2, want_score)
        ref = R.rank_ids(s[:nq, :n], shifted, id_base=base)
        np.testing.assert_array_equal(rank2, ref[0])
        # a ragged list of lists is padded with -1
        r = ix.rank_ids(_cuda(q[:2]), [[299], [5, 6, 7]])
        np.testing.assert_array_equal(r.rank.cpu().numpy(), R.rank_ids(s[:2, :n], np.array([[299, -1, -1], [5, 6, 7]]))[0])


# ---- stale rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_past_ntotal_are_never_counted(dtype):
    q, x, s = _int_case(65)
    nq = 129
    ids = ((np.arange(nq * 8, dtype=np.int64) * 37) % 700).reshape(nq, 8)
    ids[:, 7] = 700 + np.arange(nq)  # a stale row as a target: absent
    with _index(x, dtype, capacity=3000) as ix:
        ix.reset()
        ix.add(x[2300:])  # 700 rows; rows 700 .. 2999 of the store still hold the first ingest
        assert ix.ntotal == 700
        rank, score = _rank(ix, q[:nq], ids)
        want = R.rank_ids(s[:nq, 2300:], ids)
        np.testing.assert_array_equal(rank, want[0])
        assert _same_bits(score, want[1]) and (rank[:, 7] == -1).all()
        thr = np.full((nq, 1), -np.inf, dtype=np.float32)
        np.testing.assert_array_equal(_count(ix, q[:nq], thr, np.full((nq, 1), 2 ** 40)), np.full((nq, 1), 700))
    with _index(x[:700], dtype, capacity=3000) as ix:  # nothing beyond ntotal was ever written
        np.testing.assert_array_equal(_rank(ix, q[:nq], ids)[0], R.rank_ids(s[:nq, :700], ids)[0])
    with _index(x[:300], dtype, capacity=300) as ix:  # the last tile reaches past the capacity
        np.testing.assert_array_equal(_rank(ix, q[:65], ids[:65] % 300)[0], R.rank_ids(s[:65, :300], ids[:65] % 300)[0])


# ---- non-finite scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_are_never_counted_and_infinite_scores_rank(dtype):
    q, x, _ = _int_case(65)
    q = np.array(q[:70])
    q[:, 0] = 1.0
    s = (q.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    xn = np.array(x)
    xn[7, 3] = np.nan       # every score of row 7 is NaN
    xn[300, 0] = -np.inf    # every score of rows 300 and 1700 is -inf: they tie at the very end, by id
    xn[1700, 0] = -np.inf
    xn[2999, 0] = np.inf    # +inf for every query (q[:, 0] = 1)
    s[:, 7], s[:, 300], s[:, 1700], s[:, 2999] = np.nan, -np.inf, -np.inf, np.inf
    ids = np.tile(np.array([7, 300, 1700, 2999, 0, 8], dtype=np.int64), (70, 1))
    want_rank, want_score = R.rank_ids(s, ids)
    assert (want_rank[:, 0] == -1).all() and (want_rank[:, 1] == 2997).all() and (want_rank[:, 2] == 2998).all() and (want_rank[:, 3] == 0).all()
    with _index(xn, dtype) as ix:
        rank, score = _rank(ix, q, ids)
        np.testing.assert_array_equal(rank, want_rank)
        assert np.isnan(score[:, 0]).all()  # the score as computed
        assert _same_bits(score[:, 1:], want_score[:, 1:])
        thr = np.tile(np.array([np.inf, -np.inf, np.nan, 0.0], dtype=np.float32), (70, 1))
        np.testing.assert_array_equal(_count(ix, q, thr), R.count(s, thr))
        tie = np.full((70, 4), 3000, dtype=np.int64)
        got = _count(ix, q, thr, tie)
        np.testing.assert_array_equal(got, R.count(s, thr, tie))
        assert (got[:, 0] == 1).all() and (got[:, 1] == 2999).all() and (got[:, 2] == -1).all()  # the NaN row is in neither count


# ---- subset labels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 132])
def test_subset_labels(nq, dtype):
    q, x, s = _int_case(65)
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    ids = ((np.arange(nq * 9, dtype=np.int64) * 101) % len(x)).reshape(nq, 9)
    ids[:, 0] = 4 * (np.arange(nq) % 700)  # label 0: inside the subset of queries 0, 4, ..
    want_rank, want_score = R.rank_ids(s[:nq], ids, eligible=elig)
    assert (want_rank[3::4] == -1).all() and (want_rank[0::4, 0] >= 0).all() and (want_rank[1::4, 0] == -1).all()
    thr = np.tile(np.array([[0.0, 100.5, -np.inf]], dtype=np.float32), (nq, 1))
    tie = np.tile(np.array([[1500, 0, 5000]], dtype=np.int64), (nq, 1))
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        rank, score = _rank(ix, q[:nq], ids, subset=sub)
        np.testing.assert_array_equal(rank, want_rank)  # among the eligible rows only; a target outside the subset is absent
        assert _same_bits(score, want_score)
        got = _count(ix, q[:nq], thr, tie, subset=sub)
        np.testing.assert_array_equal(got, R.count(s[:nq], thr, tie, eligible=elig))
        np.testing.assert_array_equal(got[:, 2], elig.sum(axis=1))
        # row labels set but no query labels given: unrestricted
        np.testing.assert_array_equal(_rank(ix, q[:nq], ids)[0], R.rank_ids(s[:nq], ids)[0])


# ---- batches above one slice --------------------------------------------------------------------------------------------------------------
def test_a_batch_of_two_slices_with_labels_ids_and_thresholds_offset_into_the_second():
    _, x, _ = _int_case(64)
    n, nq = 300, 1100  # slices of 1024 and 76 queries: the second runs at another query-tile count, from offsets into every input
    rng = np.random.default_rng(1100)
    q = rng.integers(-8, 9, size=(nq, 64)).astype(np.float32)
    s = (q.astype(np.float64) @ x[:n].astype(np.float64).T).astype(np.float32)
    labels = (np.arange(n) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[rng.integers(0, 4, size=nq)]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(n, dtype=bool) for row in sub])
    ids = rng.integers(-1, n + 1, size=(nq, 3))
    thr = np.take_along_axis(s, rng.integers(0, n, size=(nq, 3)), axis=1)
    tie = rng.integers(0, n, size=(nq, 3))
    with _index(x[:n], "float16") as ix:
        ix.set_row_labels(labels)
        rank, score = _rank(ix, q, ids, subset=sub)
        want = R.rank_ids(s, ids, eligible=elig)
        np.testing.assert_array_equal(rank, want[0])
        assert _same_bits(score, want[1])
        np.testing.assert_array_equal(_count(ix, q, thr, tie, subset=sub), R.count(s, thr, tie, eligible=elig))
        np.testing.assert_array_equal(rank[1024:], _rank(ix, q[1024:], ids[1024:], subset=sub[1024:])[0])


# ---- thresholds -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,n", [(1, 3000), (65, 1500), (768, 257)])
def test_count_above_thresholds(d, n, dtype):
    q, x, s = _int_case(d)
    s = s[:, :n]
    nq = 129
    rng = np.random.default_rng(d)
    on = np.take_along_axis(s[:nq], rng.integers(0, n, size=(nq, 4)), axis=1)             # on the integer scores
    special = np.tile(np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 0.5, -0.5], dtype=np.float32), (nq, 1))
    thr = np.concatenate([on, on + np.float32(0.5), special], axis=1)                      # and between them
    tie = rng.integers(-5, n + 5, size=thr.shape)
    tie[:, 0], tie[:, 1] = 0, n
    with _index(x[:n], dtype) as ix:
        strict = _count(ix, q[:nq], thr)
        np.testing.assert_array_equal(strict, R.count(s[:nq], thr))
        tied = _count(ix, q[:nq], thr, tie)
        np.testing.assert_array_equal(tied, R.count(s[:nq], thr, tie))
        assert (strict[:, 10] == -1).all() and (strict[:, 8] == 0).all() and (strict[:, 9] == n).all()
        np.testing.assert_array_equal(strict[:, 11], strict[:, 12])  # -0.0 and +0.0 are one threshold
        np.testing.assert_array_equal(tied[:, 11], R.count(s[:nq], np.zeros((nq, 1), dtype=np.float32), tie[:, 11:12])[:, 0])
        if d == 1:
            assert ((s[:nq] == 0).sum(axis=1) > 100).all()  # zero scores of both signs in the products: they tie with either threshold
        assert (tied >= strict).all() and (tied[:, 4:8] == strict[:, 4:8]).all()  # nothing ties with a half-integer
        np.testing.assert_array_equal(_count(ix, q[:nq], thr, tie + 777, id_base=777), tied)
        # count_above(q, score, tie_ids=ids) is rank_ids(q, ids).rank
        ids = rng.integers(0, n, size=(nq, 9))
        rank, score = _rank(ix, q[:nq], ids)
        np.testing.assert_array_equal(_count(ix, q[:nq], score, ids), rank)
        # host inputs are uploaded by the call
        got = ix.count_above(q[:5], thr[:5], tie_ids=tie[:5])
        np.testing.assert_array_equal(got.cpu().numpy(), tied[:5])


# ---- batch independence and repeatability ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 768])
def test_a_query_has_the_same_result_in_any_batch_and_on_every_repeat(d, dtype):
    q, x, _ = _int_case(d)
    rng = np.random.default_rng(d)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)  # inexact sums: the order of summation matters
    qg = (q + rng.standard_normal(q.shape)).astype(np.float32)
    ids = rng.integers(0, len(x), size=(300, 8))
    with _index(xg, dtype) as ix:
        a = _rank(ix, qg, ids)
        b = _rank(ix, qg, ids)
        c = _rank(ix, qg[:65], ids[:65])
        assert np.array_equal(a[0], b[0]) and _same_bits(a[1], b[1])
        assert np.array_equal(a[0][:65], c[0]) and _same_bits(a[1][:65], c[1])
        for j in (0, 63, 64, 217, 299):
            one = _rank(ix, qg[j:j + 1], ids[j:j + 1])
            assert np.array_equal(a[0][j:j + 1], one[0]) and _same_bits(a[1][j:j + 1], one[1]), j
        moved = _rank(ix, qg[::-1], ids[::-1])  # every query at another place in the batch
        assert np.array_equal(a[0], moved[0][::-1]) and _same_bits(a[1], moved[1][::-1])
        fewer = _rank(ix, qg, ids[:, :3])       # and with another list length
        assert np.array_equal(a[0][:, :3], fewer[0]) and _same_bits(a[1][:, :3], fewer[1])


# ---- beside searches -------------------------------------------------------------------------------------------------------------------
def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x, _ = _int_case(768)
    qd = _cuda(q[:129])
    ids = _cuda(((np.arange(129 * 8, dtype=np.int64) * 37) % 3000).reshape(129, 8))
    with _index(x, "float16") as ix:
        serial_s, serial_i = ix.search(qd, 100)
        serial = ix.rank_ids(qd, ids)
        serial_c = ix.count_above(qd, serial.score, tie_ids=ids)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            r = ix.rank_ids(qd, ids)
            c = ix.count_above(qd, r.score, tie_ids=ids)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert torch.equal(r.rank, serial.rank) and torch.equal(r.score.view(torch.int32), serial.score.view(torch.int32))
        assert torch.equal(c, serial_c) and torch.equal(c, r.rank)
        assert ix.get_stat("last_overflow") == 0


# ---- node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 65])
@pytest.mark.parametrize("n_shards,capacity", [(1, 3000), (2, 3000), (3, 3000), (3, 12000)])
def test_node_index_equals_the_flat_index(n_shards, capacity, d):
    from vod_amd.index import HipNodeIndex

    q, x, s = _int_case(d)
    nq = 129
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    rng = np.random.default_rng(n_shards)
    ids = rng.integers(0, len(x), size=(nq, 9))
    ids[:, 0] = 1000 + np.arange(nq)  # owned by the middle one of 3 shards of 1000 rows
    ids[:, 1], ids[:, 2], ids[:, 3], ids[:, 4] = 999, 1000, 1999, 2000  # the shard edges
    ids[:, 7], ids[:, 8] = -1, len(x)
    if d == 1:  # scores in [-64, 64]: the middle shard's targets tie with rows of both neighbours
        tied = s[:nq, 1000:1000 + nq].diagonal()
        assert ((s[:nq, :1000] == tied[:, None]).any(axis=1) & (s[:nq, 2000:] == tied[:, None]).any(axis=1)).all()
    thr = np.concatenate([np.take_along_axis(s[:nq], ids[:, :4], axis=1), np.array([[np.nan, 0.5, -np.inf]] * nq, dtype=np.float32)], axis=1)
    tie = np.concatenate([ids[:, :4], np.array([[5, 1500, 2 ** 40]] * nq)], axis=1)
    with _index(x, "float16") as ix:
        flat = _rank(ix, q[:nq], ids)
        flat_c = _count(ix, q[:nq], thr, tie)
        flat_strict = _count(ix, q[:nq], thr)
        ix.set_row_labels(labels)
        flat_sub = _rank(ix, q[:nq], ids, subset=sub)
        flat_sub_c = _count(ix, q[:nq], thr, tie, subset=sub)
    np.testing.assert_array_equal(flat[0], R.rank_ids(s[:nq], ids)[0])
    with HipNodeIndex(d, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        nx.add(x.astype(np.float32))
        got = nx.rank_ids(np.array(q[:nq]), ids)
        got_c = nx.count_above(np.array(q[:nq]), thr, tie_ids=tie)
        got_strict = nx.count_above(np.array(q[:nq]), thr)
        nx.set_row_labels(labels)
        got_sub = nx.rank_ids(np.array(q[:nq]), ids, subset=sub)
        got_sub_c = nx.count_above(np.array(q[:nq]), thr, tie_ids=tie, subset=sub)
    for res, ref in ((got, flat), (got_sub, flat_sub)):
        assert isinstance(res.rank, np.ndarray) and res.rank.dtype == np.int64 and res.score.dtype == np.float32
        np.testing.assert_array_equal(res.rank, ref[0])
        assert _same_bits(res.score, ref[1])
    for res, ref in ((got_c, flat_c), (got_strict, flat_strict), (got_sub_c, flat_sub_c)):
        assert res.dtype == np.int64
        np.testing.assert_array_equal(res, ref)


# ---- refusals and empty cases ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    q, x, s = _int_case(65)
    qd = _cuda(q[:5])
    ids = _cuda(np.arange(10, dtype=np.int64).reshape(5, 2))
    thr = torch.zeros((5, 2), device="cuda")
    out_r = torch.full((5, 2), 123, dtype=torch.int64, device="cuda")
    out_s = torch.full((5, 2), 123.0, device="cuda")
    out_w = torch.full((5, 2), 123, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def rank(h, queries=qd, code=2, nq=5, lst=ids, m=2, lab=None, n_lab=0, o_r=out_r, o_s=out_s):
        return lib.vodhip_index_rank_ids(h, ptr(queries), code, nq, ptr(lst), m, 0, ptr(lab), n_lab, ptr(o_r), ptr(o_s), None)

    def count(h, queries=qd, code=2, nq=5, t=thr, tie=None, m=2, lab=None, n_lab=0, o=out_r):
        return lib.vodhip_index_count_above(h, ptr(queries), code, nq, ptr(t), ptr(tie), m, 0, ptr(lab), n_lab, ptr(o), None)

    def pick(h, queries=qd, code=2, nq=5, lst=ids, m=2, lab=None, n_lab=0, o_s=out_s, o_w=out_w):
        return lib.vodhip_index_scan_score_ids(h, ptr(queries), code, nq, ptr(lst), m, 0, ptr(lab), n_lab, ptr(o_s), ptr(o_w), None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x[:300], "float16") as ix:
        for call in (rank, count, pick):
            refused(call(None), "index is NULL")
            refused(call(ix._h, queries=None), "invalid query pointer")
            refused(call(ix._h, nq=-1), "invalid query pointer")
            refused(call(ix._h, code=3), "invalid q_dtype 3")
            refused(call(ix._h, code=-1), "invalid q_dtype -1")
            refused(call(ix._h, m=0), "m=0: must be in [1, 64]")
            refused(call(ix._h, m=65), "m=65: must be in [1, 64]")
            refused(call(ix._h, lab=lab, n_lab=0), "n_per_query must be in [1, 64]")
            refused(call(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
            refused(call(ix._h, lab=lab, n_lab=2), "set the row labels first")
        refused(rank(ix._h, lst=None), "ids is NULL")
        refused(pick(ix._h, lst=None), "ids is NULL")
        refused(count(ix._h, t=None), "thresholds is NULL")
        refused(rank(ix._h, o_r=None), "out_ranks is NULL")
        refused(rank(ix._h, o_s=None), "out_scores is NULL")
        refused(pick(ix._h, o_s=None), "out_scores is NULL")
        refused(count(ix._h, o=None), "out_counts is NULL")
        with pytest.raises(_native.NativeLibraryError, match="m=65"):
            ix.rank_ids(qd, torch.zeros((5, 65), dtype=torch.int64, device="cuda"))
        with pytest.raises(ValueError):
            ix.rank_ids(qd, ids[:4])
        with pytest.raises(ValueError):
            ix.count_above(qd, thr, tie_ids=ids[:, :1])
        torch.cuda.synchronize()
        assert (out_r == 123).all() and (out_s == 123.0).all() and (out_w == 123).all()  # a refused call writes nothing
        # nq == 0: returns 0, needs nothing, writes nothing
        assert rank(ix._h, queries=None, nq=0, lst=None, o_r=None, o_s=None) == 0
        assert count(ix._h, queries=None, nq=0, t=None, o=None) == 0
        assert pick(ix._h, queries=None, nq=0, lst=None, o_s=None, o_w=None) == 0
        empty = ix.rank_ids(torch.zeros((0, 65), device="cuda"), torch.zeros((0, 3), dtype=torch.int64, device="cuda"))
        assert empty.rank.shape == (0, 3) and empty.score.shape == (0, 3)
        assert ix.count_above(torch.zeros((0, 65), device="cuda"), torch.zeros((0, 3), device="cuda")).shape == (0, 3)
        # the pick alone: the scores of rank_ids and the local rows; out_rows may be NULL
        assert pick(ix._h) == 0 and pick(ix._h, o_w=None) == 0
        torch.cuda.synchronize()
        want = R.rank_ids(s[:5, :300], ids.cpu().numpy())
        assert _same_bits(out_s.cpu().numpy(), want[1]) and torch.equal(out_w.cpu(), ids.cpu().to(torch.int32))
        # after all that the index still searches, and the calls still work
        sc, _ = ix.search(qd, 3)
        np.testing.assert_array_equal(sc.cpu().numpy(), np.sort(s[:5, :300], axis=1)[:, ::-1][:, :3])
        np.testing.assert_array_equal(_rank(ix, q[:5], ids.cpu().numpy())[0], want[0])
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="rank_ids is not supported on an L2 index"):
            ix.rank_ids(qd, ids)
        with pytest.raises(_native.NativeLibraryError, match="count_above is not supported on an L2 index"):
            ix.count_above(qd, thr)
        refused(pick(ix._h), "scan_score_ids is not supported on an L2 index")
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="rank_ids is not supported on a VODHIP_EXACT_F32 store"):
            ix.rank_ids(qd, ids)
        with pytest.raises(_native.NativeLibraryError, match="count_above is not supported on a VODHIP_EXACT_F32 store"):
            ix.count_above(qd, thr)
        refused(pick(ix._h), "scan_score_ids is not supported on a VODHIP_EXACT_F32 store")
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty index
        rank_e, score_e = _rank(ix, q[:5], ids.cpu().numpy())
        assert (rank_e == -1).all() and np.isneginf(score_e).all()
        cnt = _count(ix, q[:5], np.array([[0.0, np.nan]] * 5, dtype=np.float32))
        np.testing.assert_array_equal(cnt, [[0, -1]] * 5)
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        got = nx.rank_ids(np.array(q[:5]), ids.cpu().numpy())  # empty
        assert (got.rank == -1).all() and np.isneginf(got.score).all()
        nx.add(x[:600].astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="m=65"):
            nx.rank_ids(np.array(q[:5]), np.zeros((5, 65), dtype=np.int64))
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.count_above(np.array(q[:5]), np.zeros((5, 2), dtype=np.float32), subset=np.zeros((5, 2), dtype=np.int32))
        assert nx.rank_ids(np.zeros((0, 65), dtype=np.float32), np.zeros((0, 2), dtype=np.int64)).rank.shape == (0, 2)
        got = nx.rank_ids(np.array(q[:5]), ids.cpu().numpy())
        np.testing.assert_array_equal(got.rank, R.rank_ids(s[:5, :600], ids.cpu().numpy())[0])
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.rank_ids(np.array(q[:5]), ids.cpu().numpy())
