"""`range_search`, `outranking` and `posterior_support` of `HipFlatIndex` and `HipNodeIndex` on the GPU.

Everything but the last comparison of the posterior-support test is EXACT: list lengths and ids are integers, scores are compared as
bits.  The contract is the PREFIX IDENTITY: with hit `p` of a search's full order as threshold and tie id, `range_search` returns
exactly the `p` hits ahead of it, with their bits.  (A search returns at most 2048 hits; for the 2100-row store the full order is the
scan's scores - `rank_ids`, 64 listed rows per call - sorted by (score desc, id asc), checked against the search on its 2048 hits.)
Integer data (values in [-8, 8]: every score an exact integer in float32, so the restatement's score matrix IS the scan's) for the
count identity with `count_above`, the edges, the two-slice batch, the capacity rules and the node index.
"""
import ctypes
import functools

import numpy as np
import pytest

import partition_ref as P
import range_ref as G
import rank_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
INF = np.float32(np.inf)


def _index(x, dtype="float16", capacity=None, dim=None, **kw):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, **kw)
    if len(x):
        ix.add(x)
    return ix


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _range(ix, q, thr, tie=None, **kw):
    """(lims, scores, ids) as NumPy; the status words of the call must read 0"""
    r = ix.range_search(_cuda(q), _cuda(np.asarray(thr, dtype=np.float32)), tie_ids=None if tie is None else _cuda(np.asarray(tie, dtype=np.int64)), **kw)
    assert r.lims.dtype == torch.int64 and r.scores.dtype == torch.float32 and r.ids.dtype == torch.int64
    assert r.lims.shape == (len(q) + 1,) and r.scores.shape == r.ids.shape == (int(r.lims[-1]),)
    assert ix.get_stat("last_range_selfcheck") == 0 and ix.get_stat("last_range_overflow") == 0
    return r.lims.cpu().numpy(), r.scores.cpu().numpy(), r.ids.cpu().numpy()


def _same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(_bits(got[1]), _bits(want[1]))


@functools.lru_cache(maxsize=None)
def _int_case(d, n=3000, nq=300):
    """integer rows / queries and their exact float32 scores (test_rank_ids_gpu.py's construction)"""
    rng = np.random.default_rng(4000 + d)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    s64 = q.astype(np.float64) @ x.astype(np.float64).T
    s = s64.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), s64)
    for a in (q, x, s):
        a.setflags(write=False)
    return q, x, s


@functools.lru_cache(maxsize=None)
def _gauss_case(d, n=2100, nq=130):
    rng = np.random.default_rng(7000 + d)
    q, x = rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    q.setflags(write=False)
    x.setflags(write=False)
    return q, x


def _scan_scores(ix, qd, n):
    """the scan's score of every (query, row): [nq, n] float32, 64 listed rows per `rank_ids` call"""
    cols = []
    for c0 in range(0, n, 64):
        ids = torch.arange(c0, min(n, c0 + 64), device="cuda").expand(qd.shape[0], -1).contiguous()
        cols.append(ix.rank_ids(qd, ids).score)
    return torch.cat(cols, dim=1).cpu().numpy()


def _full_order(ix, qd, n):
    """(scores, ids) [nq, n]: what a search of unlimited depth returns"""
    k = min(n, 2048)
    ss, si = ix.search(qd, k)
    ss, si = ss.cpu().numpy(), si.cpu().numpy()
    if k == n:
        return ss, si
    s = _scan_scores(ix, qd, n)
    order = np.lexsort((np.broadcast_to(np.arange(n), s.shape), -(s.astype(np.float64) + 0.0)), axis=1)  # (score desc, id asc)
    full_s = np.take_along_axis(s, order, axis=1)
    np.testing.assert_array_equal(order[:, :k], si)
    np.testing.assert_array_equal(_bits(full_s[:, :k]), _bits(ss))
    return full_s, order.astype(np.int64)


# ---- 1. the prefix identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [64, 200])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 700, 2100])
def test_prefix_identity_with_a_search(n, d, dtype):
    q, x = _gauss_case(d)
    with _index(x[:n], dtype) as ix:
        full_s, full_i = _full_order(ix, _cuda(q), n)
        assert np.isfinite(full_s).all() and (np.sort(full_i, axis=1) == np.arange(n)).all()
        for nq in (1, 64, 65, 130):
            for p in sorted({0, 1, 255, 256, 257, n - 1}):
                if p >= n:
                    continue
                lims, scores, ids = _range(ix, q[:nq], full_s[:nq, p], full_i[:nq, p], order="score")
                np.testing.assert_array_equal(np.diff(lims), np.full(nq, p), err_msg=f"nq {nq} p {p}")
                np.testing.assert_array_equal(ids.reshape(nq, p), full_i[:nq, :p], err_msg=f"nq {nq} p {p}")
                np.testing.assert_array_equal(_bits(scores.reshape(nq, p)), _bits(full_s[:nq, :p]), err_msg=f"nq {nq} p {p}")
            lims, scores, ids = _range(ix, q[:nq], np.full(nq, -INF), inclusive=True)
            np.testing.assert_array_equal(lims, n * np.arange(nq + 1))
            np.testing.assert_array_equal(ids.reshape(nq, n), np.broadcast_to(np.arange(n), (nq, n)))
            by_id = np.take_along_axis(full_s[:nq], np.argsort(full_i[:nq], axis=1), axis=1)
            np.testing.assert_array_equal(_bits(scores.reshape(nq, n)), _bits(by_id))


# ---- 2. the count identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [64, 130])
def test_list_lengths_equal_count_above_on_heavily_tied_data(nq, dtype):
    q, x, s = _int_case(1)  # scores in [-64, 64]: hundreds of ties per score, zeros of both signs among the products
    n = 700                 # three tiles
    s = s[:nq, :n]
    rng = np.random.default_rng(nq)
    on = s[np.arange(nq), rng.integers(0, n, size=nq)]
    assert ((s == 0).sum(axis=1) > 10).all()
    with _index(x[:n], dtype) as ix:
        qd = _cuda(q[:nq])
        for thr in (on, on + np.float32(0.5), np.full(nq, np.float32(-0.0)), np.zeros(nq, dtype=np.float32)):
            ties = {"strict": None, "inclusive": np.full(nq, G.TIE_PAST_EVERY_ROW),
                    "middle tile": rng.integers(256, 512, size=nq).astype(np.int64),  # the tie row's own tile is the second of three
                    "tile edges": np.array([0, 1, 255, 256, 257, 511, 512, 699, 700, 5000], dtype=np.int64)[np.arange(nq) % 10]}
            for name, tie in ties.items():
                if name == "inclusive":
                    got = _range(ix, q[:nq], thr, inclusive=True)
                else:
                    got = _range(ix, q[:nq], thr, tie)
                cnt = ix.count_above(qd, _cuda(thr[:, None]), tie_ids=None if tie is None else _cuda(tie[:, None]))[:, 0].cpu().numpy()
                np.testing.assert_array_equal(np.diff(got[0]), cnt, err_msg=name)
                _same(got, G.range_search(s, thr, tie))
        zeros = [_range(ix, q[:nq], np.full(nq, np.float32(z)), np.full(nq, 350)) for z in (-0.0, 0.0)]
        _same(zeros[0], zeros[1])  # -0.0 and +0.0 are one threshold


# ---- 3. order and determinism ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_ids_ascend_and_a_query_has_the_same_bytes_in_any_batch_and_on_every_repeat(dtype):
    q, x = _gauss_case(200)
    n = 2100
    with _index(x, dtype) as ix:
        s = _scan_scores(ix, _cuda(q), n)
        thr = np.sort(s, axis=1)[:, n - 300]  # about 300 hits per query
        a = _range(ix, q, thr)
        for j in range(len(q)):
            seg = a[2][a[0][j]:a[0][j + 1]]
            assert len(seg) > 200 and (np.diff(seg) > 0).all()
        _same(a, G.range_search(s, thr))
        _same(_range(ix, q, thr), a)  # a repeat
        one = _range(ix, q[70:71], thr[70:71])  # query 70 of 130, alone
        np.testing.assert_array_equal(one[2], a[2][a[0][70]:a[0][71]])
        np.testing.assert_array_equal(_bits(one[1]), _bits(a[1][a[0][70]:a[0][71]]))
        b = _range(ix, q[::-1], thr[::-1])  # every query at another place of the batch
        for j in (0, 63, 64, 129):
            k = len(q) - 1 - j
            np.testing.assert_array_equal(b[2][b[0][k]:b[0][k + 1]], a[2][a[0][j]:a[0][j + 1]])
            np.testing.assert_array_equal(_bits(b[1][b[0][k]:b[0][k + 1]]), _bits(a[1][a[0][j]:a[0][j + 1]]))


# ---- 4. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_stale_rows_nan_rows_infinite_scores_and_special_thresholds(dtype):
    q, x, s = _int_case(65)
    nq = 70
    q = np.array(q[:nq])
    q[:, 0] = 1.0
    s = (q.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    with _index(x, dtype, capacity=3000) as ix:  # rows past ntotal after a reset and a shorter add
        ix.reset()
        ix.add(x[2300:])
        assert ix.ntotal == 700
        got = _range(ix, q, np.full(nq, -INF), inclusive=True)
        _same(got, G.range_search(s[:, 2300:], np.full(nq, -INF), inclusive=True))
        assert (np.diff(got[0]) == 700).all()
        thr = s[np.arange(nq), 2300 + (np.arange(nq) * 7) % 700]
        tie = (np.arange(nq) * 13) % 800  # some past ntotal
        _same(_range(ix, q, thr, tie), G.range_search(s[:, 2300:], thr, tie))
    xn = np.array(x[:700])
    xn[7, 3] = np.nan       # every score of row 7 is NaN
    xn[300, 0] = -np.inf    # every score of rows 300 and 600 is -inf
    xn[600, 0] = -np.inf
    xn[699, 0] = np.inf     # +inf for every query (q[:, 0] = 1)
    sn = np.array(s[:, :700])
    sn[:, 7], sn[:, 300], sn[:, 600], sn[:, 699] = np.nan, -np.inf, -np.inf, np.inf
    with _index(xn, dtype) as ix:
        for thr_v, tie_v, inclusive in ((-INF, None, False), (-INF, None, True), (-INF, 600, False), (INF, None, False), (INF, None, True),
                                        (INF, 699, False), (INF, 700, False), (np.nan, None, False), (np.nan, None, True), (0.0, 350, False)):
            thr = np.full(nq, thr_v, dtype=np.float32)
            tie = None if tie_v is None else np.full(nq, tie_v, dtype=np.int64)
            got = _range(ix, q, thr, tie, inclusive=inclusive)
            _same(got, G.range_search(sn, thr, tie, inclusive=inclusive))
            assert 7 not in got[2]  # the NaN row is in no list
        assert (np.diff(_range(ix, q, np.full(nq, -INF))[0]) == 697).all()                       # strict: above -inf
        assert (np.diff(_range(ix, q, np.full(nq, -INF), inclusive=True)[0]) == 699).all()       # every eligible row
        assert (np.diff(_range(ix, q, np.full(nq, INF), inclusive=True)[0]) == 1).all()
        assert _range(ix, q, np.full(nq, np.nan), inclusive=True)[0][-1] == 0
        mixed = np.where(np.arange(nq) % 3 == 0, np.float32(np.nan), np.float32(10.0)).astype(np.float32)
        _same(_range(ix, q, mixed), G.range_search(sn, mixed))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [3, 70])
def test_subset_labels_and_id_base(nq, dtype):
    q, x, s = _int_case(65)
    n = 700
    labels = (np.arange(n) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(n, dtype=bool) for row in sub])
    thr = s[np.arange(nq), (np.arange(nq) * 31) % n]
    tie = (np.arange(nq) * 53) % n
    with _index(x[:n], dtype) as ix:
        ix.set_row_labels(labels)
        got = _range(ix, q[:nq], thr, tie, subset=sub)
        _same(got, G.range_search(s[:nq, :n], thr, tie, eligible=elig))
        assert (np.diff(got[0])[3::4] == 0).all()  # a label no row has
        _same(_range(ix, q[:nq], thr, tie), G.range_search(s[:nq, :n], thr, tie))  # row labels set, no query labels: unrestricted
        base = 10 ** 12
        shifted = _range(ix, q[:nq], thr, tie + base, subset=sub, id_base=base)
        _same(shifted, G.range_search(s[:nq, :n], thr, tie + base, eligible=elig, id_base=base))
        np.testing.assert_array_equal(shifted[2], got[2] + base)
        below = _range(ix, q[:nq], thr, tie, id_base=base)  # tie ids below the base: strict
        _same(below, G.range_search(s[:nq, :n], thr, None, id_base=base))


# ---- 5. a batch of two slices ------------------------------------------------------------------------------------------------------------
def test_lims_continue_across_the_slice_boundary():
    _, x, _ = _int_case(64)
    n, nq = 300, 1100  # slices of 1024 and 76 queries
    rng = np.random.default_rng(1100)
    q = rng.integers(-8, 9, size=(nq, 64)).astype(np.float32)
    s = (q.astype(np.float64) @ x[:n].astype(np.float64).T).astype(np.float32)
    thr = s[np.arange(nq), rng.integers(0, n, size=nq)]
    tie = rng.integers(0, n + 1, size=nq)
    labels = (np.arange(n) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[rng.integers(0, 4, size=nq)]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(n, dtype=bool) for row in sub])
    with _index(x[:n], "float16") as ix:
        ix.set_row_labels(labels)
        got = _range(ix, q, thr, tie, subset=sub)
        _same(got, G.range_search(s, thr, tie, eligible=elig))
        assert got[0][1024] > 0 and got[0][-1] > got[0][1024]
        tail = _range(ix, q[1024:], thr[1024:], tie[1024:], subset=sub[1024:])
        np.testing.assert_array_equal(tail[0], got[0][1024:] - got[0][1024])
        np.testing.assert_array_equal(tail[2], got[2][got[0][1024]:])


# ---- 6. capacity -------------------------------------------------------------------------------------------------------------------------
def test_sizing_call_capacity_overflow_and_status_words():
    from vod_amd import _native

    lib = _native.load_library()
    q, x, s = _int_case(65)
    n, nq = 700, 70
    thr = s[np.arange(nq), (np.arange(nq) * 31) % n]
    want = G.range_search(s[:nq, :n], thr)
    total = int(want[0][-1])
    assert total > 1000
    with _index(x[:n], "float16") as ix:
        qd, td = _cuda(q[:nq]), _cuda(thr)
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

        def call(lims, scores, ids, capacity):
            return lib.vodhip_index_range_search(ix._h, ptr(qd), 2, nq, ptr(td), None, 0, None, 0, ptr(lims), ptr(scores), ptr(ids), capacity, None)

        lims = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
        assert call(lims, None, None, 0) == 0  # the sizing call
        torch.cuda.synchronize()
        np.testing.assert_array_equal(lims.cpu().numpy(), want[0])
        _same(_range(ix, q[:nq], thr), want)                       # sizing + full call
        _same(_range(ix, q[:nq], thr, max_results=total), want)    # one call, exact capacity
        _same(_range(ix, q[:nq], thr, max_results=total + 100), want)
        assert ix.get_stat("last_range_emit_groups") == 3 and ix.get_stat("last_range_emit_skipped") == 0
        with pytest.raises(_native.NativeLibraryError, match=rf"max_results >= {total}\b"):
            ix.range_search(qd, td, max_results=total - 1)
        assert ix.get_stat("last_range_overflow") == 1
        with pytest.raises(_native.NativeLibraryError, match=rf"holds {total} rows, the outputs 0 "):
            ix.range_search(qd, td, max_results=0)
        # the native call on overflow: lims complete, positions below the capacity hold the right rows, nothing past them is written
        cap = total - 1
        lims.fill_(-1)
        scores = torch.full((total,), 123.0, device="cuda")
        ids = torch.full((total,), 123, dtype=torch.int64, device="cuda")
        assert call(lims, scores, ids, cap) != 0
        msg = lib.vodhip_last_error().decode()
        assert str(total) in msg and str(cap) in msg
        np.testing.assert_array_equal(lims.cpu().numpy(), want[0])
        np.testing.assert_array_equal(ids[:cap].cpu().numpy(), want[2][:cap])
        np.testing.assert_array_equal(_bits(scores[:cap].cpu().numpy()), _bits(want[1][:cap]))
        assert ids[cap].item() == 123 and scores[cap].item() == 123.0
        assert ix.get_stat("last_range_overflow") == 1 and ix.get_stat("last_range_selfcheck") == 0
        _same(_range(ix, q[:nq], thr), want)  # (reads both status words as 0 again)
        # thresholds above everything: every emit workgroup leaves before its K loop
        none = _range(ix, q[:nq], np.full(nq, 1e9, dtype=np.float32), max_results=5)
        assert none[0][-1] == 0 and ix.get_stat("last_range_emit_skipped") == ix.get_stat("last_range_emit_groups") == 3


# ---- 7. the node index -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards,capacity", [(1, 3000), (2, 3000), (3, 3000), (3, 12000)])
def test_node_index_equals_the_flat_index(n_shards, capacity):
    from vod_amd import _native
    from vod_amd.index import HipNodeIndex

    q, x, s = _int_case(1)  # scores in [-64, 64]: the middle shard's tie rows tie with rows of both neighbours
    nq = 129
    tie = 1000 + np.arange(nq, dtype=np.int64)  # owned by the middle one of 3 shards of 1000 rows
    thr = s[np.arange(nq), tie]
    assert ((s[:nq, :1000] == thr[:, None]).any(axis=1) & (s[:nq, 2000:] == thr[:, None]).any(axis=1)).all()
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    with _index(x, "float16") as ix:
        flat = {"tie": _range(ix, q[:nq], thr, tie), "strict": _range(ix, q[:nq], thr), "inclusive": _range(ix, q[:nq], thr, inclusive=True),
                "score": _range(ix, q[:nq], thr, tie, order="score")}
        ix.set_row_labels(labels)
        flat["subset"] = _range(ix, q[:nq], thr, tie, subset=sub)
    _same(flat["tie"], G.range_search(s[:nq], thr, tie))
    total = int(flat["tie"][0][-1])
    with HipNodeIndex(1, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        empty = nx.range_search(np.array(q[:nq]), thr)
        assert (empty.lims == 0).all() and empty.ids.shape == (0,)
        nx.add(x.astype(np.float32))
        got = {"tie": nx.range_search(np.array(q[:nq]), thr, tie_ids=tie), "strict": nx.range_search(np.array(q[:nq]), thr),
               "inclusive": nx.range_search(np.array(q[:nq]), thr, inclusive=True),
               "score": nx.range_search(np.array(q[:nq]), thr, tie_ids=tie, order="score")}
        sized = nx.range_search(np.array(q[:nq]), thr, tie_ids=tie, max_results=total)
        with pytest.raises(_native.NativeLibraryError, match=rf"max_results >= {total}\b"):
            nx.range_search(np.array(q[:nq]), thr, tie_ids=tie, max_results=total - 1)
        nx.set_row_labels(labels)
        got["subset"] = nx.range_search(np.array(q[:nq]), thr, tie_ids=tie, subset=sub)
    for name, res in got.items():
        assert isinstance(res.ids, np.ndarray) and res.lims.dtype == np.int64 and res.scores.dtype == np.float32 and res.ids.dtype == np.int64
        _same(tuple(res), flat[name])
    _same(tuple(sized), flat["tie"])


# ---- 8. outranking and posterior_support ---------------------------------------------------------------------------------------------------
def test_outranking_returns_the_rows_rank_ids_counts():
    q, x, s = _int_case(1)
    nq, n = 129, 1500
    tgt = (np.arange(nq, dtype=np.int64) * 37) % n
    tgt[5], tgt[6] = n + 3, -1  # absent targets
    with _index(x[:n], "float16") as ix:
        ranks = ix.rank_ids(_cuda(q[:nq]), _cuda(tgt[:, None])).rank[:, 0].cpu().numpy()
        res = ix.outranking(_cuda(q[:nq]), _cuda(tgt))
        lims, scores, ids = res.lims.cpu().numpy(), res.scores.cpu().numpy(), res.ids.cpu().numpy()
        np.testing.assert_array_equal(np.diff(lims), np.where(ranks < 0, 0, ranks))
        assert ranks[5] == ranks[6] == -1 and lims[6] == lims[5] and lims[7] == lims[6]
        assert ranks.max() > 1000  # deep targets: far past any search's k
        want_rank = R.ranks_by_argsort(s[:nq, :n])
        for j in (0, 1, 64, 128):  # in search order: exactly the rows with a smaller rank than the target, by rank
            ahead = np.argsort(want_rank[j])[:ranks[j]]
            np.testing.assert_array_equal(ids[lims[j]:lims[j + 1]], ahead)
            np.testing.assert_array_equal(_bits(scores[lims[j]:lims[j + 1]]), _bits(s[j, ahead]))
        by_id = ix.outranking(_cuda(q[:nq]), _cuda(tgt), order="id")
        assert torch.equal(by_id.lims, res.lims)
        np.testing.assert_array_equal(by_id.ids.cpu().numpy()[lims[0]:lims[1]], np.sort(ids[lims[0]:lims[1]]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_posterior_support_is_the_set_above_the_rounded_threshold(dtype):
    """The last comparison - logsumexp(log_p) against `topk_log_coverage` of a search of the same length - is the one inexact check.
    Both sides use the same score bits and the same (max_score, log_rel); they differ by the float32 evaluation of a sum of at most n
    terms on torch's side, which is what `partition_ref.device_bound` (without its dot-product part) bounds for log_rel."""
    from vod_amd.index import topk_log_coverage

    rng = np.random.default_rng(64)
    n, d, nq, T, eps = 3000, 64, 70, 8.0, 1e-3
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    with _index(x, dtype) as ix:
        qd = _cuda(q)
        s = _scan_scores(ix, qd, n)
        sup = ix.posterior_support(qd, eps, temperature=T)
        lp = sup.log_partition
        log_z = lp.max_score.double().cpu().numpy() / T + lp.log_rel.double().cpu().numpy()
        thr = (T * (log_z + np.log(eps))).astype(np.float32)
        got = (sup.lims.cpu().numpy(), sup.scores.cpu().numpy(), sup.ids.cpu().numpy())
        _same(got, G.range_search(s, thr))
        lens = np.diff(got[0])
        assert lens.min() >= 1 and lens.max() < 2048 and lens.sum() > 20 * nq
        log_p = sup.log_p.cpu().numpy().astype(np.float64)
        np.testing.assert_array_equal(sup.log_p.cpu().numpy(), (got[1].astype(np.float64) / T - np.repeat(log_z, lens)).astype(np.float32))
        assert (log_p > np.log(eps) - 1e-4).all()
        lse = np.array([np.log(np.exp(log_p[got[0][j]:got[0][j + 1]]).sum()) for j in range(nq)])
        assert (lse <= 0).all()
        ss, _ = ix.search(qd, int(lens.max()))
        ss = torch.where(torch.arange(ss.shape[1], device="cuda")[None, :] < _cuda(lens)[:, None], ss, torch.full_like(ss, -float("inf")))
        cov = topk_log_coverage(ss, lp, T).cpu().numpy().astype(np.float64)
        tol = P.device_bound(np.zeros((nq, 1)), None, None, 1 / T, n, dot=False)
        print(f"{dtype}: support sizes {lens.min()} .. {lens.max()}, coverage {lse.min():.4f} .. {lse.max():.4f}, "
              f"max |lse - topk_log_coverage| = {np.abs(lse - cov).max():.3e}, tol {tol.min():.3e}")
        assert (np.abs(lse - cov) <= tol).all()


# ---- 9. refusals and empty cases -----------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    q, x, s = _int_case(65)
    qd = _cuda(q[:5])
    thr = torch.zeros((5,), device="cuda")
    lims = torch.full((6,), 123, dtype=torch.int64, device="cuda")
    out_s = torch.full((50,), 123.0, device="cuda")
    out_i = torch.full((50,), 123, dtype=torch.int64, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(h, queries=qd, code=2, nq=5, t=thr, lab=None, n_lab=0, lm=lims, o_s=out_s, o_i=out_i, cap=50):
        return lib.vodhip_index_range_search(h, ptr(queries), code, nq, ptr(t), None, 0, ptr(lab), n_lab, ptr(lm), ptr(o_s), ptr(o_i), cap, None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x[:300], "float16") as ix:
        refused(call(None), "index is NULL")
        refused(call(ix._h, queries=None), "invalid query pointer")
        refused(call(ix._h, nq=-1), "invalid query pointer")
        refused(call(ix._h, code=3), "invalid q_dtype 3")
        refused(call(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(call(ix._h, lab=lab, n_lab=2), "set the row labels first")
        refused(call(ix._h, t=None), "thresholds is NULL")
        refused(call(ix._h, lm=None), "lims is NULL")
        refused(call(ix._h, o_s=None), "out_scores and out_ids must both be given")
        refused(call(ix._h, o_i=None), "out_scores and out_ids must both be given")
        refused(call(ix._h, cap=-1), "capacity=-1")
        torch.cuda.synchronize()
        assert (lims == 123).all() and (out_s == 123.0).all() and (out_i == 123).all()  # a refused call writes nothing
        with pytest.raises(ValueError, match="thresholds of shape"):
            ix.range_search(qd, thr[:4])
        with pytest.raises(ValueError, match="order must be"):
            ix.range_search(qd, thr, order="rank")
        with pytest.raises(ValueError, match="max_results"):
            ix.range_search(qd, thr, max_results=-1)
        with pytest.raises(ValueError, match="min_prob"):
            ix.posterior_support(qd, 0.0)
        # nq == 0: lims is [0]
        assert call(ix._h, queries=None, nq=0, t=None) == 0
        torch.cuda.synchronize()
        assert lims[0].item() == 0 and (lims[1:] == 123).all()
        empty = ix.range_search(torch.zeros((0, 65), device="cuda"), torch.zeros((0,), device="cuda"))
        assert empty.lims.tolist() == [0] and empty.ids.shape == (0,) and empty.scores.shape == (0,)
        _same(_range(ix, q[:5], np.zeros(5)), G.range_search(s[:5, :300], np.zeros(5)))  # after all that the call works
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="range_search is not supported on an L2 index"):
            ix.range_search(qd, thr)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="range_search is not supported on a VODHIP_EXACT_F32 store"):
            ix.range_search(qd, thr)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty store
        for kw in ({}, {"max_results": 4}, {"inclusive": True}):
            got = _range(ix, q[:5], np.full(5, -INF), **kw)
            assert got[0].tolist() == [0] * 6 and got[2].shape == (0,)
        assert ix.outranking(qd, torch.zeros((5,), dtype=torch.int64, device="cuda")).lims.tolist() == [0] * 6
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.range_search(np.array(q[:5]), np.zeros(5, dtype=np.float32))
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        nx.add(x[:600].astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.range_search(np.array(q[:5]), np.zeros(5, dtype=np.float32), subset=np.zeros((5, 2), dtype=np.int32))
        got = nx.range_search(np.zeros((0, 65), dtype=np.float32), np.zeros((0,), dtype=np.float32))
        assert got.lims.tolist() == [0] and got.ids.shape == (0,)
        _same(tuple(nx.range_search(np.array(q[:5]), np.zeros(5, dtype=np.float32))), G.range_search(s[:5, :600], np.zeros(5)))
        out = nx.outranking(np.array(q[:5]), np.arange(5, dtype=np.int64))
        np.testing.assert_array_equal(np.diff(out.lims), R.rank_ids(s[:5, :600], np.arange(5)[:, None])[0][:, 0])
        sup = nx.posterior_support(np.array(q[:5]), 1e-3, temperature=64.0)
        assert sup.log_p.shape == sup.ids.shape and (sup.log_p > np.log(1e-3) - 1e-4).all()
