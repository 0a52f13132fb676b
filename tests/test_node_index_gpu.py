"""GPU parity tests of the one-process, several-device index (`vodhip_node_index_*`: H1 + H2 + H3 behind one handle).

On the 1-GPU box the shards all live on device 0 (`devices=[0, 0, 0]`): row ranges, id offsets, the peer-copy / merge path
and the host / device entry modes are exercised exactly as with distinct devices.  Bar: identical to one index holding all the
rows = the oracle, ids and scores bit-exact on the integer-valued data (ties everywhere)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _int_data(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(nq, d)).astype(np.float16), rng.integers(-8, 9, size=(n, d)).astype(np.float16)


def _oracle(q, x, k):
    from oracle.flat_ip import flat_ip_topk

    return flat_ip_topk(q, x, k)


@pytest.mark.parametrize("n_shards", [1, 2, 3, 8])
@pytest.mark.parametrize("location", ["host", "device"])
def test_matches_one_index_over_all_rows(n_shards, location):
    from vod_amd.index import HipNodeIndex

    q, x = _int_data(5, 50_000, 128, 70)
    k = 100
    with HipNodeIndex(128, len(x), [0] * n_shards) as nx:
        # three appends that straddle shard boundaries (float16 and float32 sources)
        nx.add(x[:7_001])
        nx.add(x[7_001:33_333].astype(np.float32))
        nx.add(x[33_333:])
        assert nx.ntotal == len(x)
        rs, ri = _oracle(q, x, k)
        for _ in range(3):  # buffers are reused; back-to-back calls must not race
            if location == "host":
                s, i = nx.search(q, k)
            else:
                s, i = nx.search(torch.from_numpy(q).cuda(), k)
                s, i = s.cpu().numpy(), i.cpu().numpy()
            np.testing.assert_array_equal(i, ri)
            np.testing.assert_array_equal(s, rs)


def test_partly_filled_store_empty_shards_and_k_larger_than_the_store():
    from vod_amd.index import HipNodeIndex

    q, x = _int_data(6, 900, 64, 9)
    with HipNodeIndex(64, 40_000, [0, 0, 0, 0]) as nx:  # 10,000 rows per shard: only shard 0 holds rows
        nx.add(x)
        s, i = nx.search(q, 1000)
        rs, ri = _oracle(q, x, 1000)
        np.testing.assert_array_equal(i, ri)  # 900 hits, then -1 pads
        np.testing.assert_array_equal(s, rs)
        assert (i[:, 900:] == -1).all() and np.isneginf(s[:, 900:]).all()
        nx.reset()
        assert nx.ntotal == 0
        s, i = nx.search(q, 5)
        assert (i == -1).all() and np.isneginf(s).all()


def test_gaussian_rows_recall_and_score_tolerance_with_a_recovery_pass_on_one_shard():
    """A tiny candidate capacity on ONE shard forces its recovery pass; the merged answer is still exact."""
    from vod_amd import _native
    from vod_amd.index import HipNodeIndex

    rng = np.random.default_rng(7)
    x = rng.standard_normal((300_000, 64)).astype(np.float16)
    x[150_000:] = x[150_000:] * np.linspace(1.0, 3.0, 150_000, dtype=np.float16)[:, None]  # norms grow along shard 1: its thresholds lag
    q = rng.standard_normal((200, 64)).astype(np.float16)
    k = 50
    with HipNodeIndex(64, len(x), [0, 0]) as nx:
        nx.add(x)
        h, base, dev = nx.shard(1)
        assert base == 150_000 and dev == 0
        lib = _native.load_library()
        _native.check(lib.vodhip_index_set_param(ctypes.c_void_p(h), b"cand_cap", 256))
        s, i = nx.search(q, k)
        ref = q.astype(np.float64) @ x.astype(np.float64).T
        top = np.argsort(-ref, axis=1, kind="stable")[:, :k]
        kth = np.take_along_axis(ref, top[:, -1:], axis=1)
        got = np.take_along_axis(ref, i, axis=1)
        assert (got >= kth - 1e-3 * np.abs(kth)).all()  # recall 1.0 up to near-ties
        np.testing.assert_allclose(s, got, rtol=1e-3, atol=1e-3)
        assert all(len(set(r)) == k for r in i)


def test_errors_are_reported_not_thrown_across_the_boundary():
    from vod_amd import _native
    from vod_amd.index import HipNodeIndex

    with HipNodeIndex(32, 100, [0, 0]) as nx:
        with pytest.raises(_native.NativeLibraryError, match="index full"):
            nx.add(np.zeros((101, 32), np.float32))
        with pytest.raises(_native.NativeLibraryError, match="out of range"):
            nx.search(np.zeros((1, 32), np.float32), 5000)
        with pytest.raises(_native.NativeLibraryError, match="shard 7 out of range"):
            nx.shard(7)
    with pytest.raises(_native.NativeLibraryError):
        HipNodeIndex(32, 100, [99])  # no such device
    # a reported failure must not linger in the HIP runtime's sticky error and fail the NEXT launch check
    from vod_amd.gradients import RetrievalGradients

    q = torch.randn(4, 16, device="cuda", requires_grad=True)
    s = torch.randn(4, 3, 16, device="cuda")
    batch = {"section__score": torch.zeros(4, 3, device="cuda"), "section__relevance": torch.ones(4, 3, dtype=torch.int64, device="cuda")}
    assert torch.isfinite(RetrievalGradients()(batch=batch, query_encoding=q, section_encoding=s).loss)


def test_subset_labels_travel_to_every_shard():
    """Row labels split by shard, per-query allowed labels replicated with the queries: exact top-k over the eligible rows."""
    from vod_amd.index import HipNodeIndex

    q, x = _int_data(8, 30_000, 64, 12)
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 7, size=len(x)).astype(np.int32)
    subset = np.full((len(q), 3), -1, dtype=np.int32)
    for r in range(len(q)):
        picks = rng.choice(7, size=rng.integers(0, 4), replace=False)  # 0 picks = unrestricted
        subset[r, : len(picks)] = picks
    subset[3] = [-2, -1, -1]  # an unknown label: restricted and empty
    k = 20
    with HipNodeIndex(64, len(x), [0, 0, 0]) as nx:
        nx.add(x)
        nx.set_row_labels(labels)
        s, i = nx.search(q, k, subset=subset)
        ref = q.astype(np.float64) @ x.astype(np.float64).T
        for r in range(len(q)):
            allowed = subset[r][subset[r] != -1]
            ok = np.ones(len(x), bool) if len(allowed) == 0 else np.isin(labels, allowed)
            sc = np.where(ok, ref[r], -np.inf)
            order = np.lexsort((np.arange(len(x)), -sc))[:k]
            n_ok = int(min(k, ok.sum()))
            np.testing.assert_array_equal(i[r, :n_ok], order[:n_ok])
            np.testing.assert_array_equal(s[r, :n_ok], sc[order[:n_ok]].astype(np.float32))
            assert (i[r, n_ok:] == -1).all()
        s2, i2 = nx.search(q, k)  # cleared again: unrestricted
        rs, ri = _oracle(q, x, k)
        np.testing.assert_array_equal(i2, ri)


@pytest.mark.parametrize("location", ["host", "device"])
def test_no_peer_access_route_staged_through_pinned_host_memory(location):
    """Round-3 verdict: the node index's peer copies had never crossed a device boundary and had no alternative.  At create the
    library now reads the topology (`hipDeviceCanAccessPeer` both ways); a shard that cannot exchange with devices[0] directly sends its
    queries / subset labels / top-k list through pinned host memory.  `host_staging` forces that route for every shard but the first,
    so it runs on a 1-GPU box: results must equal the oracle, subset filter included, back to back."""
    from oracle.flat_ip import topk_desc_tiebreak
    from vod_amd.index import HipNodeIndex

    q, x = _int_data(15, 60_000, 64, 90)
    k = 64
    labels = (np.arange(len(x)) % 5).astype(np.int32)
    with HipNodeIndex(64, len(x), [0, 0, 0]) as nx:
        nx.add(x)
        assert nx.peer_access() == [2, 2, 2]          # every shard on devices[0] itself: no exchange over a link at all
        nx.set_param("host_staging", 1)
        assert nx.peer_access() == [2, 0, 0]
        rs, ri = _oracle(q, x, k)
        for _ in range(3):
            if location == "host":
                s, i = nx.search(q, k)
            else:
                s, i = nx.search(torch.from_numpy(q).cuda(), k)
                s, i = s.cpu().numpy(), i.cpu().numpy()
            np.testing.assert_array_equal(i, ri)
            np.testing.assert_array_equal(s, rs)
        # the subset labels travel the same way
        nx.set_row_labels(labels)
        sub = np.full((len(q), 2), -1, dtype=np.int32)
        sub[::2] = [1, 3]
        full = q.astype(np.float64) @ x.astype(np.float64).T
        for r in range(0, len(q), 2):
            full[r, ~np.isin(labels, [1, 3])] = np.nan
        ms, mi = topk_desc_tiebreak(full, k)
        s, i = nx.search(q, k, subset=sub)
        np.testing.assert_array_equal(i, mi)
        np.testing.assert_array_equal(s, ms)


def test_row_labels_set_on_a_non_blocking_stream_survive_the_initial_fill():
    """Found by the round-4 campaign (fuzz_search seed 404, trial 1051): the FIRST `set_row_labels` of an index allocated the label array,
    filled it with -1 on the NULL stream and copied the labels on the caller's stream - the node index's shard streams are non-blocking, so
    the fill could land after the copy and every restricted query came back empty.  Run in a fresh process (the race needs the first,
    slow, memset of a process) several times: every restricted row must match the masked oracle."""
    import subprocess
    import sys

    from conftest import ROOT

    code = f"""
import sys
import numpy as np
sys.path.insert(0, {str(ROOT)!r})
from oracle.flat_ip import topk_desc_tiebreak
from vod_amd.index import HipNodeIndex
rng = np.random.default_rng(3)
n, d, nq, k = 9000, 65, 300, 128
x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
labels = rng.integers(0, 6, size=n).astype(np.int32)
sub = np.full((nq, 2), -1, dtype=np.int32)
sub[::2] = [5, 2]
nx = HipNodeIndex(d, n, [0])
nx.add(x)
nx.set_row_labels(labels)
s, i = nx.search(q, k, subset=sub)
full = q.astype(np.float64) @ x.astype(np.float64).T
for r in range(0, nq, 2):
    full[r, ~np.isin(labels, [5, 2])] = np.nan
rs, ri = topk_desc_tiebreak(full, k)
assert np.array_equal(i, ri) and np.array_equal(s, rs), int((i != ri).any(axis=1).sum())
print("ok")
"""
    for _ in range(3):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-1500:] + out.stdout[-300:]


@pytest.mark.parametrize("location", ["host", "device"])
@pytest.mark.parametrize("staging", [0, 1])
def test_two_searches_in_flight_return_what_the_synchronous_search_returns(location, staging):
    """Round 6: `search_async` / `finish` - the host enqueues batch i + 1 on every shard while batch i runs.  Different batches (and k, and a
    subset filter on one of them) in flight together, both entry modes, peer copies and the host-staged route: every result equals the oracle
    = what the synchronous search returns; the FIFO order is the enqueue order; a third search is refused until one is finished."""
    from vod_amd.index import HipNodeIndex

    rng = np.random.default_rng(11)
    x = rng.integers(-8, 9, size=(40_000, 96)).astype(np.float16)
    qs = [rng.integers(-8, 9, size=(nq, 96)).astype(np.float16) for nq in (70, 300, 5, 129)]
    ks = [100, 7, 33, 64]
    labels = (np.arange(len(x)) % 5).astype(np.int32)
    sub = np.full((300, 2), -1, dtype=np.int32)
    sub[::2, 0] = 3
    with HipNodeIndex(96, len(x), [0, 0, 0]) as nx:
        nx.add(x)
        nx.set_row_labels(labels)
        if staging:
            nx.set_param("host_staging", 1)
        want = []
        for j, (q, k) in enumerate(zip(qs, ks)):
            if j == 1:
                rows = [np.nonzero(labels == 3)[0] if r % 2 == 0 else np.arange(len(x)) for r in range(len(q))]
                rs = np.full((len(q), k), -np.inf, dtype=np.float32)
                ri = np.full((len(q), k), -1, dtype=np.int64)
                for r in range(len(q)):
                    a, b = _oracle(q[r : r + 1], x[rows[r]], k)
                    rs[r], ri[r] = a[0], rows[r][b[0]]
                want.append((rs, ri))
            else:
                want.append(_oracle(q, x, k))
        as_in = (lambda q: q) if location == "host" else (lambda q: torch.from_numpy(q).cuda())
        as_out = (lambda t: t) if location == "host" else (lambda t: t.cpu().numpy())
        for _ in range(2):  # slots are reused
            nx.search_async(as_in(qs[0]), ks[0])
            nx.search_async(as_in(qs[1]), ks[1], subset=sub)
            with pytest.raises(Exception, match="in flight"):
                nx.search_async(as_in(qs[2]), ks[2])
            with pytest.raises(Exception, match="pending|in flight"):
                nx.search(as_in(qs[2]), ks[2])
            with pytest.raises(Exception, match="in flight"):
                nx.add(x[:1])
            for j in (0, 1):
                s, i = nx.finish()
                np.testing.assert_array_equal(as_out(i), want[j][1])
                np.testing.assert_array_equal(as_out(s), want[j][0])
                if j == 0:  # one ahead: the next batch goes in before the older one of the pair is finished
                    nx.search_async(as_in(qs[2 + (_ % 2)]), ks[2 + (_ % 2)])
            s, i = nx.finish()
            np.testing.assert_array_equal(as_out(i), want[2 + (_ % 2)][1])
            np.testing.assert_array_equal(as_out(s), want[2 + (_ % 2)][0])
            with pytest.raises(Exception, match="no search is pending"):
                nx.finish()
        s, i = nx.search(as_in(qs[3]), ks[3])  # the synchronous call still works afterwards
        np.testing.assert_array_equal(as_out(i), want[3][1])


def _arrays(result):
    """Every array of a (nested) result tuple, in order."""
    if isinstance(result, tuple):
        return [a for part in result for a in _arrays(part)]
    return [np.asarray(result)]


def _assert_same_bits(got, want):
    got, want = _arrays(got), _arrays(want)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.dtype in (np.float32, np.int64)
        view = np.uint32 if a.dtype == np.float32 else np.int64
        np.testing.assert_array_equal(a.view(view), b.view(view))


def test_a_shard_that_refuses_mid_fan_out_leaves_the_handle_usable():
    """Every operation that replicates host inputs to the shards, when shard 1's flat call refuses (its row labels were cleared behind
    the node index's back) after shard 0 was enqueued: the error names the shard, what shard 0 had in flight is freed and waited for,
    and once the labels are back every operation returns the bits it returned before."""
    from vod_amd import _native
    from vod_amd.index import HipNodeIndex

    rng = np.random.default_rng(21)
    n, d, nq = 600, 65, 3
    x = rng.standard_normal((n, d)).astype(np.float16)
    q = rng.standard_normal((nq, d)).astype(np.float16)
    qb = rng.standard_normal((nq, d)).astype(np.float16)
    labels = (np.arange(n) % 2).astype(np.int32)
    subset = np.array([[r % 2] for r in range(nq)], dtype=np.int32)
    ids = np.array([[r, 199, 200 + 7 * r, 401, 599 - r] for r in range(nq)], dtype=np.int64)  # all three shards, both labels
    weights = rng.standard_normal(ids.shape).astype(np.float32)
    thresholds = rng.standard_normal(ids.shape).astype(np.float32)
    with HipNodeIndex(d, n, [0, 0, 0]) as nx:
        nx.add(x)
        nx.set_row_labels(labels)
        ops = {
            "score_ids": lambda: nx.score_ids(q, ids, subset=subset),
            "score_ids_k2": lambda: nx.score_ids(q, ids, 2, subset=subset),
            "sum_ids": lambda: nx.sum_ids(ids, weights, subset=subset),
            "log_partition": lambda: nx.log_partition(q, subset=subset),
            "posterior_stats": lambda: nx.posterior_stats(q, subset=subset),
            "posterior_divergence": lambda: nx.posterior_divergence(q, qb, subset=subset),
            "posterior_mean": lambda: nx.posterior_mean(q, subset=subset),
            "sample_posterior": lambda: nx.sample_posterior(q, 4, seed=7, subset=subset),
            "rank_ids": lambda: nx.rank_ids(q, ids, subset=subset),
            "count_above": lambda: nx.count_above(q, thresholds, tie_ids=ids, subset=subset),
        }
        before = {name: op() for name, op in ops.items()}
        lib = _native.load_library()
        _native.check(lib.vodhip_index_set_row_labels(ctypes.c_void_p(nx.shard(1)[0]), None, 0, 0, None))
        for name, op in ops.items():
            with pytest.raises(_native.NativeLibraryError, match=r"shard 1: set the row labels first \(vodhip_index_set_row_labels\)"):
                op()
        nx.set_row_labels(labels)
        for name, op in ops.items():
            _assert_same_bits(op(), before[name])
