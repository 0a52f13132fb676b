"""`HipFlatIndex(metric="l2")` on the GPU against the float64 restatement (tests/l2_ref.py).

Bit-exact cases: integers in [-8, 8] (fp16 and bf16 hold them exactly), so that |x|^2 / 2 is a half-integer the bias split carries
exactly, every partial sum of the dim + 3 products is exact in float32 and every distance is an exact integer with many ties: scores and
ids must equal the restatement bit for bit.  The shapes of the existing exactness fixtures; stores of 1500 rows (the dense path) and
3000 rows (FILTER stages) at widths 1, 61, 62 (the bias columns stay within / cross the 64-column tile), 64, 65, 125, 127, 128, 765,
768 and batches of 1, 64, 65, 128, 129, 300 queries (both small-batch rings, the 128 x 128 tile, the 8-phase kernel); every filter
kernel forced on one shape.  One reference per data set (300 queries, k = 100): a smaller batch is its first rows.

Lifecycle and contract: pads, an empty index, nq = 0, id_base, a query equal to a row, incremental / reset / device ingest giving the
same bits, stored_rows, save / load, subset labels, the overflow recovery (converted once, after the last pass), four searches in
flight on two lanes, a saturated row, the refusals.

Gaussian data, N(0, 1) at 3000 x 768 and 3000 x 765, nq 129, k 100: every returned distance is within `l2_ref.device_bound` of the
float64 distance of its (query, id) pair - the any-order float32 bound of the three sums involved, derived in DESIGN.md 4, not measured -
and the ids equal the restatement's except where the float64 distance of the returned row is within that bound of the slot's; fewer than
1 % of the slots may use that exception (tests/test_l2_cpu.py shows the seeds allow it).  A query equal to a Gaussian row: its
distance is 2 (n2 - n2') for two float32 sums of the same squares in different orders - clamped at 0, within the bound, not exactly 0;
on integer rows it is exactly 0.
"""
import functools

import numpy as np
import pytest

import l2_ref as R
from test_l2_cpu import GAUSS_CASES, gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
K = 100


def _index(x, dtype="float16", capacity=None, dim=None, **params):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, metric="l2")
    for key, v in params.items():
        ix.set_param(key, v)
    if len(x):
        ix.add(x)
    return ix


@functools.lru_cache(maxsize=None)
def _int_case(seed, n, d, nq, k=K):
    """integer rows / queries and their restatement; the same for both store dtypes (both hold the values exactly)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    assert np.array_equal(R.round_store(x, R.BF16), x) and np.array_equal(R.round_store(x, R.F16), x)
    dist = R.distances(q, x, R.F16)
    rd, ri = R.topk_from(dist, k)
    for a in (q, x, rd, ri):
        a.setflags(write=False)
    return q, x, rd, ri


def _search(ix, q, k, **kw):
    s, i = ix.search(torch.from_numpy(np.array(q)).cuda(), k, **kw)  # (a copy: the cached cases are read-only)
    return s.cpu().numpy(), i.cpu().numpy()


def _assert_bits(got, rd, ri):
    s, i = got
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rd.astype(np.float32))
    assert s.dtype == np.float32 and np.array_equal(rd.astype(np.float32).astype(np.float64), rd)  # the reference itself is exact


# ---- bit-exact cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,nq,k", [(4096, 64, 16, 10), (20000, 768, 64, 100)])
def test_exactness_fixture_shapes(n, d, nq, k, dtype):
    q, x, rd, ri = _int_case(1, n, d, nq, k)
    with _index(x, dtype) as ix:
        assert ix.get_stat("l2") == 1 and ix.get_stat("dim_pad") == (d + 3 + 63) // 64 * 64
        _assert_bits(_search(ix, q, k), rd, ri)
        assert ix.get_stat("last_overflow") == 0 and ix.get_stat("l2_saturated_rows") == 0


WIDTHS = [1, 61, 62, 64, 65, 125, 127, 128, 765, 768]
BATCHES = [1, 64, 65, 128, 129, 300]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", [1500, 3000])
def test_widths_store_sizes_and_batch_sizes(n, d, dtype):
    q, x, rd, ri = _int_case(100 + d, n, d, 300)
    with _index(x, dtype) as ix:
        for nq in BATCHES:
            _assert_bits(_search(ix, q[:nq], K), rd[:nq], ri[:nq])
        _assert_bits(_search(ix, q[:65], 7), rd[:65, :7], ri[:65, :7])  # the order is total: a smaller k is a prefix


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", [1, 8, 14, 42, 46])
def test_every_filter_kernel(tile, dtype):
    q, x, rd, ri = _int_case(100 + 765, 3000, 765, 300)
    with _index(x, dtype, tile=tile) as ix:
        for nq in (129, 300):
            _assert_bits(_search(ix, q[:nq], K), rd[:nq], ri[:nq])


# ---- lifecycle and contract -------------------------------------------------------------------------------------------------------
def test_pads_empty_index_no_queries_and_id_base():
    q, x, rd, ri = _int_case(7, 3000, 65, 300)
    with _index(x[:5], capacity=8) as ix:  # k > ntotal
        s, i = _search(ix, q[:3], 10)
        rd5, ri5 = R.l2_topk(q[:3], x[:5], 10, R.F16)
        np.testing.assert_array_equal(i, ri5)
        np.testing.assert_array_equal(s, rd5.astype(np.float32))
        assert np.isposinf(s[:, 5:]).all() and (i[:, 5:] == -1).all()
        s, i = _search(ix, q[:3], 10, id_base=1 << 40)
        assert (i[:, :5] == ri5[:, :5] + (1 << 40)).all() and (i[:, 5:] == -1).all() and np.isposinf(s[:, 5:]).all()
    with _index(x[:0], capacity=8, dim=65) as ix:  # empty index
        s, i = _search(ix, q[:3], 4)
        assert np.isposinf(s).all() and (i == -1).all()
        s, i = _search(ix, q[:0], 4)
        assert s.shape == (0, 4) and i.shape == (0, 4)
    with _index(x) as ix:
        s, i = _search(ix, q[:0], 4)  # nq = 0 on a filled index
        assert s.shape == (0, 4)
        s, i = _search(ix, q[:70], K, id_base=12345)
        np.testing.assert_array_equal(i, ri[:70] + 12345)
        np.testing.assert_array_equal(s, rd[:70].astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_query_equal_to_a_stored_row(dtype):
    q, x, _, _ = _int_case(7, 3000, 65, 300)
    rows = np.array([0, 17, 1499, 2999])
    with _index(x, dtype) as ix:
        s, i = _search(ix, x[rows], 5)
    assert (s[:, 0] == 0.0).all() and not np.signbit(s).any()  # exactly 0 on integer rows
    rd, ri = R.l2_topk(x[rows], x, 5, dtype)
    np.testing.assert_array_equal(i, ri)  # (the smallest id among the copies of the row comes first)
    gq, gx = gauss_case(765, 3, n=3000, nq=1)
    with _index(gx, dtype) as ix:
        s, i = _search(ix, gx[rows], 5)
    d64 = R.distances(gx[rows], gx, dtype)
    assert (i[:, 0] == rows).all() and (s >= 0).all() and not np.signbit(s).any()
    assert (s[:, 0] <= R.device_bound(gx[rows], gx, dtype, d64)[np.arange(4), rows]).all()


def test_ingest_in_parts_after_reset_and_from_the_device_gives_the_same_bits():
    gq, gx = gauss_case(65, 21, n=3000, nq=70)

    def bits(ix):
        s, i = _search(ix, gq, K)
        data = ix.stored_rows().cpu().numpy()
        return s, i, data

    with _index(gx) as ix:
        one = bits(ix)
    assert one[2].shape == (3000, 65)
    np.testing.assert_array_equal(one[2], gx.astype(np.float16))  # stored_rows: [n, dim], the rounded input
    builds = []
    with _index(gx[:0], capacity=3000, dim=65) as ix:
        for lo, hi in ((0, 1), (1, 1301), (1301, 3000)):  # three calls, host rows
            ix.add(gx[lo:hi])
        builds.append(bits(ix))
        ix.reset()  # reset + re-add, other rows first so that stale bias columns would show
        ix.add(gx[::-1].copy())
        ix.reset()
        ix.add(torch.from_numpy(gx).cuda())  # one call, device rows
        builds.append(bits(ix))
        ix.reset()
        for lo, hi in ((0, 257), (257, 258), (258, 3000)):  # three calls, device rows (float16 and float32 sources)
            part = torch.from_numpy(gx[lo:hi]).cuda()
            ix.add(part.half() if lo == 0 else part)
        builds.append(bits(ix))
    for b in builds:
        for got, want in zip(b, one):
            np.testing.assert_array_equal(got, want)


def test_save_and_load(tmp_path):
    from vod_amd.index import HipFlatIndex

    gq, gx = gauss_case(61, 22, n=3000, nq=70)
    for dtype in DTYPES:
        with _index(gx, dtype) as ix:
            want = _search(ix, gq, K)
            ix.save(tmp_path / f"{dtype}.npy")
        saved = np.load(tmp_path / f"{dtype}.npy")
        assert saved.shape == (3000, 61)  # the user's columns only
        with HipFlatIndex.load(tmp_path / f"{dtype}.npy", dtype=TDT[dtype], metric="l2") as ix:
            assert ix.metric == "l2" and ix.get_stat("l2") == 1
            got = _search(ix, gq, K)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])


def test_subset_labels_restrict_l2_results():
    q, x, _, _ = _int_case(7, 3000, 65, 300)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 6, size=3000).astype(np.int32)
    subset = rng.integers(0, 6, size=(130, 2)).astype(np.int32)
    subset[5] = -1        # unrestricted
    subset[6] = (-1, 3)   # one label
    subset[7] = (-2, -1)  # an unknown label: no row is eligible
    elig = (labels[None, :, None] == subset[:, None, :]).any(-1) | (subset == -1).all(1)[:, None]
    rd, ri = R.l2_topk(q[:130], x, K, R.F16, eligible=elig)
    assert (ri[7] == -1).all() and (ri[5] >= 0).all()
    with _index(x) as ix:
        ix.set_row_labels(labels)
        _assert_bits(_search(ix, q[:130], K, subset=subset), rd, ri)
        full = _search(ix, q[:130], K)  # and the filter is gone with the next unrestricted search
    _, _, frd, fri = _int_case(7, 3000, 65, 300)
    _assert_bits(full, frd[:130], fri[:130])


def test_overflow_recovery_converts_once_after_the_last_pass():
    """`duplicates`-style rows (tests/fuzz/fuzz_search.py: each of n / 50 base rows ~50 times) against 256-slot candidate lists: a list
    overflows, recovery passes seed their thresholds from the similarity-form scores of the incomplete result and rewrite them; the
    distances are converted from that buffer again.  Seeding from the distances, or converting twice, breaks the bits below.  Whether a
    list overflows depends on the stage sizes the planner picks: like tests/test_fuzz_gpu.py, the first store that overflows is used."""
    rng = np.random.default_rng(31)
    d, nq = 64, 300
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    for n in (70000, 200000):
        base = rng.integers(-8, 9, size=(n // 50, d)).astype(np.float32)
        pick = rng.integers(0, len(base), size=n)
        x = base[pick]
        with _index(x, cand_cap=256) as ix:
            got = _search(ix, q, K)
            overflow, reruns = ix.get_stat("last_overflow"), ix.get_stat("last_safe_reruns")
        if overflow:
            break
    assert overflow == 1 and reruns >= 1
    db = R.distances(q, base, R.F16)  # (a copy has its base row's distance)
    per_query = [R.topk_from(db[a : a + 1][:, pick], K) for a in range(nq)]
    rd, ri = np.concatenate([p[0] for p in per_query]), np.concatenate([p[1] for p in per_query])
    _assert_bits(got, rd, ri)


def test_four_searches_in_flight_on_two_lanes():
    q, x, rd, ri = _int_case(7, 3000, 65, 300)
    with _index(x, lanes=2) as ix:
        batches = [torch.from_numpy(np.array(q[b * 64 : b * 64 + 60 + b])).cuda() for b in range(4)]
        sync = [tuple(t.cpu().numpy() for t in ix.search(b, K)) for b in batches]
        outs = [(torch.empty((len(b), K), dtype=torch.float32, device="cuda"), torch.empty((len(b), K), dtype=torch.int64, device="cuda"))
                for b in batches]
        for b, o in zip(batches, outs):
            ix.search_async(b, K, out=o)
        with pytest.raises(Exception, match="in flight"):
            ix.search_async(batches[0], K)
        for _ in batches:
            ix.finish()
        for b, (s, i) in enumerate(outs):
            np.testing.assert_array_equal(s.cpu().numpy(), sync[b][0])
            np.testing.assert_array_equal(i.cpu().numpy(), sync[b][1])
            _assert_bits(sync[b], rd[b * 64 : b * 64 + 60 + b], ri[b * 64 : b * 64 + 60 + b])


def test_a_row_beyond_the_limit_saturates_ranks_last_and_is_counted():
    rng = np.random.default_rng(4)
    x = rng.integers(-8, 9, size=(300, 64)).astype(np.float32)
    x[3] = 65504.0       # |x|^2 = 2.7e11: beyond the fp16 split's limit (just under 2^25)
    x[200, :8] = 1000.0  # |x|^2 just above 8e6, below 2^23: inside it, and every sum involved is still exact in float32
    q = rng.integers(-8, 9, size=(4, 64)).astype(np.float32)
    with _index(x) as ix:
        assert ix.get_stat("l2_saturated_rows") == 1
        s, i = _search(ix, q, 300)
        assert (i[:, -1] == 3).all() and np.isfinite(s).all() and (np.diff(s, axis=1) >= 0).all()
        rd, ri = R.l2_topk(q, np.delete(x, 3, axis=0), 299, R.F16)
        np.testing.assert_array_equal(i[:, :299], ri + (ri >= 3))  # the rows within the limit: exact, the large one included
        np.testing.assert_array_equal(s[:, :299], rd.astype(np.float32))
        ix.reset()
        assert ix.get_stat("l2_saturated_rows") == 0


# ---- Gaussian data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_distances_within_the_derived_bound(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    d64 = R.distances(q, x, dtype)
    bound = R.device_bound(q, x, dtype, d64)
    rd, ri = R.topk_from(d64, K)
    with _index(x, dtype) as ix:
        s, i = _search(ix, q, K)
    assert (i >= 0).all() and (np.diff(s, axis=1) >= 0).all() and (s >= 0).all()
    assert all(len(set(row)) == K for row in i)
    rows = np.arange(len(q))[:, None]
    err = np.abs(s.astype(np.float64) - d64[rows, i])
    slack = bound[rows, i]
    differs = i != ri
    off = np.abs(d64[rows, i] - rd)  # float64 distance of the returned row against the slot's
    print(f"dim {dim} {dtype}: max |d - d64| {err.max():.3e} (bound there {slack.flat[err.argmax()]:.3e}, smallest bound {slack.min():.3e}); "
          f"{100 * differs.mean():.3f} % of the slots differ, largest float64 gap at one {off[differs].max() if differs.any() else 0.0:.3e}")
    assert (err <= slack).all()
    assert (off[differs] < slack[differs]).all()
    assert differs.mean() < 0.01


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_inner_product_stat():
    from vod_amd._native import NativeLibraryError
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    with pytest.raises(NativeLibraryError, match=r"VODHIP_L2 \| VODHIP_EXACT_F32 is not supported"):
        HipFlatIndex(64, 10, device=0, exact_f32=True, metric="l2")
    with pytest.raises(NativeLibraryError, match="VODHIP_L2 is not supported by the node index"):
        HipNodeIndex(64, 10, [0], metric="l2")
    with pytest.raises(ValueError, match="metric must be one of"):
        HipFlatIndex(64, 10, device=0, metric="cosine")
    x = np.random.default_rng(0).integers(-8, 9, size=(300, 64)).astype(np.float32)
    ids = np.arange(6, dtype=np.int64).reshape(2, 3)
    with _index(x) as ix:
        for k in (None, 2):
            with pytest.raises(NativeLibraryError, match="listed ids are not supported on an L2 index"):
                ix.score_ids(x[:2], ids, k)
        s, i = _search(ix, x[:2], 3)  # and the index still searches
        assert (i[:, 0] == (0, 1)).all() and (s[:, 0] == 0).all()
    with HipFlatIndex(64, 300, device=0) as ip:
        ip.add(x)
        assert ip.get_stat("l2") == 0 and ip.get_stat("l2_saturated_rows") == 0 and ip.metric == "inner_product"
        assert ip.get_stat("dim_pad") == 64
        assert np.isfinite(ip.score_ids(x[:2], ids).cpu().numpy()).all()
