"""`score_ids`: scores of listed rows and the top-k over a list (include/vodhip.h H2i, kernels_listed.hip) against the float64 restatement
of tests/score_ids_ref.py.

Integer data in -8 .. 8 (every partial sum exact in fp32 up to dim 16384): the aligned scores, and the ids and scores of the top-k
form, equal the restatement bit for bit - across the load-pass edges of the kernel (dim_pad 64 .. 16384), list lengths around the
64-slot run of a wave and the three workgroup shapes of the launcher, batch sizes, and lists that hold every kind of absent slot.
Gaussian data: |aligned - float64| <= SCORE_TOL = 1e-3; a CPU simulation of the kernel's summation order on N(0, 1) fp16
data stays within 1.0e-5 / 2.6e-5 at dim 768 / 4096.  The top-k form must ORDER THE DEVICE'S OWN aligned scores: bitwise.
Measured on an MI355X (3000 rows, 9 x 385 slots): 1.04e-5 / 7.4e-6 (fp16 / bf16) at dim 768, 2.30e-5 / 2.35e-5 at dim 4096.
"""
import functools

import numpy as np
import pytest

import score_ids_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-3  # "scores within 1e-3 fp32"
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}


def _flat(x, dtype=torch.float16, capacity=None, exact=False):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(x.shape[1], capacity or max(len(x), 1), dtype=dtype, device=0, exact_f32=exact)
    ix.add(x)
    return ix


def _dev(a):
    """a device tensor of a (read-only) NumPy array"""
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def _int_data(seed, n, d, nq):
    """integers in -8 .. 8 (exact in fp16 and bf16); rows 10 .. 39 are one row: many equal scores"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    if n >= 40:
        x[10:40] = x[10]
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    x.setflags(write=False)
    q.setflags(write=False)
    return q, x


def _lists(seed, nq, m, ntotal, id_base=0):
    """[nq, m] ids that hold, where m leaves room: random rows, empty slots in between, the tied rows 10 .. 25, row 0 and row ntotal-1,
    id = ntotal, an id >= 2^32, an id below id_base, one id three times; query 1 (if any) lists only -1."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, ntotal, size=(nq, m)).astype(np.int64) + id_base
    ids[rng.random((nq, m)) < 0.1] = -1
    special = [id_base, id_base + ntotal - 1, id_base + ntotal, (1 << 32) + 5 + id_base, id_base - 1 if id_base else -7]
    special += [id_base + 3] * 3
    if ntotal >= 40:
        special += [id_base + r for r in range(25, 9, -1)]
    for i in range(nq):
        pos = rng.permutation(m)[: len(special)]
        ids[i, pos] = special[: len(pos)]
    if nq > 1:
        ids[1] = -1
    return ids


def _check_both_forms(ix, q, x, ids, ks, id_base=0, row_labels=None, q_labels=None, other=None):
    """the aligned form and the top-k form at every k of `ks` against the restatement, bit for bit; `other`: a second index that must
    return the same bits (the node index)"""
    ref = R.score_ids_aligned(q, x, ids, id_base, row_labels, q_labels)
    kw = {} if q_labels is None else {"subset": q_labels}
    flat_kw = dict(kw, id_base=id_base)
    got = ix.score_ids(_dev(q), _dev(ids), **flat_kw).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ids.shape
    np.testing.assert_array_equal(got.astype(np.float64), ref)
    if other is not None:
        np.testing.assert_array_equal(other.score_ids(q, ids, **kw), got)
    if ids.shape[1] > 8192:
        return
    for k in ks:
        rs, ri = R.score_ids_topk(ref, ids, k)
        s, i = ix.score_ids(_dev(q), _dev(ids), k, **flat_kw)
        np.testing.assert_array_equal(i.cpu().numpy(), ri)
        np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), rs)
        if other is not None:
            os_, oi = other.score_ids(q, ids, k, **kw)
            np.testing.assert_array_equal(oi, ri)
            np.testing.assert_array_equal(os_.astype(np.float64), rs)


# dim -> dim_pad: 1, 64 -> 64 (less than one load pass); 100 -> 128; 512 -> 512 (one pass), 520 -> 576 (one pass + tail); 768 (the
# workload); 1030 -> 1088 (two passes + tail); 16384 (the widest supported; 300 rows)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("dim", [1, 64, 100, 512, 520, 768, 1030, 16384])
def test_widths_bit_exact(dim, dtype):
    n = 300 if dim == 16384 else 2000
    q, x = _int_data(11, n, dim, 3)
    with _flat(x, DTYPES[dtype]) as ix:
        # k = 10 < distinct ids; k = 100 > m = 65: pads; id_base = 1000
        _check_both_forms(ix, q, x, _lists(dim, 3, 65, n, 1000), (10, 100), id_base=1000)


# around the 64-slot run (m = 63, 64, 65), the launcher's three workgroup shapes, the top-k form's limit, the aligned form beyond it
@pytest.mark.parametrize("m", [1, 63, 64, 65, 385, 1000, 8192, 10000])
def test_list_lengths_bit_exact(m):
    q, x = _int_data(12, 8192, 100, 3)
    with _flat(x) as ix:
        _check_both_forms(ix, q, x, _lists(m, 3, m, len(x)), (1, 50, 2048))


@pytest.mark.parametrize("nq", [1, 3, 64, 257])
def test_batch_sizes_bit_exact(nq):
    q, x = _int_data(13, 4000, 768, nq)
    with _flat(x, torch.bfloat16) as ix:
        _check_both_forms(ix, q, x, _lists(nq, nq, 385, len(x)), (128,))


def test_rows_left_behind_by_a_reset_are_absent():
    q, x = _int_data(14, 100, 64, 2)
    with _flat(x, capacity=100) as ix:
        ix.reset()
        ix.add(x[50:])  # 50 rows: slots 50 .. 99 of the store still hold the old rows
        ids = np.array([[70, 49, 0, 50], [99, 70, 70, 1]], dtype=np.int64)
        got = ix.score_ids(q, ids).cpu().numpy()
        assert np.isneginf(got[[0, 0, 1, 1, 1], [0, 3, 0, 1, 2]]).all()
        _check_both_forms(ix, q, x[50:], ids, (3,))


def test_every_row_listed_once_equals_search():
    q, x = _int_data(15, 8192, 64, 5)
    with _flat(x) as ix:
        ids = np.stack([np.random.default_rng(i).permutation(len(x)) for i in range(len(q))]).astype(np.int64)
        s, i = ix.score_ids(q, ids, 100)
        rs, ri = ix.search(q, 100)
        assert torch.equal(i, ri) and torch.equal(s, rs)


@functools.lru_cache(maxsize=None)
def _gauss(seed, n, d, nq):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(nq, d, generator=g).numpy(), torch.randn(n, d, generator=g).numpy()


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("dim", [768, 4096])
def test_gaussian_within_score_tol_and_topk_orders_the_aligned_bits(dim, dtype):
    q, x = _gauss(dim, 3000, dim, 9)
    dt = DTYPES[dtype]
    qr, xr = torch.from_numpy(q).to(dt).double().numpy(), torch.from_numpy(x).to(dt).double().numpy()
    ids = _lists(dim, len(q), 385, len(x))
    with _flat(x, dt) as ix:
        got = ix.score_ids(q, ids).cpu().numpy()
        ref = R.score_ids_aligned(qr, xr, ids)
        assert np.array_equal(np.isneginf(got), np.isneginf(ref))
        fin = np.isfinite(ref)
        err = np.abs(got[fin] - ref[fin]).max()
        print(f"dim {dim} {dtype}: max |aligned - float64| = {err:.3e}")
        assert err <= SCORE_TOL
        s, i = ix.score_ids(q, ids, 100)
        ds, di = R.score_ids_topk(got, ids, 100)  # the device's own scores, ordered by the restatement
        np.testing.assert_array_equal(i.cpu().numpy(), di)
        np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), ds.view(np.uint32))
        sn = s.cpu().numpy()
        assert (sn[:, :-1] >= sn[:, 1:]).all()  # (query 1 lists nothing: a row of -inf pads)


def test_bits_of_a_pair_do_not_depend_on_slot_batch_or_list_length():
    q, x = _gauss(21, 5000, 768, 257)
    rng = np.random.default_rng(21)
    with _flat(x) as ix:
        ids = rng.integers(0, len(x), size=(257, 1000)).astype(np.int64)
        big = ix.score_ids(q, ids).cpu().numpy()                      # 64 slots per workgroup
        perm = rng.permutation(1000)
        np.testing.assert_array_equal(ix.score_ids(q, ids[:, perm]).cpu().numpy().view(np.uint32), big[:, perm].view(np.uint32))
        mid = ix.score_ids(q[:64], ids[:64, :385]).cpu().numpy()        # 16 slots per workgroup
        np.testing.assert_array_equal(mid.view(np.uint32), big[:64, :385].view(np.uint32))
        for qi, slot in ((0, 0), (200, 999), (63, 384)):
            one = ix.score_ids(q[qi : qi + 1], ids[qi : qi + 1, slot : slot + 1]).cpu().numpy()  # nq = 1, m = 1
            assert one.view(np.uint32)[0, 0] == big.view(np.uint32)[qi, slot]


@pytest.mark.parametrize("store,qdt", [("float16", torch.float32), ("float16", torch.bfloat16), ("bfloat16", torch.float16),
                                       ("bfloat16", torch.float32), ("float16", torch.float16)])
def test_queries_are_rounded_to_the_store_dtype_saturating(store, qdt):
    """integer rows; queries = integers + a fraction the store dtype cannot hold, one float32 component of 1e5 (beyond fp16: it
    saturates to 65504, as the search's prepare kernel does) - all sums stay exact in fp32"""
    q0, x = _int_data(16, 1000, 100, 4)
    frac = np.full((4, 1), 2.0 ** -9, dtype=np.float32)
    frac[2] = 0  # (the query with the large component stays integral: its sums must stay below 2^24 units of the last place)
    q = torch.from_numpy(q0 + frac).to(qdt)  # n + 2^-9: exact in float32, rounds to n in bf16 and, from |n| = 4, in fp16 ...
    if qdt == torch.float32:
        q[2, 7] = 1e5
    dt = DTYPES[store]
    lim = 65504.0 if dt == torch.float16 else 3.3895313892515355e38
    qr = q.float().clamp(-lim, lim).to(dt).double().numpy()  # ... and whatever it rounds to is what the restatement scores
    ids = _lists(16, 4, 65, len(x))
    with _flat(x, dt) as ix:
        got = ix.score_ids(q.cuda(), ids).cpu().numpy()
        np.testing.assert_array_equal(got.astype(np.float64), R.score_ids_aligned(qr, x, ids))
        if qdt == torch.float32 and store == "float16":
            assert (qr[2, 7] == 65504.0) and np.abs(got[2][np.isfinite(got[2])]).max() > 65504.0


def test_exact_f32_store_returns_the_bits_of_search_and_so_does_the_node_index():
    from vod_amd.index import HipNodeIndex

    q, x = _gauss(31, 6000, 768, 17)
    with _flat(x, exact=True) as ix:
        s, i = ix.search(q, 50)
        got = ix.score_ids(q, i)
        assert torch.equal(got.view(torch.int32), s.view(torch.int32))
        ts, ti = ix.score_ids(q, i.flip(1), 50)
        assert torch.equal(ti, i) and torch.equal(ts.view(torch.int32), s.view(torch.int32))
        s, i = s.cpu().numpy(), i.cpu().numpy()
    with HipNodeIndex(768, len(x), [0, 0, 0], exact_f32=True) as nx:
        nx.set_param("host_staging", 1)
        nx.add(x)
        np.testing.assert_array_equal(nx.score_ids(q, i).view(np.uint32), s.view(np.uint32))
        ns, ni = nx.score_ids(q, i[:, ::-1], 50)
        np.testing.assert_array_equal(ni, i)
        np.testing.assert_array_equal(ns.view(np.uint32), s.view(np.uint32))


def test_subset_labels_are_an_argument():
    q, x = _int_data(17, 1000, 64, 4)
    row_labels = (np.arange(len(x)) % 5).astype(np.int32)
    q_labels = np.array([[1, -1, -1], [-1, -1, -1], [9, -2, -1], [0, 4, 2]], dtype=np.int32)  # one, unrestricted, foreign only, three
    ids = _lists(17, 4, 385, len(x))
    ids[1] = _lists(18, 1, 385, len(x))[0]
    with _flat(x) as ix:
        ix.set_row_labels(row_labels)
        _check_both_forms(ix, q, x, ids, (20, 385), row_labels=row_labels, q_labels=q_labels)
        got = ix.score_ids(q, ids, subset=q_labels).cpu().numpy()
        assert np.isneginf(got[2]).all() and np.isfinite(got[1]).sum() > 300
        _check_both_forms(ix, q, x, ids, (20,))  # the same lists, unrestricted: no label of an earlier call sticks


def test_a_nan_row_scores_nan_and_never_enters_the_topk():
    q, x = _int_data(19, 200, 64, 2)
    x = x.copy()
    x[5, 3] = np.nan
    ids = np.array([[4, 5, 6, 5], [5, -1, 5, 7]], dtype=np.int64)
    with _flat(x) as ix:
        got = ix.score_ids(q, ids).cpu().numpy()
        assert np.isnan(got[[0, 0, 1, 1], [1, 3, 0, 2]]).all() and np.isfinite(got[[0, 0, 1], [0, 2, 3]]).all()
        _check_both_forms(ix, q, x, ids, (4,))
        s, i = ix.score_ids(q, ids, 4)
        assert not (i == 5).any().item() and not torch.isnan(s).any().item()


@pytest.mark.parametrize("n_shards", [1, 3])
def test_node_index_equals_one_index(n_shards):
    from vod_amd.index import HipNodeIndex

    q, x = _int_data(20, 3000, 128, 6)
    row_labels = (np.arange(len(x)) % 3).astype(np.int32)
    q_labels = np.array([[0], [1], [-1], [2], [-2], [0]], dtype=np.int32)
    ids = _lists(20, 6, 385, len(x))  # random rows of every shard in every list, the shard edges 999 / 1000 / 1999 / 2000 among them
    ids[0, :4] = [999, 1000, 1999, 2000]
    with _flat(x) as ix, HipNodeIndex(128, len(x), [0] * n_shards) as nx:
        nx.set_param("host_staging", 1)
        nx.add(x)
        _check_both_forms(ix, q, x, ids, (10, 500), other=nx)
        ix.set_row_labels(row_labels)
        nx.set_row_labels(row_labels)
        _check_both_forms(ix, q, x, ids, (10,), row_labels=row_labels, q_labels=q_labels, other=nx)
        # tensors on devices[0] in -> tensors out, the same bits
        ref = R.score_ids_aligned(q, x, ids)
        got = nx.score_ids(_dev(q), _dev(ids))
        np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), ref)
        s, i = nx.score_ids(_dev(q), _dev(ids), 10)
        rs, ri = R.score_ids_topk(ref, ids, 10)
        np.testing.assert_array_equal(i.cpu().numpy(), ri)
        np.testing.assert_array_equal(s.cpu().numpy().astype(np.float64), rs)


def test_listed_call_on_a_side_stream_between_search_async_and_finish():
    from oracle.flat_ip import flat_ip_topk

    q, x = _int_data(22, 8192, 128, 70)
    ids = _lists(22, 70, 385, len(x))
    side = torch.cuda.Stream()
    with _flat(x) as ix:
        qd, idd = _dev(q), _dev(ids)
        torch.cuda.synchronize()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            got = ix.score_ids(qd, idd)
            ts, ti = ix.score_ids(qd, idd, 20)
        ix.finish()
        side.synchronize()
        rs, ri = flat_ip_topk(q, x, 100)
        np.testing.assert_array_equal(i.cpu().numpy(), ri)
        np.testing.assert_array_equal(s.cpu().numpy(), rs)
        ref = R.score_ids_aligned(q, x, ids)
        np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), ref)
        ls, li = R.score_ids_topk(ref, ids, 20)
        np.testing.assert_array_equal(ti.cpu().numpy(), li)
        np.testing.assert_array_equal(ts.cpu().numpy().astype(np.float64), ls)


def test_ragged_lists_are_padded_and_bad_arguments_are_refused():
    from vod_amd import _native
    from vod_amd.index import HipNodeIndex

    q, x = _int_data(23, 100, 64, 3)
    with _flat(x) as ix:
        got = ix.score_ids(q, [[5, 7, 9], [], [3]]).cpu().numpy()
        assert got.shape == (3, 3)
        np.testing.assert_array_equal(got.astype(np.float64), R.score_ids_aligned(q, x, np.array([[5, 7, 9], [-1, -1, -1], [3, -1, -1]])))
        with pytest.raises(_native.NativeLibraryError, match="at least one slot"):
            ix.score_ids(q, np.zeros((3, 0), np.int64))
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_MAX_LISTED"):
            ix.score_ids(q, np.zeros((3, 8193), np.int64), 5)
        for k in (0, 2049):
            with pytest.raises(_native.NativeLibraryError, match="out of range"):
                ix.score_ids(q, np.zeros((3, 4), np.int64), k)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            ix.score_ids(q, np.zeros((3, 4), np.int64), subset=np.zeros((3, 1), np.int32))
        with pytest.raises(ValueError, match="expected ids of shape"):
            ix.score_ids(q, np.zeros((2, 4), np.int64))
        assert np.isfinite(ix.score_ids(q, [[1], [2], [3]]).cpu().numpy()).all()  # a refused call leaves nothing behind
    with HipNodeIndex(64, 100, [0, 0]) as nx:
        nx.set_param("host_staging", 1)
        nx.add(x)
        with pytest.raises(_native.NativeLibraryError, match="at least one slot"):
            nx.score_ids(q, np.zeros((3, 0), np.int64))
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_MAX_LISTED"):
            nx.score_ids(q, np.zeros((3, 8193), np.int64), 5)
        with pytest.raises(_native.NativeLibraryError, match="out of range"):
            nx.score_ids(q, np.zeros((3, 4), np.int64), 2049)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.score_ids(q, np.zeros((3, 4), np.int64), subset=np.zeros((3, 1), np.int32))
