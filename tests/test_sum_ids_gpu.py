"""`sum_ids` and `listed_scores` (include/vodhip.h H2w, sum_listed_kernel of kernels_listed.hip) against the float64 restatement and
the derived bound of tests/sum_ids_ref.py.

Integer fixture: rows in -8 .. 8, weights in -4 .. 4 divided by 8 - every partial sum is exact in float32 up to m = 10 000
(10 000 * 8 * 4 = 320 000 eighths < 2^24), so ANY summation order gives the same bits and the device equals float64 bit for bit: across
the kernel's column passes and column blocks (512 / 2048 columns), the 4 rows a wave has in flight, its 8-slot run, the 32-slot chunk
and one / two / many chunks through the fold, and batch sizes.  Gaussian data: every element inside the derived bound (no tolerance
here is fitted); the fraction of the bound each case reaches is printed.
Measured on an MI355X: 0.1 % of the bound with N(0, 1) weights and 0.5 - 0.8 % with softmax weights (dim 768 / 4096, fp16 / bf16), 0.1 % on
the exact_f32 store, 0.2 % on the node index; `listed_scores` backward 0.3 % (float32 queries), 75 % / 93 % (fp16 / bf16 queries: the
cast of the gradient is the error); the two identities 13 % and 25 % of the sum of the two bounds.
"""
import functools

import numpy as np
import pytest

import posterior_ref as PR
import sum_ids_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
CHUNK, BLOCK = 32, 2048  # slots of a sum workgroup, columns of a column block (kernels_listed.hip: SC, SB)


def _flat(x, dtype=torch.float16, capacity=None, exact=False):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(x.shape[1], capacity or max(len(x), 1), dtype=dtype, device=0, exact_f32=exact)
    ix.add(x)
    return ix


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _round(a, dtype):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(DTYPES[dtype]).double().numpy()


@functools.lru_cache(maxsize=None)
def _int_rows(seed, n, d):
    x = np.random.default_rng(seed).integers(-8, 9, size=(n, d)).astype(np.float32)
    x.setflags(write=False)
    return x


def _int_lists(seed, nq, m, ntotal, id_base=0):
    """ids [nq, m]: random rows with empty slots, id = ntotal, an id >= 2^32 and one id three times where m leaves room; query 1 (if any)
    lists only -1.  weights [nq, m]: integers in -4 .. 4 over 8 (zeros among them); NaN / inf on some of the absent slots."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, ntotal, size=(nq, m)).astype(np.int64) + id_base
    ids[rng.random((nq, m)) < 0.1] = -1
    special = [id_base + ntotal - 1, id_base + ntotal, (1 << 32) + 5 + id_base, id_base + 3, id_base + 3, id_base + 3, id_base]
    for i in range(nq):
        pos = rng.permutation(m)[: len(special)]
        ids[i, pos] = special[: len(pos)]
    if nq > 1:
        ids[1] = -1
    w = (rng.integers(-4, 5, size=(nq, m)) / 8).astype(np.float32)
    absent = (ids < id_base) | (ids >= id_base + ntotal)
    w[absent & (rng.random((nq, m)) < 0.5)] = np.nan
    w[absent & (rng.random((nq, m)) < 0.2)] = np.inf
    return ids, w


def _check_exact(ix, x, ids, w, other=None, **kw):
    ref, _ = R.sum_ids(x, ids, w, kw.get("id_base", 0))
    got = ix.sum_ids(_dev(ids), _dev(w), **kw)
    assert got.dtype == torch.float32 and got.shape == (len(ids), x.shape[1]) and got.is_cuda
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got.astype(np.float64), ref)
    if other is not None:
        np.testing.assert_array_equal(other.sum_ids(ids, w), got)
    return got


# ---- bit-exact on the integer fixture ---------------------------------------------------------------------------------------------
# dim -> dim_pad: 1, 64 -> 64 (part of one 512-column pass); 100 -> 128; 512 (one pass), 520 -> 576 (a pass + tail); 768 (the workload);
# 1030 -> 1088; 2048 (one full column block), 2056 -> 2112 (a second column block of one partial pass); 16384 (8 column blocks)
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("dim", [1, 64, 100, 512, 520, 768, 1030, BLOCK, BLOCK + 8, 16384])
def test_widths_bit_exact(dim, dtype):
    n = 4096
    x = _int_rows(100 + dim, n, dim)
    ids, w = _int_lists(dim, 3, 65, n, 1000)
    with _flat(x, DTYPES[dtype]) as ix:
        _check_exact(ix, x, ids, w, id_base=1000)


# the tail of the 4 rows in flight (1, 3, 4, 5), the edge of a wave's 8-slot run and of the chunk (31, 32, 33: one and two chunks),
# 63 / 64 / 65, the two benchmark shapes (13 and 32 chunks), 313 chunks
@pytest.mark.parametrize("m", [1, 3, 4, 5, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 63, 64, 65, 385, 1000, 10000])
def test_list_lengths_bit_exact(m):
    x = _int_rows(12, 8192, 100)
    ids, w = _int_lists(m, 3, m, len(x))
    with _flat(x) as ix:
        _check_exact(ix, x, ids, w)


@pytest.mark.parametrize("nq", [1, 3, 64, 257])
def test_batch_sizes_bit_exact(nq):
    x = _int_rows(13, 4096, 768)
    ids, w = _int_lists(nq, nq, 385, len(x))
    with _flat(x, torch.bfloat16) as ix:
        _check_exact(ix, x, ids, w)


# ---- order ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauss(seed, n, d):
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed)).numpy()
    x.setflags(write=False)
    return x


def test_a_query_has_the_same_bits_alone_elsewhere_in_a_larger_batch_and_on_a_repeat():
    x = _gauss(21, 5000, 768)
    rng = np.random.default_rng(21)
    ids = rng.integers(0, len(x), size=(257, 1000)).astype(np.int64)
    w = rng.standard_normal((257, 1000)).astype(np.float32)
    with _flat(x) as ix:
        idd, wd = _dev(ids), _dev(w)
        big = ix.sum_ids(idd, wd).cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(ix.sum_ids(idd, wd).cpu().numpy().view(np.uint32), big)  # a repeat
        for qi in (0, 100, 256):
            one = ix.sum_ids(ids[qi : qi + 1], w[qi : qi + 1]).cpu().numpy().view(np.uint32)  # alone
            np.testing.assert_array_equal(one[0], big[qi])
        perm = rng.permutation(257)
        np.testing.assert_array_equal(ix.sum_ids(ids[perm], w[perm]).cpu().numpy().view(np.uint32), big[perm])  # at another position
        np.testing.assert_array_equal(ix.sum_ids(ids[5:69], w[5:69]).cpu().numpy().view(np.uint32), big[5:69])  # in a smaller batch
        # (the order is the query's own: a permuted list is another sum, inside the bound but not the same bits everywhere)
        p = rng.permutation(1000)
        assert (ix.sum_ids(ids[:4, p], w[:4, p]).cpu().numpy().view(np.uint32) != big[:4]).any()


# ---- skipping ---------------------------------------------------------------------------------------------------------------------
def test_absent_slots_carry_nan_and_inf_weights_and_add_nothing():
    """-1, out of range, below id_base, left behind by reset(), excluded by subset: the result equals the call with those slots
    removed, bit for bit (integer fixture: the remaining slots move, and any order gives the same bits)"""
    x = _int_rows(14, 4096, 100)
    row_labels = (np.arange(2048) % 5).astype(np.int32)
    q_labels = np.array([[1, 3, -1], [-1, -1, -1], [9, -2, -1], [0, -1, -1]], dtype=np.int32)
    rng = np.random.default_rng(14)
    ids = rng.integers(0, 2048, size=(4, 200)).astype(np.int64) + 500
    w = (rng.integers(-4, 5, size=(4, 200)) / 8).astype(np.float32)
    ids[:, 3], ids[:, 50], ids[:, 51], ids[:, 52], ids[:, 99] = -1, 499, 500 + 2048, 500 + 3000, (1 << 40)  # 3000: a row reset() left behind
    with _flat(x, capacity=4096) as ix:
        ix.reset()
        ix.add(x[:2048])
        ix.set_row_labels(row_labels)
        keep = R.contributing(ids, np.ones_like(w), 2048, 500, row_labels, q_labels)
        assert not keep[:, [3, 50, 51, 52, 99]].any() and not keep[2].any() and keep[1].sum() == 195 and 20 < keep[0].sum() < 150
        poisoned = w.copy()
        poisoned[~keep] = np.resize(np.array([np.nan, np.inf, -np.inf, 3.5], dtype=np.float32), (~keep).sum())
        got = ix.sum_ids(ids, poisoned, subset=q_labels, id_base=500).cpu().numpy()
        ref, _ = R.sum_ids(x[:2048], ids, poisoned, 500, row_labels, q_labels)
        np.testing.assert_array_equal(got.astype(np.float64), ref)
        assert (got[2] == 0).all() and np.isfinite(got).all()  # an all-absent list: the zero row
        removed = ix.sum_ids([r[k] for r, k in zip(ids, keep)], [r[k] for r, k in zip(w, keep)], subset=q_labels, id_base=500).cpu().numpy()
        np.testing.assert_array_equal(removed.view(np.uint32), got.view(np.uint32))
        # no label of this call sticks: the same lists unrestricted
        ref, _ = R.sum_ids(x[:2048], ids, w, 500)
        np.testing.assert_array_equal(ix.sum_ids(ids, w, id_base=500).cpu().numpy().astype(np.float64), ref)


def test_zero_weights_nan_rows_nan_weights_and_duplicates():
    x = _int_rows(15, 4096, 100).copy()
    x[5, [3, 70]] = np.nan
    x[6, 9] = np.inf
    nan = np.nan
    ids = np.array([[4, 5, 6, 7], [4, 5, 7, 5], [4, 4, 4, 7], [4, 7, 8, 9], [5, 6, -1, -1]], dtype=np.int64)
    w = np.array([[1, 0.0, -0.0, 2], [1, 0.5, 2, 0], [1, 1, -0.5, 0.25], [1, nan, 1, 1], [0, 0, nan, 1]], dtype=np.float32)
    with _flat(x) as ix:
        got = ix.sum_ids(ids, w).cpu().numpy()
        ref, _ = R.sum_ids(x, ids, w)
        assert np.isfinite(got[0]).all()                                        # zero weights (either sign) skip the NaN and the inf row
        assert np.isnan(got[1, [3, 70]]).all() and np.isfinite(np.delete(got[1], [3, 70])).all()  # a non-zero weight: exactly those columns
        np.testing.assert_array_equal(got[2], 1.5 * x[4] + 0.25 * x[7])         # duplicates add, once per slot
        assert np.isnan(got[3]).all()                                           # a NaN weight on a present slot: that query's row ...
        assert (got[4] == 0).all()                                              # ... and every slot skipped: the zero row
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_array_equal(got[~np.isnan(ref)].astype(np.float64), ref[~np.isnan(ref)])
        alone = ix.sum_ids(ids[[0, 1, 2, 4]], w[[0, 1, 2, 4]]).cpu().numpy()    # ... and no other query's row changes
        np.testing.assert_array_equal(alone.view(np.uint32), got[[0, 1, 2, 4]].view(np.uint32))


# ---- Gaussian data inside the derived bound -----------------------------------------------------------------------------------------
def _check_bound(got, ref, bound, what):
    assert np.isfinite(got).all() and got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref)
    frac = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"{what}: max |device - float64| = {err.max():.3e}, largest fraction of the bound = {frac.max():.3f}")
    assert (err <= bound).all(), (what, frac.max())
    return frac.max()


@pytest.mark.parametrize("weights", ["normal", "softmax"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("dim", [768, 4096])
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, weights):
    x = _gauss(dim, 4096, dim)
    rng = np.random.default_rng(dim)
    ids = rng.integers(0, len(x), size=(9, 1000)).astype(np.int64)
    ids[rng.random(ids.shape) < 0.05] = -1
    ids[1] = -1
    if weights == "normal":
        w = rng.standard_normal(ids.shape).astype(np.float32)
    else:
        z = rng.standard_normal(ids.shape) * 3
        w = (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).astype(np.float32)
    with _flat(x, DTYPES[dtype]) as ix:
        got = ix.sum_ids(ids, w).cpu().numpy()
    ref, bound = R.sum_ids(_round(x, dtype), ids, w)
    assert (got[1] == 0).all()
    _check_bound(got, ref, bound, f"dim {dim} {dtype} {weights} weights")


def test_exact_f32_store_sums_the_float32_plane():
    rng = np.random.default_rng(31)
    x = (1 + rng.integers(1, 16, size=(4096, 768)) * 2.0 ** -20).astype(np.float32) * rng.choice([-1.0, 1.0], size=(4096, 768)).astype(np.float32)
    ids = rng.integers(0, len(x), size=(5, 385)).astype(np.int64)
    w = rng.standard_normal(ids.shape).astype(np.float32)
    with _flat(x, exact=True) as ix:
        got = ix.sum_ids(ids, w).cpu().numpy()
        rounded_rows = ix.stored_rows().float().cpu().numpy()
    ref, bound = R.sum_ids(x, ids, w)  # float64 of the UNROUNDED rows
    _check_bound(got, ref, bound, "exact_f32 store")
    rounded, _ = R.sum_ids(rounded_rows, ids, w)  # the fp16 plane holds +-1: another sum, which the device did not compute
    assert (np.abs(x) != 1).all() and (np.abs(rounded_rows) == 1).all()
    assert (got != rounded.astype(np.float32)).mean() > 0.99
    assert np.abs(got - ref).max() < np.abs(got - rounded).max()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    x = _int_rows(23, 4096, 64)
    ids, w = np.zeros((3, 4), np.int64), np.ones((3, 4), np.float32)
    with _flat(x) as ix:
        with pytest.raises(_native.NativeLibraryError, match="at least one slot"):
            ix.sum_ids(np.zeros((3, 0), np.int64), np.zeros((3, 0), np.float32))
        for bad in (np.ones((3, 5), np.float32), np.ones((2, 4), np.float32), torch.ones(3, 5).cuda()):
            with pytest.raises(ValueError, match="expected weights of shape"):
                ix.sum_ids(ids, bad)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            ix.sum_ids(ids, w, subset=np.zeros((3, 1), np.int32))
        with pytest.raises(ValueError, match="expected subset labels of shape"):
            ix.sum_ids(ids, w, subset=np.zeros((2, 1), np.int32))
        np.testing.assert_array_equal(ix.sum_ids(ids, w).cpu().numpy(), np.tile(4 * x[0], (3, 1)))  # a refused call leaves nothing behind
    with HipFlatIndex(64, 4096, device=0, metric="l2") as l2:
        l2.add(x)
        with pytest.raises(_native.NativeLibraryError, match="not supported on an L2 index"):
            l2.sum_ids(ids, w)
        with pytest.raises(_native.NativeLibraryError, match="not supported on an L2 index"):
            l2.listed_scores(torch.ones(3, 64, device="cuda", requires_grad=True), ids)
    with HipNodeIndex(64, 4096, [0, 0]) as nx:
        nx.set_param("host_staging", 1)
        nx.add(x)
        with pytest.raises(_native.NativeLibraryError, match="at least one slot"):
            nx.sum_ids(np.zeros((3, 0), np.int64), np.zeros((3, 0), np.float32))
        with pytest.raises(ValueError, match="expected weights of shape"):
            nx.sum_ids(ids, np.ones((3, 5), np.float32))
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.sum_ids(ids, w, subset=np.zeros((3, 1), np.int32))


# ---- the node index -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards", [1, 3])
def test_node_index(n_shards):
    from vod_amd.index import HipNodeIndex

    x = _int_rows(20, 6000, 128)
    ids, w = _int_lists(20, 6, 385, len(x))
    ids[0, :4] = [1999, 2000, 3999, 4000]  # the shard edges
    row_labels = (np.arange(len(x)) % 3).astype(np.int32)
    q_labels = np.array([[0], [1], [-1], [2], [-2], [0]], dtype=np.int32)
    g = _gauss(20, 6000, 128)
    gw = np.random.default_rng(20).standard_normal(ids.shape).astype(np.float32)
    with _flat(x) as ix, HipNodeIndex(128, len(x), [0] * n_shards) as nx:
        nx.set_param("host_staging", 1)
        nx.add(x)
        got = _check_exact(ix, x, ids, w, other=nx)  # host buffers: NumPy out, the flat index's bits
        dev = nx.sum_ids(_dev(ids), _dev(w))          # devices[0] buffers: a tensor there
        assert isinstance(dev, torch.Tensor) and dev.is_cuda
        np.testing.assert_array_equal(dev.cpu().numpy(), got)
        ix.set_row_labels(row_labels)
        nx.set_row_labels(row_labels)
        ref, _ = R.sum_ids(x, ids, w, 0, row_labels, q_labels)
        np.testing.assert_array_equal(nx.sum_ids(ids, w, subset=q_labels).astype(np.float64), ref)
        np.testing.assert_array_equal(ix.sum_ids(ids, w, subset=q_labels).cpu().numpy().astype(np.float64), ref)
    with HipNodeIndex(128, len(g), [0] * n_shards) as nx:
        nx.set_param("host_staging", 1)
        nx.add(g)
        got = nx.sum_ids(ids, gw)
        ref, bound = R.sum_ids(_round(g, "float16"), ids, gw)
        _check_bound(got, ref, bound, f"node index, {n_shards} shards")
        np.testing.assert_array_equal(nx.sum_ids(ids, gw).view(np.uint32), got.view(np.uint32))           # a repeat
        np.testing.assert_array_equal(nx.sum_ids(_dev(ids), _dev(gw)).cpu().numpy().view(np.uint32), got.view(np.uint32))


# ---- beside searches ----------------------------------------------------------------------------------------------------------------
def test_a_call_on_a_side_stream_between_search_async_and_finish():
    from oracle.flat_ip import flat_ip_topk

    x = _int_rows(22, 8192, 128)
    q = np.random.default_rng(22).integers(-8, 9, size=(70, 128)).astype(np.float32)
    ids, w = _int_lists(22, 70, 385, len(x))
    side = torch.cuda.Stream()
    with _flat(x) as ix:
        qd, idd, wd = _dev(q), _dev(ids), _dev(w)
        torch.cuda.synchronize()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            got = ix.sum_ids(idd, wd)
        ix.finish()
        side.synchronize()
        rs, ri = flat_ip_topk(q, x, 100)
        np.testing.assert_array_equal(i.cpu().numpy(), ri)
        np.testing.assert_array_equal(s.cpu().numpy(), rs)
        np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), R.sum_ids(x, ids, w)[0])


# ---- listed_scores --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qdt", ["float32", "float16", "bfloat16"])
def test_listed_scores_forward_bits_and_backward(qdt):
    x = _gauss(41, 4096, 768)
    rng = np.random.default_rng(41)
    ids = rng.integers(0, len(x), size=(7, 385)).astype(np.int64)
    ids[rng.random(ids.shape) < 0.1] = -1
    ids[2] = -1
    g = rng.standard_normal(ids.shape).astype(np.float32)
    g[ids < 0] = np.nan  # what a loss over -inf scores sends back
    qt = torch.randn(7, 768, generator=torch.Generator().manual_seed(41)).cuda().to(getattr(torch, qdt)).requires_grad_()
    with _flat(x) as ix:
        idd, gd = _dev(ids), _dev(g)
        s = ix.listed_scores(qt, idd)
        assert s.requires_grad and s.dtype == torch.float32
        fwd = ix.score_ids(qt.detach(), idd)
        assert torch.equal(s.detach().view(torch.int32), fwd.view(torch.int32)) and torch.isneginf(s[2]).all()
        s.backward(gd)
        want = ix.sum_ids(idd, gd).to(qt.dtype)
        assert qt.grad.dtype == qt.dtype and qt.grad.device == qt.device and torch.isfinite(qt.grad).all()
        assert torch.equal(qt.grad, want) and (qt.grad[2] == 0).all()
        assert ix.listed_scores(qt.detach(), ids.tolist()).requires_grad is False  # (ragged lists work; nothing to differentiate)
    # against float64 torch autograd over the materialised gather of the rounded rows
    x64 = torch.from_numpy(_round(x, "float16"))
    q64 = qt.detach().double().cpu().requires_grad_()
    live = torch.from_numpy(ids >= 0)
    dense = (x64[torch.from_numpy(np.clip(ids, 0, None))] @ q64[:, :, None])[:, :, 0]
    (torch.where(live, dense, torch.zeros((), dtype=torch.float64)) * torch.from_numpy(np.nan_to_num(g)).double()).sum().backward()
    ref, bound = R.sum_ids(x64.numpy(), ids, g)
    np.testing.assert_allclose(q64.grad.numpy(), ref, rtol=0, atol=1e-9)  # (the restatement is that autograd)
    err = np.abs(qt.grad.double().cpu().numpy() - q64.grad.numpy())
    tol = R.cast_bound(ref, bound, qdt)
    print(f"listed_scores backward, {qdt} queries: max |grad - float64| = {err.max():.3e}, largest fraction of the bound = {(err / np.maximum(tol, 1e-300)).max():.3f}")
    assert (err <= tol).all()


def test_node_index_listed_scores_from_a_cpu_leaf():
    from vod_amd.index import HipNodeIndex

    x = _int_rows(20, 6000, 128)
    ids, _ = _int_lists(24, 5, 65, len(x))
    rng = np.random.default_rng(24)
    g = (rng.integers(-4, 5, size=ids.shape) / 8).astype(np.float32)
    g[(ids < 0) | (ids >= len(x))] = np.nan
    q = torch.from_numpy(rng.integers(-8, 9, size=(5, 128)).astype(np.float32)).requires_grad_()  # a leaf on the host
    with _flat(x) as ix, HipNodeIndex(128, len(x), [0, 0, 0]) as nx:
        nx.set_param("host_staging", 1)
        nx.add(x)
        s = nx.listed_scores(q, ids)
        assert s.is_cuda and s.requires_grad
        assert torch.equal(s.detach().view(torch.int32), ix.score_ids(q.detach().cuda(), ids).view(torch.int32))
        s.backward(_dev(g))
    assert q.grad.device == q.device and q.grad.dtype == torch.float32
    np.testing.assert_array_equal(q.grad.numpy().astype(np.float64), R.sum_ids(x, ids, g)[0])


# ---- two identities that tie the feature to log_z and sample_posterior ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_store():
    rng = np.random.default_rng(51)
    x = (rng.standard_normal((180, 64)) * 0.5).astype(np.float32)
    q = rng.standard_normal((6, 64)).astype(np.float32)
    return q, x


def test_gradient_of_logsumexp_of_all_listed_scores_is_the_gradient_of_log_z():
    q, x = _small_store()
    T = 2.0
    beta = 1.0 / T
    all_ids = np.tile(np.arange(len(x), dtype=np.int64), (len(q), 1))
    with _flat(x) as ix:
        qa = _dev(q).requires_grad_()
        (T * torch.logsumexp(ix.listed_scores(qa, all_ids) / T, dim=1)).sum().backward()
        qb = _dev(q).requires_grad_()
        (T * ix.log_z(qb, T)).sum().backward()
        s = ix.score_ids(_dev(q), all_ids).double().cpu().numpy()
    # both are the posterior mean: within the sum of the two derived bounds (the softmax weights that reach sum_ids are the ones a
    # float64 softmax of the device's scores gives, to float32 rounding)
    mean, _, _ = PR.posterior_mean(q, x, "float16", beta)
    p = np.exp(beta * s - (beta * s).max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    _, sum_bound = R.sum_ids(_round(x, "float16"), all_ids, p)
    pm_bound = PR.device_bound(q, x, "float16", beta, dot=True)
    tol = sum_bound + pm_bound
    ga, gb = qa.grad.double().cpu().numpy(), qb.grad.double().cpu().numpy()
    print(f"grad T logsumexp(listed_scores / T) vs grad T log_z: max |diff| = {np.abs(ga - gb).max():.3e}, largest fraction = {(np.abs(ga - gb) / tol).max():.3f}")
    assert (np.abs(ga - mean) <= tol).all()
    assert (np.abs(ga - gb) <= tol).all()


def test_sum_ids_over_a_complete_posterior_sample_is_the_posterior_mean():
    q, x = _small_store()
    with _flat(x) as ix:
        qd = _dev(q)
        s = ix.sample_posterior(qd, 200, seed=7)  # k >= the 180 rows: every row is drawn, log_tau = -inf, the weights are the probabilities
        assert torch.isneginf(s.log_tau).all() and ((s.ids >= 0).sum(dim=1) == len(x)).all()
        weights = torch.exp(s.log_weight)
        got = ix.sum_ids(s.ids, weights).double().cpu().numpy()
        pm = ix.posterior_mean(qd).mean.double().cpu().numpy()
        ids, w = s.ids.cpu().numpy(), weights.cpu().numpy()
    ref, sum_bound = R.sum_ids(_round(x, "float16"), ids, w)
    assert (np.abs(got - ref) <= sum_bound).all()                      # the sum of what it was given ...
    pm_bound = PR.device_bound(q, x, "float16", 1.0, dot=True)
    tol = sum_bound + pm_bound                                        # ... which are the probabilities of posterior_mean
    print(f"sum_ids(sample) vs posterior_mean: max |diff| = {np.abs(got - pm).max():.3e}, largest fraction = {(np.abs(got - pm) / tol).max():.3f}")
    assert (np.abs(got - pm) <= tol).all()
