"""`HipFlatIndex.posterior_mean` / `log_z` / `HipNodeIndex.posterior_mean` on the GPU against the float64 restatement
(tests/posterior_ref.py); every element of every case is compared against `posterior_ref.device_bound`, which is derived, not fitted.

Integer data (values in [-8, 8]: exact in fp16 and bf16, every score an exact integer in float32, so the bound's dot-product part is
dropped): stores of 1, 5, 255, 256, 257, 1500 and 3000 rows, one on each side of a group boundary (G = 16384 rows) and two groups plus a
partial tile, widths 1, 64, 65, 765, 768 and 570 (dim_pad 576: two 256-column chunks and one extra 64-column slice), batches 1, 64, 65,
129, 300, beta 1, 1/64, 4; `max_score` and `log_rel` carry the bits of `log_partition` on the same index.  Then: one-hot posteriors (the
test of the transposed reads' row order), ties, flat and deep tails over 300 000 rows, a column of ones, subset labels, stale rows, NaN
and +inf, batch independence, Gaussian data within the full bound, autograd, a call beside a search in flight, the node index, refusals.
Measured maxima (MI355X): DESIGN.md 4 "Posterior mean" and profiles/posterior_mean.json.
"""
import ctypes
import functools

import numpy as np
import pytest

import partition_ref as P
import posterior_ref as R
from test_l2_cpu import GAUSS_CASES, gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
STORES = [1, 5, 255, 256, 257, 1500, 3000]
WIDTHS = [1, 64, 65, 765, 768, 570]
BATCHES = [1, 64, 65, 129, 300]
BETAS = [1.0, 1.0 / 64.0, 4.0]
G = R.GROUP_ROWS


def _index(x, dtype="float16", capacity=None, dim=None, **kw):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, **kw)
    if len(x):
        ix.add(x)
    return ix


@functools.lru_cache(maxsize=None)
def _int_case(d, n=3000, nq=300):
    """integer rows / queries; the same for both store dtypes (both hold the values exactly); every score is exact in float32"""
    rng = np.random.default_rng(7000 + d + n)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    for a in (q, x):
        a.setflags(write=False)
    return q, x


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _pm(ix, q, beta=1.0, **kw):
    """(mean, log_z, max_score, log_rel) as NumPy, and the bits of log_partition on the same index are asserted equal"""
    qd = _dev(q)
    r = ix.posterior_mean(qd, temperature=1.0 / beta, **kw)
    lp = ix.log_partition(qd, temperature=1.0 / beta, **kw)
    assert r.mean.dtype == torch.float32 and r.mean.shape == (len(q), ix.dim) and r.mean.is_cuda
    for a, b in zip(r.log_partition, lp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return (r.mean.cpu().numpy(),) + tuple(t.cpu().numpy() for t in r.log_partition)


def _check(got, q, x, dtype, beta, eligible=None, dot=False, what="", cols=None):
    """every (query, column) within the derived bound; queries without a finite log Z: the zero row"""
    mean = got[0]
    ref, rm, _ = R.posterior_mean(q, x, dtype, beta, eligible)
    bound = R.device_bound(q, x, dtype, beta, eligible, dot=dot)
    live = np.isfinite(rm)
    assert np.array_equal(np.isfinite(got[2]), live), what
    assert (mean[~live] == 0).all(), what
    err = np.abs(mean.astype(np.float64) - ref)
    if cols is not None:
        err, bound = err[:, cols], bound[:, cols]
    ratio = np.divide(err[live], bound[live], out=np.zeros_like(err[live]), where=bound[live] > 0).max() if live.any() else 0.0
    print(f"{what}: max |mean - float64| = {err[live].max() if live.any() else 0.0:.3e}, max err / bound = {ratio:.3e}")
    assert not np.isnan(err[live]).any(), what
    assert (err[live] <= bound[live]).all(), (what, ratio)
    return ratio


# ---- sizes, widths, batches, betas on integer data ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_widths_batches_and_betas(n, d, dtype):
    q, x = _int_case(d)
    x = x[:n]
    with _index(x, dtype) as ix:
        full = {}
        for beta in BETAS:
            full[beta] = _pm(ix, q, beta)
            _check(full[beta], q, x, dtype, beta, what=f"n {n} d {d} {dtype} beta {beta:g}")
        for nq in BATCHES[:-1]:
            beta = BETAS[nq % 3]
            got = _pm(ix, q[:nq], beta)
            for a, b in zip(got, full[beta]):
                assert np.array_equal(a.view(np.uint32), b[:nq].view(np.uint32)), (nq, beta)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [G - 1, G + 1, 2 * G + 5])
def test_stores_around_a_group_boundary(n, dtype):
    q, x = _int_case(65, n=2 * G + 5, nq=129)
    for beta in (1.0 / 64.0, 1.0):
        with _index(x[:n], dtype) as ix:
            _check(_pm(ix, q, beta), q, x[:n], dtype, beta, what=f"group edge n {n} {dtype} beta {beta:g}")


# ---- one-hot posteriors: the row order of the transposed reads ------------------------------------------------------------------------
TOPS = [1, 5, 70, 78 + 4, 147, 154 + 36, 200, 252, 256 + 9, 256 + 64 + 13, 256 + 128 + 50, 256 + 192 + 31, 512 + 3, 512 + 22, 512 + 47, 599]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 768])
def test_one_hot_posterior_returns_the_top_row(d, dtype):
    assert {((t % 256) // 64, (t % 8) // 4) for t in TOPS} == {(w, h) for w in range(4) for h in range(2)}  # 4 row waves x 2 lane halves
    rng = np.random.default_rng(d)
    n = 600
    x = rng.integers(-1, 2, size=(n, d)).astype(np.float32)
    q = rng.integers(-1, 2, size=(len(TOPS), d)).astype(np.float32)
    x[:, : len(TOPS)] = 0
    q[:, : len(TOPS)] = 0
    for i, t in enumerate(TOPS):  # query i scores row t 2048 + .., every other row at most d: a margin above 512
        x[t, i] = 8
        q[i, i] = 256
    s = q.astype(np.float64) @ x.astype(np.float64).T
    assert (np.argmax(s, axis=1) == TOPS).all() and (np.sort(s, axis=1)[:, -1] - np.sort(s, axis=1)[:, -2] >= 512).all()
    with _index(x, dtype) as ix:
        got = _pm(ix, q, 64.0)
    tol = n * np.exp(-64.0) * 8 + 2.0 ** -23 * np.abs(x[TOPS])
    np.testing.assert_array_less(np.abs(got[0] - x[TOPS]), tol + 1e-30)
    _check(got, q, x, dtype, 64.0, what=f"one-hot d {d} {dtype}")


# ---- ties ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("other", [300, G + 700])
def test_two_tied_top_rows_give_their_average(other, dtype):
    _, x = _int_case(65, n=2 * G + 5, nq=129)
    x = np.array(x[: G + 1000])
    x[:, 0] = 0
    x[10, 0] = x[other, 0] = 8
    q = np.zeros((3, 65), dtype=np.float32)
    q[:, 0] = 256  # the two rows score 2048, every other row 0: with beta 1 their weights are exp(-2048) = 0
    with _index(x, dtype) as ix:
        got = _pm(ix, q, 1.0)
    avg = (x[10].astype(np.float64) + x[other]) / 2
    # P' = 1 twice and exact sums; what is left is logf(2) (1 ulp of 0.69: u in the exponent), expf (1 ulp: 2 u), the product (u) and
    # the sum of the two groups' terms (u): 5 u relative, asserted at 6 u
    mag = (np.abs(x[10]).astype(np.float64) + np.abs(x[other])) / 2  # (in two groups the halves are added after the product rounded)
    assert (np.abs(got[0] - avg[None, :]) <= 6 * 2.0 ** -24 * mag[None, :] + 1e-30).all()
    _check(got, q, x, dtype, 1.0, what=f"tie rows 10 / {other} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_1024_identical_rows_give_that_row(dtype):
    q, x = _int_case(65)
    rows = np.repeat(x[:1], 1024, axis=0)
    with _index(rows, dtype) as ix:
        got = _pm(ix, q[:70], 4.0)
    # 1024 weights of exactly 1 and exact sums (|1024 x| <= 8192); the coefficient is expf(-logf(1024)): logf is 1 ulp of 6.93
    # (2^-21 absolute = relative in the exponential), expf 1 ulp (2^-23), the product half an ulp (2^-24)
    tol = (2.0 ** -21 + 2.0 ** -23 + 2.0 ** -24) * 1.01 * np.abs(x[0])
    assert (np.abs(got[0] - x[0][None, :]) <= tol[None, :] + 1e-30).all(), np.abs(got[0] - x[0][None, :]).max()


# ---- flat and deep tails ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_and_deep_tails_over_300000_rows(dtype):
    n, d = 300_000, 64
    rng = np.random.default_rng(5)
    base = rng.integers(-8, 9, size=d).astype(np.float32)
    base[0] = 0
    q = rng.integers(-2, 3, size=(4, d)).astype(np.float32)
    q[:, 0] = 1
    x = np.repeat(base[None, :], n, axis=0)
    with _index(x, dtype) as ix:
        _check(_pm(ix, q, 1.0), q, x, dtype, 1.0, what=f"flat tail {dtype}")  # every row the same: p = 1 / n
        for beta in (1.0, 0.25):
            top = rng.integers(-8, 9, size=d).astype(np.float32)
            top[1:] = np.where(q[0, 1:] != 0, base[1:], top[1:])  # the same score as the tail apart from column 0 (for query 0)
            top[0] = 20.0 / beta                                   # one row ahead by 20 / beta: the tail is e^-20 ~ 2^-28.9 of it
            x[123_457] = top
            ix.reset()
            ix.add(x)
            _check(_pm(ix, q, beta), q, x, dtype, beta, what=f"deep tail {dtype} beta {beta:g}")


# ---- normalisation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_of_ones_has_mean_one(dtype):
    q, x = _int_case(65)
    x = np.array(x)
    x[:, 64] = 1
    for beta in (1.0 / 64.0, 1.0):
        with _index(x, dtype) as ix:
            got = _pm(ix, q[:129], beta)
        bound = R.device_bound(q[:129], x, dtype, beta, dot=False)[:, 64]
        assert (np.abs(got[0][:, 64].astype(np.float64) - 1.0) <= bound).all()
        _check(got, q[:129], x, dtype, beta, what=f"ones column {dtype} beta {beta:g}")


# ---- masks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 132])
def test_subset_labels(nq, dtype):
    q, x = _int_case(65)
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        for beta in (1.0, 1.0 / 64.0):
            got = _pm(ix, q[:nq], beta, subset=sub)
            _check(got, q[:nq], x, dtype, beta, elig, what=f"subset nq {nq} {dtype} beta {beta:g}")
            assert (got[0][3::4] == 0).all() and np.isneginf(got[1][3::4]).all()  # no eligible row: the zero row
        _check(_pm(ix, q[:nq], 1.0), q[:nq], x, dtype, 1.0, what="row labels without query labels")


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_past_ntotal_are_never_counted(dtype):
    q, x = _int_case(65)
    b = 1.0 / 64.0
    with _index(x, dtype, capacity=3000) as ix:
        ix.reset()
        ix.add(x[2300:])  # 700 rows; rows 700 .. 2999 of the store still hold the first ingest
        assert ix.ntotal == 700
        _check(_pm(ix, q[:129], b), q[:129], x[2300:], dtype, b, what=f"reset {dtype}")
    with _index(x[:700], dtype, capacity=3000) as ix:  # nothing beyond ntotal was ever written
        _check(_pm(ix, q[:129], b), q[:129], x[:700], dtype, b, what=f"capacity > ntotal {dtype}")
    with _index(x[:300], dtype, capacity=300) as ix:  # the last tile reaches past the capacity
        _check(_pm(ix, q[:65], 1.0), q[:65], x[:300], dtype, 1.0, what=f"tile padding {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_are_left_out_and_a_stored_nan_makes_its_column_nan(dtype):
    q, x = _int_case(65)
    q = np.array(q[:70])
    q[:, 0] = 1.0
    b = 1.0 / 64.0
    xn = np.array(x)
    xn[7, 3] = np.nan  # every score of row 7 is NaN: the row is left out of every sum - and column 3 of every mean is NaN (0 * NaN)
    keep = np.ones(len(x), dtype=bool)
    keep[7] = False
    others = np.arange(65) != 3
    with _index(xn, dtype) as ix:
        got = _pm(ix, q, b)  # (the two scalar words: log_partition's bits, asserted inside)
        _check(got, q, x[keep], dtype, b, what=f"NaN row {dtype}", cols=others)
        assert np.isnan(got[0][:, 3]).all() and np.isfinite(got[0][:, others]).all()
        # the same behind a reset: row 720 is stale (ntotal = 700) but inside the last scanned tile
        xs = np.array(x)
        xs[720, 5] = np.nan
        ix.reset()
        ix.add(xs)
        ix.reset()
        ix.add(x[:700])
        got = _pm(ix, q, b)
        _check(got, q, x[:700], dtype, b, what=f"stale NaN {dtype}", cols=np.arange(65) != 5)
        assert np.isnan(got[0][:, 5]).all()
    xi = np.array(x)
    xi[2999, 0] = np.inf  # +inf for every query (q[:, 0] = 1): the zero row
    with _index(xi, dtype) as ix:
        mean, log_z, m, r = _pm(ix, q, 1.0)
    assert np.isposinf(m).all() and np.isposinf(r).all() and (mean == 0).all()


# ---- one order -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 768])
def test_a_query_has_the_same_bits_in_any_batch_and_on_every_repeat(d, dtype):
    q, x = _int_case(d)
    rng = np.random.default_rng(d)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)  # inexact sums: the order matters
    qg = (q + rng.standard_normal(q.shape)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(xg, dtype) as ix:
        a = _pm(ix, qg, beta)
        b = _pm(ix, qg, beta)
        c = _pm(ix, qg[:64], beta)   # the 64-query instantiation of the partition scan
        e = _pm(ix, qg[:65], beta)   # the 128-query one
        for u, v, w, z in zip(a, b, c, e):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
            assert np.array_equal(u[:64].view(np.uint32), w.view(np.uint32))
            assert np.array_equal(u[:65].view(np.uint32), z.view(np.uint32))
        for j in (0, 63, 64, 217, 299):
            one = _pm(ix, qg[j : j + 1], beta)
            for u, v in zip(a, one):
                assert np.array_equal(u[j : j + 1].view(np.uint32), v.view(np.uint32)), j
    assert not np.isnan(a[0]).any()


# ---- Gaussian data: the full bound, every element -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    beta = float(np.float32(1.0 / np.sqrt(dim)))  # the float32 the call receives
    with _index(x, dtype) as ix:
        got = _pm(ix, q, beta)
    _check(got, q, x, dtype, beta, dot=True, what=f"gaussian dim {dim} {dtype}")


# ---- autograd ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qdt", [torch.float32, torch.float16])
def test_log_z_backward_on_the_gpu(qdt):
    dim, dtype, seed = GAUSS_CASES[0]
    q, x = gauss_case(dim, seed)
    T = float(np.sqrt(dim))
    beta = float(np.float32(1.0 / T))
    qt = _dev(q).to(qdt).requires_grad_(True)
    qh = qt.detach().float().cpu().numpy()  # what the index sees before it rounds to the store dtype
    with _index(x, dtype) as ix:
        lz = ix.log_z(qt, temperature=1.0 / beta)
        ref_lp = ix.log_partition(qt.detach(), temperature=1.0 / beta)
        assert lz.requires_grad and lz.dtype == torch.float32 and torch.equal(lz.detach().view(torch.int32), ref_lp.log_z.view(torch.int32))
        lz.sum().backward()
    g = qt.grad
    assert g.dtype == qdt and g.shape == qt.shape
    ref, _, _ = R.posterior_mean(qh, x, dtype, beta)
    bound = beta * R.device_bound(qh, x, dtype, beta, dot=True)
    want = beta * ref
    tol = bound + 2.0 ** -23 * (np.abs(want) + bound)  # beta * mean and its product with grad_out round in float32
    if qdt == torch.float16:  # the cast of grad_q to fp16 rounds once more (half a subnormal spacing at the least)
        tol = tol + 2.0 ** -11 * (np.abs(want) + tol) + 2.0 ** -25
    err = np.abs(g.float().cpu().numpy().astype(np.float64) - want)
    print(f"log_z backward, {qdt} queries: max |grad - float64| = {err.max():.3e}, max err / tol = {(err / tol).max():.3e}")
    assert (err <= tol).all()


# ---- beside searches ---------------------------------------------------------------------------------------------------------------------
def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x = _int_case(768)
    qd = _dev(q[:129])
    with _index(x, "float16") as ix:
        serial_s, serial_i = ix.search(qd, 100)
        serial = ix.posterior_mean(qd, temperature=64.0)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            pm = ix.posterior_mean(qd, temperature=64.0)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert torch.equal(pm.mean.view(torch.int32), serial.mean.view(torch.int32))
        for a, b in zip(pm.log_partition, serial.log_partition):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert ix.get_stat("last_overflow") == 0


# ---- node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards,capacity", [(1, 3000), (2, 3000), (3, 3000), (3, 12000)])
def test_node_index_folds_the_shards(n_shards, capacity):
    from vod_amd.index import HipNodeIndex

    q, x = _int_case(65)
    nq, beta = 129, 1.0 / 64.0
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, "float16") as ix:
        flat = _pm(ix, q[:nq], beta)
        ix.set_row_labels(labels)
        flat_sub = _pm(ix, q[:nq], beta, subset=sub)
    with HipNodeIndex(65, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        nx.add(x.astype(np.float32))
        got = nx.posterior_mean(np.array(q[:nq]), temperature=1.0 / beta)
        nx.set_row_labels(labels)
        got_sub = nx.posterior_mean(np.array(q[:nq]), temperature=1.0 / beta, subset=sub)
    for res, ref, e in ((got, flat, None), (got_sub, flat_sub, elig)):
        mean, lp = res
        assert isinstance(mean, np.ndarray) and mean.dtype == np.float32 and mean.shape == (nq, 65)
        assert np.array_equal(lp.max_score.view(np.uint32), ref[2].view(np.uint32))  # max_score: the flat index's bits
        want, rm, _ = R.posterior_mean(q[:nq], x, "float16", beta, e)
        live = np.isfinite(rm)
        # every shard is within the flat bound of its own rows (each shard's S adds up to the store's); the fold's weights use float32
        # (max, log_rel) pairs - log_rel within PB + 4 u (1 + log n) of the truth, as in the partition fold - and the result rounds once
        n = len(x) if e is None else e.sum(axis=1)
        fold = 2 * (P.device_bound(np.zeros((nq, 1)), None, None, beta, n, dot=False) + 4 * P.U * (1 + np.log(len(x)))) + 2 * P.U
        absx = np.abs(x).astype(np.float64)
        S = R.weights(q[:nq].astype(np.float64) @ x.astype(np.float64).T, beta, e)[0] @ absx
        bound = R.device_bound(q[:nq], x, "float16", beta, e, dot=False) * (1 + fold[:, None]) + fold[:, None] * S
        err = np.abs(mean.astype(np.float64) - want)
        assert (err[live] <= bound[live]).all(), (err[live] / bound[live]).max()
        assert (mean[~live] == 0).all() and np.isneginf(lp.log_z[~live]).all() and not np.isnan(mean).any()


# ---- refusals and empty cases ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    q, x = _int_case(65)
    s = q.astype(np.float64) @ x.astype(np.float64).T
    qd = _dev(q[:5])
    out = torch.full((2, 5), 123.0, device="cuda")
    out_mean = torch.full((5, 65), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(h, queries=qd, code=2, nq=5, beta=1.0, lab=None, n_lab=0, om=out[0], ol=out[1], mean=out_mean):
        return lib.vodhip_index_posterior_mean(h, None if queries is None else ptr(queries), code, nq, ctypes.c_float(beta),
                                               None if lab is None else ptr(lab), n_lab, None if om is None else ptr(om),
                                               None if ol is None else ptr(ol), None if mean is None else ptr(mean), None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x[:300], "float16") as ix:
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        refused(raw(ix._h, om=None), "invalid query / output pointers")
        refused(raw(ix._h, ol=None), "invalid query / output pointers")
        refused(raw(ix._h, mean=None), "invalid query / output pointers")
        refused(raw(ix._h, nq=-1), "invalid query / output pointers")
        refused(raw(ix._h, code=3), "invalid q_dtype 3")
        refused(raw(ix._h, code=-1), "invalid q_dtype -1")
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            refused(raw(ix._h, beta=beta), "beta must be finite and > 0")
        refused(raw(ix._h, lab=lab, n_lab=0), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=2), "set the row labels first")
        for bad in (0.0, -2.0, float("inf")):
            with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
                ix.posterior_mean(qd, temperature=bad)
        torch.cuda.synchronize()
        assert (out == 123.0).all() and (out_mean == 123.0).all()  # a refused call writes nothing
        assert raw(ix._h, queries=None, nq=0, om=None, ol=None, mean=None) == 0  # nq == 0: returns 0, needs nothing, writes nothing
        empty = ix.posterior_mean(torch.zeros((0, 65), device="cuda"))
        assert empty.mean.shape == (0, 65) and all(t.shape == (0,) for t in empty.log_partition)
        # after all that the index still searches, and the call still works
        sc, ids = ix.search(qd, 3)
        ref = np.sort(s[:5, :300], axis=1)[:, ::-1][:, :3]
        np.testing.assert_array_equal(sc.cpu().numpy(), ref.astype(np.float32))
        _check(_pm(ix, q[:5], 1.0), q[:5], x[:300], "float16", 1.0, what="after the refusals")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="L2 index"):
            ix.posterior_mean(qd)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            ix.posterior_mean(qd)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty index
        mean, log_z, m, r = _pm(ix, q[:5], 1.0)
        assert np.isneginf(m).all() and np.isneginf(r).all() and (mean == 0).all()
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        mean, lp = nx.posterior_mean(np.array(q[:5]))  # empty
        assert np.isneginf(lp.max_score).all() and (mean == 0).all()
        nx.add(x[:600].astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            nx.posterior_mean(np.array(q[:5]), temperature=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.posterior_mean(np.array(q[:5]), subset=np.zeros((5, 2), dtype=np.int32))
        assert nx.posterior_mean(np.zeros((0, 65), dtype=np.float32)).mean.shape == (0, 65)
        got = nx.posterior_mean(np.array(q[:5]))
        np.testing.assert_array_equal(got.log_partition.max_score, s[:5, :600].max(axis=1).astype(np.float32))
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.posterior_mean(np.array(q[:5]))
