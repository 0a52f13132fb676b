"""`HipFlatIndex.log_partition` / `HipNodeIndex.log_partition` on the GPU against the float64 restatement (tests/partition_ref.py).

Integer data (values in [-8, 8]: exact in fp16 and bf16, every score an exact integer in float32): `max_score` must equal the score of
`search(q, 1)` bit for bit and `log_rel` must be within `partition_ref.device_bound` with its dot-product part set to zero; stores of 1, 5,
255, 256, 257 (one tile, the tile edge, two tiles), 1500 and 3000 rows, widths 1, 64, 65, 765, 768, batches 1, 64 (the 64-query kernel),
65, 129, 300 (the 128-query kernel, one to three query tiles), beta 1, 1/64 and 4 - at dim 768 exp(beta s) overflows float32 by thousands
of orders at beta 1 and 4, so only the max-stabilised form passes; at 1/64 thousands of rows contribute.  One data set per width (300
queries, 3000 rows): a smaller store or batch is its first rows.

Then: stale rows behind `reset`, a capacity larger than ntotal, batch independence and repeatability (identical bits), 1024 tied rows,
subset labels, NaN / +inf / -inf scores, Gaussian data within the full derived bound (every query), `topk_log_coverage` behind a search,
a call between `search_async` and `finish` on another stream, the node index on 1, 2 and 3 shards of device 0, refusals and empty cases.
Measured maxima (MI355X): see DESIGN.md 4 "Log-partition scan" and profiles/log_partition.json.
"""
import ctypes
import functools

import numpy as np
import pytest

import partition_ref as P
from test_l2_cpu import GAUSS_CASES, gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
STORES = [1, 5, 255, 256, 257, 1500, 3000]
WIDTHS = [1, 64, 65, 765, 768]
BATCHES = [1, 64, 65, 129, 300]
BETAS = [1.0, 1.0 / 64.0, 4.0]


def _index(x, dtype="float16", capacity=None, dim=None, **kw):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, **kw)
    if len(x):
        ix.add(x)
    return ix


@functools.lru_cache(maxsize=None)
def _int_case(d, n=3000, nq=300):
    """integer rows / queries and their exact scores; the same for both store dtypes (both hold the values exactly)"""
    rng = np.random.default_rng(4000 + d)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    s = q.astype(np.float64) @ x.astype(np.float64).T
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)  # every score is exact in float32
    for a in (q, x, s):
        a.setflags(write=False)
    return q, x, s


def _lp(ix, q, beta=1.0, **kw):
    r = ix.log_partition(torch.from_numpy(np.array(q)).cuda(), temperature=1.0 / beta, **kw)
    return tuple(t.cpu().numpy() for t in r)


def _check_int(got, s, beta, eligible=None, what=""):
    """exact integer scores: max_score bit for bit, log_rel within the bound without its dot-product part, log_rel >= 0 bitwise"""
    log_z, m, r = got
    rm, rr = P.from_scores(s, beta, eligible)
    n = s.shape[1] if eligible is None else eligible.sum(axis=1)
    bound = P.device_bound(np.zeros((len(rm), 1)), None, None, beta, n, dot=False)
    assert m.dtype == np.float32 and r.dtype == np.float32 and log_z.dtype == np.float32
    np.testing.assert_array_equal(m, rm.astype(np.float32), err_msg=what)
    live = np.isfinite(rm)
    err = np.abs(r[live].astype(np.float64) - rr[live])
    print(f"{what}: max |log_rel - float64| = {err.max() if err.size else 0.0:.3e}, bound >= {bound[live].min() if err.size else 0.0:.3e}")
    assert (err <= bound[live]).all(), (what, err.max(), bound[live].min())
    assert not np.signbit(r[live]).any()
    assert np.isneginf(r[~live]).all() and np.isneginf(log_z[~live]).all()
    mb, want_z = (m.astype(np.float64) * beta)[live], (m.astype(np.float64) * beta + r)[live]  # log_z: one float32 product, one sum
    assert (np.abs(log_z[live] - want_z) <= np.spacing(np.abs(mb).astype(np.float32)) + np.spacing(np.abs(want_z).astype(np.float32))).all()


# ---- bit checks and edges on integer data -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_widths_batches_and_betas(n, d, dtype):
    q, x, s = _int_case(d)
    x, s = x[:n], s[:, :n]
    with _index(x, dtype) as ix:
        top1 = ix.search(torch.from_numpy(np.array(q)).cuda(), 1)[0].cpu().numpy()[:, 0]
        full = {}
        for beta in BETAS:
            full[beta] = _lp(ix, q, beta)
            _check_int(full[beta], s, beta, what=f"n {n} d {d} {dtype} beta {beta:g}")
            assert np.array_equal(full[beta][1].view(np.uint32), top1.view(np.uint32))  # the bits search(q, 1) returns
        for nq in BATCHES[:-1]:
            for beta in (BETAS[nq % 3],):
                got = _lp(ix, q[:nq], beta)
                for a, b in zip(got, full[beta]):
                    assert np.array_equal(a.view(np.uint32), b[:nq].view(np.uint32)), (nq, beta)


# ---- stale rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_past_ntotal_are_never_counted(dtype):
    q, x, s = _int_case(65)
    with _index(x, dtype, capacity=3000) as ix:
        ix.reset()
        ix.add(x[2300:])  # 700 rows; rows 700 .. 2999 of the store still hold the first ingest
        assert ix.ntotal == 700
        _check_int(_lp(ix, q[:129], 1.0 / 64.0), s[:129, 2300:], 1.0 / 64.0, what=f"reset {dtype}")
    with _index(x[:700], dtype, capacity=3000) as ix:  # nothing beyond ntotal was ever written
        _check_int(_lp(ix, q[:129], 1.0 / 64.0), s[:129, :700], 1.0 / 64.0, what=f"capacity > ntotal {dtype}")
    with _index(x[:300], dtype, capacity=300) as ix:  # the last tile reaches past the capacity
        _check_int(_lp(ix, q[:65], 1.0), s[:65, :300], 1.0, what=f"tile padding {dtype}")


# ---- batch independence and repeatability --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 768])
def test_a_query_has_the_same_bits_in_any_batch_and_on_every_repeat(d, dtype):
    q, x, _ = _int_case(d)
    rng = np.random.default_rng(d)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)  # inexact sums: the order matters
    qg = (q + rng.standard_normal(q.shape)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(xg, dtype) as ix:
        a = _lp(ix, qg, beta)
        b = _lp(ix, qg, beta)
        c = _lp(ix, qg[:65], beta)
        for u, v, w in zip(a, b, c):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
            assert np.array_equal(u[:65].view(np.uint32), w.view(np.uint32))
        for j in (0, 63, 64, 217, 299):
            one = _lp(ix, qg[j : j + 1], beta)
            for u, v in zip(a, one):
                assert u[j : j + 1].view(np.uint32) == v.view(np.uint32), j


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_1024_identical_rows_give_log_1024(dtype):
    q, x, _ = _int_case(65)
    rows = np.repeat(x[:1], 1024, axis=0)
    with _index(rows, dtype) as ix:
        _, m, r = _lp(ix, q[:70], 4.0)
    np.testing.assert_array_equal(m, (q[:70].astype(np.float64) @ x[0].astype(np.float64)).astype(np.float32))
    # every term is exp(0) = 1 and the sums 256, 512, .. are exact: what is left is logf's 1 ulp and the rounding of log(1024) itself
    want = np.log(1024.0)
    assert (np.abs(r.astype(np.float64) - want) <= 1.5 * np.spacing(np.float32(want))).all(), np.abs(r - want).max()


# ---- subset labels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 132])
def test_subset_labels(nq, dtype):
    q, x, s = _int_case(65)
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        for beta in (1.0, 1.0 / 64.0):
            got = _lp(ix, q[:nq], beta, subset=sub)
            _check_int(got, s[:nq], beta, elig, what=f"subset nq {nq} {dtype} beta {beta:g}")
            assert np.isneginf(got[0][3::4]).all() and np.isneginf(got[1][3::4]).all() and np.isneginf(got[2][3::4]).all()
            assert not np.isnan(got[0]).any()
        # row labels set but no query labels given: unrestricted
        _check_int(_lp(ix, q[:nq], 1.0), s[:nq], 1.0, what="row labels without query labels")


# ---- non-finite scores -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_are_left_out_and_an_infinite_score_gives_infinity(dtype):
    q, x, s = _int_case(65)
    q = np.array(q[:70])
    q[:, 0] = 1.0
    s = q.astype(np.float64) @ x.astype(np.float64).T
    xn = np.array(x)
    xn[7, 3] = np.nan      # every score of row 7 is NaN
    xn[300, 0] = -np.inf   # every score of row 300 is -inf: a term of 0
    keep = np.ones(len(x), dtype=bool)
    keep[[7, 300]] = False
    with _index(xn, dtype) as ix:
        _check_int(_lp(ix, q, 1.0 / 64.0), s[:, keep], 1.0 / 64.0, what=f"NaN row {dtype}")
    xi = np.array(xn)
    xi[2999, 0] = np.inf   # +inf for every query (q[:, 0] = 1)
    with _index(xi, dtype) as ix:
        log_z, m, r = _lp(ix, q, 1.0)
    assert np.isposinf(m).all() and np.isposinf(r).all() and np.isposinf(log_z).all()


# ---- Gaussian data: the full bound, every query ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    beta = float(np.float32(1.0 / np.sqrt(dim)))  # the float32 the call receives
    rm, rr = P.log_partition(q, x, dtype, beta)
    with _index(x, dtype) as ix:
        _, m, r = _lp(ix, q, beta)
    err_r, err_m = np.abs(r - rr), np.abs(m - rm)
    bound_r, bound_m = P.device_bound(q, x, dtype, beta, len(x)), P.max_bound(q, x, dtype)
    print(f"dim {dim} {dtype}: max |log_rel - float64| = {err_r.max():.3e} (bound >= {bound_r.min():.3e}), "
          f"max |max_score - float64| = {err_m.max():.3e} (bound >= {bound_m.min():.3e})")
    assert (err_r <= bound_r).all() and (err_m <= bound_m).all()
    assert not np.signbit(r).any()


# ---- coverage of a top-k list ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_topk_log_coverage_behind_a_search(dtype):
    from vod_amd.index import topk_log_coverage

    q, x, s = _int_case(65)
    T, k = 64.0, 100
    u = P.U
    # torch's side, k float32 terms: (s - max) / T rounds once (|t| <= 104 matters), expf and logf within 2 ulp, k - 1 additions
    torch_side = lambda kk: (104 + 4 + kk) * u * 1.01 + 4 * u * np.log(kk)  # noqa: E731
    for n in (3000, 60):
        with _index(x[:n], dtype) as ix:
            qd = torch.from_numpy(np.array(q[:129])).cuda()
            scores, _ = ix.search(qd, k)
            lp = ix.log_partition(qd, temperature=T)
            cov = topk_log_coverage(scores, lp, T)
            assert cov.is_cuda and cov.dtype == torch.float32
            cov = cov.cpu().numpy().astype(np.float64)
        tol = P.device_bound(np.zeros((129, 1)), None, None, 1 / T, n, dot=False) + torch_side(min(k, n))
        ref = P.coverage(s[:129, :n], k, 1 / T)
        print(f"n {n} {dtype}: coverage in [{cov.min():.4f}, {cov.max():.4f}], max |cov - float64| = {np.abs(cov - ref).max():.3e}, tol {tol.min():.3e}")
        assert (cov <= tol).all()
        assert (np.abs(cov - ref) <= tol).all()
        if n <= k:
            assert (np.abs(cov) <= tol).all()  # the list is the whole store
        else:
            assert (cov < 0).all()


# ---- beside searches -------------------------------------------------------------------------------------------------------------------
def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x, _ = _int_case(768)
    qd = torch.from_numpy(np.array(q[:129])).cuda()
    with _index(x, "float16") as ix:
        serial_s, serial_i = ix.search(qd, 100)
        serial_lp = ix.log_partition(qd, temperature=64.0)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            lp = ix.log_partition(qd, temperature=64.0)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        for a, b in zip(lp, serial_lp):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert ix.get_stat("last_overflow") == 0


# ---- node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards,capacity", [(1, 3000), (2, 3000), (3, 3000), (3, 12000)])
def test_node_index_folds_the_shards(n_shards, capacity):
    from vod_amd.index import HipNodeIndex

    q, x, s = _int_case(65)
    nq, beta = 129, 1.0 / 64.0
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, "float16") as ix:
        flat = _lp(ix, q[:nq], beta)
        ix.set_row_labels(labels)
        flat_sub = _lp(ix, q[:nq], beta, subset=sub)
    with HipNodeIndex(65, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        nx.add(x.astype(np.float32))
        got = nx.log_partition(np.array(q[:nq]), temperature=1.0 / beta)
        nx.set_row_labels(labels)
        got_sub = nx.log_partition(np.array(q[:nq]), temperature=1.0 / beta, subset=sub)
    fold = 4 * P.U * (1 + np.log(len(x)))  # the fold's float32 rounding of log_rel (the sum runs in double) on top of the shards' own
    for res, ref, e in ((got, flat, None), (got_sub, flat_sub, elig)):
        assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (nq,) for a in res)
        assert np.array_equal(res[1].view(np.uint32), ref[1].view(np.uint32))  # max_score: the flat index's bits
        rm, rr = P.from_scores(s[:nq], beta, e)
        n = len(x) if e is None else e.sum(axis=1)
        bound = P.device_bound(np.zeros((nq, 1)), None, None, beta, n, dot=False) + fold
        live = np.isfinite(rm)
        assert (np.abs(res[2][live] - rr[live]) <= bound[live]).all()
        assert np.isneginf(res[2][~live]).all() and np.isneginf(res[0][~live]).all() and not np.isnan(res[0]).any()


# ---- refusals and empty cases ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    q, x, s = _int_case(65)
    qd = torch.from_numpy(np.array(q[:5])).cuda()
    out = torch.full((2, 5), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(h, queries=qd, code=2, nq=5, beta=1.0, lab=None, n_lab=0, om=out[0], ol=out[1]):
        return lib.vodhip_index_log_partition(h, None if queries is None else ptr(queries), code, nq, ctypes.c_float(beta),
                                              None if lab is None else ptr(lab), n_lab, None if om is None else ptr(om),
                                              None if ol is None else ptr(ol), None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x[:300], "float16") as ix:
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        refused(raw(ix._h, om=None), "invalid query / output pointers")
        refused(raw(ix._h, ol=None), "invalid query / output pointers")
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
                ix.log_partition(qd, temperature=bad)
        torch.cuda.synchronize()
        assert (out == 123.0).all()  # a refused call writes nothing
        assert raw(ix._h, queries=None, nq=0, om=None, ol=None) == 0  # nq == 0: returns 0, needs nothing, writes nothing
        empty = ix.log_partition(torch.zeros((0, 65), device="cuda"))
        assert all(t.shape == (0,) for t in empty)
        # after all that the index still searches, and the call still works
        sc, ids = ix.search(qd, 3)
        ref = np.sort(s[:5, :300], axis=1)[:, ::-1][:, :3]
        np.testing.assert_array_equal(sc.cpu().numpy(), ref.astype(np.float32))
        _check_int(_lp(ix, q[:5], 1.0), s[:5, :300], 1.0, what="after the refusals")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="L2 index"):
            ix.log_partition(qd)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            ix.log_partition(qd)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty index
        log_z, m, r = _lp(ix, q[:5], 1.0)
        assert np.isneginf(m).all() and np.isneginf(r).all() and np.isneginf(log_z).all()
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        log_z, m, r = nx.log_partition(np.array(q[:5]))  # empty
        assert np.isneginf(m).all() and np.isneginf(r).all() and np.isneginf(log_z).all()
        nx.add(x[:600].astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            nx.log_partition(np.array(q[:5]), temperature=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.log_partition(np.array(q[:5]), subset=np.zeros((5, 2), dtype=np.int32))
        assert nx.log_partition(np.zeros((0, 65), dtype=np.float32)).max_score.shape == (0,)
        got = nx.log_partition(np.array(q[:5]))
        np.testing.assert_array_equal(got.max_score, s[:5, :600].max(axis=1).astype(np.float32))
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.log_partition(np.array(q[:5]))
