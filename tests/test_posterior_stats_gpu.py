"""`HipFlatIndex.posterior_stats` / `HipNodeIndex.posterior_stats` and `log_z` with a tensor temperature on the GPU against the float64
restatement (tests/stats_ref.py).  Every word of every query is compared; the tolerance is the derived bound and nothing else.

Integer data (values in [-8, 8], every score exact in float32: the dot-product part of the bound is dropped): stores of 1, 255, 256, 257
and 3000 rows, widths 1, 64, 65, 768, batches 1, 64 (the 64-query kernel), 65, 129, 300 (the 128-query kernel), beta 1/64, 1, 4, fp16 and
bf16; `max_score` and `log_rel` are the bits `log_partition` returns.  The data sets are those of test_log_partition_gpu.py.

Then: stale rows behind `reset`, capacity above ntotal, NaN / -inf / +inf scores and no eligible row, batch independence and
repeatability (identical bits), 1024 identical rows, a two-valued store whose high score sits in one tile (every other tile is
re-centred), the finish's chunk edge (2049 tiles), subset labels, Gaussian data within the full bound and against `posterior_mean`,
`log_z` with a tensor temperature, the node index on 1, 2 and 3 shards, a call beside a search in flight, refusals and empty cases.
Measured shares of the bound (MI355X): DESIGN.md 5 and profiles/posterior_stats.json.
"""
import ctypes

import numpy as np
import pytest

import partition_ref as P
import posterior_ref as PM
import stats_ref as S
from l2_ref import round_store
from test_l2_cpu import GAUSS_CASES, gauss_case
from test_log_partition_gpu import _index, _int_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
STORES = [1, 255, 256, 257, 3000]
WIDTHS = [1, 64, 65, 768]
BATCHES = [1, 64, 65, 129, 300]
BETAS = [1.0 / 64.0, 1.0, 4.0]
NAMES = ("max_score", "log_rel", "mean_rel", "var")


def _words(r):
    """PosteriorStats -> the four library words and the three derived ones, as NumPy arrays"""
    lp = r.log_partition
    t = (lp.max_score, lp.log_rel, r.mean_rel, r.var_score, r.entropy, r.mean_score, lp.log_z)
    return tuple(a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in t)


def _ps(ix, q, beta=1.0, **kw):
    return _words(ix.posterior_stats(torch.from_numpy(np.array(q)).cuda(), temperature=1.0 / beta, **kw))


def _lp(ix, q, beta=1.0, **kw):
    r = ix.log_partition(torch.from_numpy(np.array(q)).cuda(), temperature=1.0 / beta, **kw)
    return r.max_score.cpu().numpy(), r.log_rel.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _check(got, ref, bounds, beta, what=""):
    """all four words of every query within their bounds of the float64 words `ref`; the derived words from the four; signs; the
    non-finite cases.  Prints the largest share of the bound per word."""
    m, r, a, v, h, ms, _ = got
    live = np.isfinite(ref[0])
    assert all(w.dtype == np.float32 for w in got)
    shares = []
    for name, g, want, b in zip(NAMES, (m, r, a, v), ref, bounds):
        err = np.abs(g[live].astype(np.float64) - want[live])
        ok = err <= b[live]
        share = float((err[b[live] > 0] / b[live][b[live] > 0]).max()) if (b[live] > 0).any() else 0.0
        shares.append(share)
        print(f"{what}: {name}: max err {err.max() if err.size else 0.0:.3e}, largest share of the bound {share:.4f}")
        assert ok.all(), (what, name, float(err.max()), float(b[live][~ok].min()))
    assert not np.signbit(r[live]).any() and (a[live] <= 0).all() and (v[live] >= 0).all()
    # the derived words are float32 arithmetic on the four
    b32 = np.float32(beta)
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(h[live], (r - b32 * a)[live])
        np.testing.assert_array_equal(ms[live], (m + a)[live])
    b_h = S.entropy_bound(beta, ref, bounds[1], bounds[2])
    assert (np.abs(h[live] - S.entropy(ref, beta)[live]) <= b_h[live]).all(), what
    assert (h[live] >= -b_h[live]).all()
    # no eligible row: (-inf, -inf, NaN, NaN); a +inf score: (+inf, +inf, NaN, NaN)
    dead = ~live
    np.testing.assert_array_equal(m[dead], ref[0][dead].astype(np.float32))
    np.testing.assert_array_equal(r[dead], ref[1][dead].astype(np.float32))
    assert np.isnan(a[dead]).all() and np.isnan(v[dead]).all() and np.isnan(h[dead]).all() and np.isnan(ms[dead]).all()
    return shares


def _check_int(got, s, beta, eligible=None, what="", node=False):
    """exact integer scores: max_score bit for bit, the other words within the bound without its dot-product part"""
    ref = S.from_scores(s, beta, eligible)
    n = s.shape[1] if eligible is None else eligible.sum(axis=1)
    bounds = S.bounds(np.zeros((len(ref[0]), 1)), None, None, beta, n, ref, dot=False, node=node)
    np.testing.assert_array_equal(got[0], ref[0].astype(np.float32), err_msg=what)
    return _check(got, ref, bounds, beta, what)


# ---- 1. sizes, widths, batches, betas, both dtypes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_widths_batches_and_betas(n, d, dtype):
    q, x, s = _int_case(d)
    x, s = x[:n], s[:, :n]
    with _index(x, dtype) as ix:
        full = {}
        for beta in BETAS:
            full[beta] = _ps(ix, q, beta)
            _check_int(full[beta], s, beta, what=f"int n {n} d {d} {dtype} beta {beta:g}")
            lp = _lp(ix, q, beta)
            assert _same_bits(full[beta][0], lp[0]) and _same_bits(full[beta][1], lp[1])  # the 128-query instantiation
        for nq in BATCHES[:-1]:
            beta = BETAS[nq % 3]
            got = _ps(ix, q[:nq], beta)
            for a, b in zip(got, full[beta]):
                assert _same_bits(a, b[:nq]), (nq, beta)
            lp = _lp(ix, q[:nq], beta)  # (nq 1 and 64: the 64-query instantiation)
            assert _same_bits(got[0], lp[0]) and _same_bits(got[1], lp[1])


# ---- 2. stale rows and non-finite scores -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_past_ntotal_are_never_counted(dtype):
    q, x, s = _int_case(65)
    with _index(x, dtype, capacity=3000) as ix:
        ix.reset()
        ix.add(x[2300:])  # 700 rows; rows 700 .. 2999 of the store still hold the first ingest
        assert ix.ntotal == 700
        _check_int(_ps(ix, q[:129], 1.0 / 64.0), s[:129, 2300:], 1.0 / 64.0, what=f"reset {dtype}")
    with _index(x[:700], dtype, capacity=3000) as ix:  # nothing beyond ntotal was ever written
        _check_int(_ps(ix, q[:129], 1.0 / 64.0), s[:129, :700], 1.0 / 64.0, what=f"capacity > ntotal {dtype}")
    with _index(x[:300], dtype, capacity=300) as ix:  # the last tile reaches past the capacity
        _check_int(_ps(ix, q[:65], 1.0), s[:65, :300], 1.0, what=f"tile padding {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_are_left_out_and_infinite_scores_and_no_row_give_the_stated_words(dtype):
    q, x, s = _int_case(65)
    q = np.array(q[:70])
    q[:, 0] = 1.0
    s = q.astype(np.float64) @ x.astype(np.float64).T
    xn = np.array(x)
    xn[7, 3] = np.nan      # every score of row 7 is NaN
    xn[300, 0] = -np.inf   # every score of row 300 is -inf: a term of 0, and no 0 * -inf
    keep = np.ones(len(x), dtype=bool)
    keep[[7, 300]] = False
    with _index(xn, dtype) as ix:
        for beta in (1.0 / 64.0, 1.0):
            got = _ps(ix, q, beta)
            assert not any(np.isnan(w).any() for w in got)
            _check_int(got, s[:, keep], beta, what=f"NaN row and -inf score {dtype} beta {beta:g}")
    with _index(np.repeat(xn[300:301], 300, axis=0), dtype) as ix:  # every score -inf: counts as no row
        m, r, a, v, h, ms, lz = _ps(ix, q, 1.0)
        assert np.isneginf(m).all() and np.isneginf(r).all() and np.isneginf(lz).all()
        assert np.isnan(a).all() and np.isnan(v).all() and np.isnan(h).all() and np.isnan(ms).all()
    xi = np.array(xn)
    xi[2999, 0] = np.inf   # +inf for every query (q[:, 0] = 1)
    with _index(xi, dtype) as ix:
        m, r, a, v, h, ms, lz = _ps(ix, q, 1.0)
    assert np.isposinf(m).all() and np.isposinf(r).all() and np.isposinf(lz).all()
    assert np.isnan(a).all() and np.isnan(v).all() and np.isnan(h).all() and np.isnan(ms).all()
    with _index(x[:0], dtype, capacity=8, dim=65) as ix:  # an empty index: no eligible row
        m, r, a, v, h, ms, lz = _ps(ix, q[:5], 1.0)
        assert np.isneginf(m).all() and np.isneginf(r).all() and np.isnan(a).all() and np.isnan(v).all()


# ---- 3. batch independence and repeatability ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 768])
def test_a_query_has_the_same_bits_in_any_batch_and_on_every_repeat(d, dtype):
    q, x, _ = _int_case(d)
    rng = np.random.default_rng(d)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)  # inexact sums: the order matters
    qg = (q + rng.standard_normal(q.shape)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(xg, dtype) as ix:
        a = _ps(ix, qg, beta)
        b = _ps(ix, qg, beta)
        c = _ps(ix, qg[:65], beta)
        for u, v, w in zip(a, b, c):
            assert _same_bits(u, v) and _same_bits(u[:65], w)
        for j in (0, 63, 64, 217, 299):
            one = _ps(ix, qg[j : j + 1], beta)  # (alone: the 64-query instantiation)
            for u, v in zip(a, one):
                assert _same_bits(u[j : j + 1], v), j
        assert (a[3] > 0).all() and (a[2] < 0).all()


# ---- 4. ties and re-centring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_1024_identical_rows_have_no_spread_and_entropy_log_1024(dtype):
    q, x, _ = _int_case(65)
    rows = np.repeat(x[:1], 1024, axis=0)
    with _index(rows, dtype) as ix:
        m, r, a, v, h, ms, _ = _ps(ix, q[:70], 4.0)
    np.testing.assert_array_equal(m, (q[:70].astype(np.float64) @ x[0].astype(np.float64)).astype(np.float32))
    assert (a == 0).all() and (v == 0).all() and not np.signbit(v).any()
    np.testing.assert_array_equal(ms, m)
    bound = P.device_bound(np.zeros((70, 1)), None, None, 4.0, 1024, dot=False)
    assert (np.abs(h.astype(np.float64) - np.log(1024.0)) <= bound).all(), np.abs(h - np.log(1024.0)).max()
    np.testing.assert_array_equal(h, r)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_high_score_in_one_tile_re_centres_every_other_tile(dtype):
    q, x, _ = _int_case(65)
    q = np.array(q[:70])
    q[:, 0] = 1.0
    rows = np.repeat(x[:1], 1200, axis=0)  # 5 tiles, the last one partial
    rows[800:810, 0] += 3.0                # tile 3 (rows 768 .. 1023): 10 rows score 3 higher for every query
    s = q.astype(np.float64) @ rows.astype(np.float64).T
    with _index(rows, dtype) as ix:
        for beta in BETAS:
            got = _check_int(_ps(ix, q, beta), s, beta, what=f"two-valued {dtype} beta {beta:g}")
    ref = S.from_scores(s, 1.0)
    p_low = 1190 * np.exp(-3.0) / (10 + 1190 * np.exp(-3.0))
    np.testing.assert_allclose(ref[2], -3.0 * p_low, rtol=1e-12)  # (the restatement against the closed form)
    np.testing.assert_allclose(ref[3], 9.0 * p_low * (1 - p_low), rtol=1e-12)


# ---- 5. the finish's chunk edge ------------------------------------------------------------------------------------------------------------
def test_2049_tiles_cross_the_finish_chunk_edge():
    n, d, nq = 524289, 64, 3  # 2049 tiles: two whole chunks of the finish and one tile; the last tile holds one row
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    s = q.astype(np.float64) @ x.astype(np.float64).T
    with _index(x, "float16") as ix:
        for beta in (1.0 / 64.0, 1.0):
            got = _ps(ix, q, beta)
            _check_int(got, s, beta, what=f"2049 tiles beta {beta:g}")
            lp = _lp(ix, q, beta)
            assert _same_bits(got[0], lp[0]) and _same_bits(got[1], lp[1])


# ---- 6. subset labels ----------------------------------------------------------------------------------------------------------------------
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
            got = _ps(ix, q[:nq], beta, subset=sub)
            _check_int(got, s[:nq], beta, elig, what=f"subset nq {nq} {dtype} beta {beta:g}")
            assert np.isneginf(got[0][3::4]).all() and np.isnan(got[2][3::4]).all() and not np.isnan(got[2][:3]).any()
            lp = _lp(ix, q[:nq], beta, subset=sub)
            assert _same_bits(got[0], lp[0]) and _same_bits(got[1], lp[1])
        # row labels set but no query labels given: unrestricted
        _check_int(_ps(ix, q[:nq], 1.0), s[:nq], 1.0, what="row labels without query labels")


# ---- 7. Gaussian data: the full bound, every query -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    beta = float(np.float32(1.0 / np.sqrt(dim)))  # the float32 the call receives
    ref = S.posterior_stats(q, x, dtype, beta)
    bounds = S.bounds(q, x, dtype, beta, len(x), ref)
    qd = torch.from_numpy(q).cuda()
    with _index(x, dtype) as ix:
        got = _ps(ix, q, beta)
        mean = ix.posterior_mean(qd, temperature=1.0 / beta).mean.cpu().numpy().astype(np.float64)
    _check(got, ref, bounds, beta, what=f"gaussian dim {dim} {dtype}")
    # E_p[s] = <q~, E_p[x~]>: the one-scan word against the two-scan route, within the sum of the two derived bounds
    qr = round_store(q, dtype)
    route = (qr * mean).sum(axis=1)
    b_route = (np.abs(qr) * PM.device_bound(q, x, dtype, beta)).sum(axis=1)
    b_ms = S.mean_score_bound(ref, bounds[0], bounds[2])
    err = np.abs(got[5].astype(np.float64) - route)
    print(f"gaussian dim {dim} {dtype}: max |mean_score - <q~, mean>| = {err.max():.3e}, bounds >= {b_ms.min():.3e} + {b_route.min():.3e}")
    assert (err <= b_ms + b_route).all()


# ---- 8. the temperature gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES[:2])
def test_log_z_with_a_tensor_temperature(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    t0 = np.float32(np.sqrt(dim))
    beta = float(np.float32(1.0 / float(t0)))
    ref = S.posterior_stats(q, x, dtype, beta)
    bounds = S.bounds(q, x, dtype, beta, len(x), ref)
    w = np.random.default_rng(seed).standard_normal(len(q)).astype(np.float32)
    wd = torch.from_numpy(w).cuda()
    with _index(x, dtype) as ix:
        calls = []
        real_mean = ix.posterior_mean
        ix.posterior_mean = lambda *a, **k: (calls.append(1), real_mean(*a, **k))[1]
        # the float path
        q0 = torch.from_numpy(q).cuda().requires_grad_(True)
        out0 = ix.log_z(q0, float(t0))
        (out0 * wd).sum().backward()
        # T and q
        q1 = torch.from_numpy(q).cuda().requires_grad_(True)
        t1 = torch.tensor([float(t0)], device="cuda", requires_grad=True)
        out1 = ix.log_z(q1, t1)
        (out1 * wd).sum().backward()
        assert torch.equal(out1.view(torch.int32), out0.view(torch.int32))
        assert torch.equal(q1.grad.view(torch.int32), q0.grad.view(torch.int32))  # the query gradient: the float path's bits
        # T alone: no posterior_mean call
        n_calls = len(calls)
        t2 = torch.tensor(float(t0), requires_grad=True)  # (0-d, on the host)
        out2 = ix.log_z(torch.from_numpy(q).cuda(), t2)
        (out2 * wd).sum().backward()
        assert len(calls) == n_calls
        assert torch.equal(out2.view(torch.int32), out0.view(torch.int32))
    # grad_T = -sum_q w_q E_p[s] / T^2: every query's mean_score within its bound, the float64 sum, the float32 rounding of the result
    want = -(w.astype(np.float64) * S.mean_score(ref)).sum() / float(t0) ** 2
    tol = (np.abs(w).astype(np.float64) * S.mean_score_bound(ref, bounds[0], bounds[2])).sum() / float(t0) ** 2
    tol = tol + P.U * (abs(want) + tol)
    for t in (t1, t2):
        got = float(t.grad.reshape(()).cpu())
        print(f"grad_T dim {dim} {dtype}: {got:.6e}, float64 {want:.6e}, |err| {abs(got - want):.3e}, tol {tol:.3e}")
        assert t.grad.shape == t.shape and t.grad.dtype == torch.float32 and t.grad.device == t.device
        assert abs(got - want) <= tol


# ---- 9. node index ---------------------------------------------------------------------------------------------------------------------------
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
        flat = _ps(ix, q[:nq], beta)
    with HipNodeIndex(65, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        nx.add(x.astype(np.float32))
        got = _words(nx.posterior_stats(np.array(q[:nq]), temperature=1.0 / beta))
        lp = nx.log_partition(np.array(q[:nq]), temperature=1.0 / beta)
        nx.set_row_labels(labels)
        got_sub = _words(nx.posterior_stats(np.array(q[:nq]), temperature=1.0 / beta, subset=sub))
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (nq,) for a in got + got_sub)
    assert _same_bits(got[0], flat[0])                                      # max_score: the flat index's bits
    assert _same_bits(got[0], lp.max_score) and _same_bits(got[1], lp.log_rel)  # the pair: the node log_partition's bits
    _check_int(got, s[:nq], beta, what=f"node {n_shards} shards", node=True)
    _check_int(got_sub, s[:nq], beta, elig, what=f"node {n_shards} shards, subset", node=True)


# ---- 10. beside searches, refusals, empty cases ------------------------------------------------------------------------------------------------
def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x, _ = _int_case(768)
    qd = torch.from_numpy(np.array(q[:129])).cuda()
    with _index(x, "float16") as ix:
        serial_s, serial_i = ix.search(qd, 100)
        serial = _words(ix.posterior_stats(qd, temperature=64.0))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            st = ix.posterior_stats(qd, temperature=64.0)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        for a, b in zip(_words(st), serial):
            assert _same_bits(a, b)
        assert ix.get_stat("last_overflow") == 0


def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    q, x, s = _int_case(65)
    qd = torch.from_numpy(np.array(q[:5])).cuda()
    out = torch.full((4, 5), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(h, queries=qd, code=2, nq=5, beta=1.0, lab=None, n_lab=0, outs=(out[0], out[1], out[2], out[3])):
        return lib.vodhip_index_posterior_stats(h, None if queries is None else ptr(queries), code, nq, ctypes.c_float(beta),
                                                None if lab is None else ptr(lab), n_lab, *[None if o is None else ptr(o) for o in outs], None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x[:300], "float16") as ix:
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        for k in range(4):  # each NULL output
            refused(raw(ix._h, outs=tuple(None if j == k else out[j] for j in range(4))), "invalid query / output pointers")
        refused(raw(ix._h, nq=-1), "invalid query / output pointers")
        refused(raw(ix._h, code=3), "invalid q_dtype 3")
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            refused(raw(ix._h, beta=beta), "beta must be finite and > 0")
        refused(raw(ix._h, lab=lab, n_lab=0), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=2), "set the row labels first")
        for bad in (0.0, -2.0, float("inf")):
            with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
                ix.posterior_stats(qd, temperature=bad)
        torch.cuda.synchronize()
        assert (out == 123.0).all()  # a refused call writes nothing
        assert raw(ix._h, queries=None, nq=0, outs=(None,) * 4) == 0  # nq == 0: returns 0, needs nothing, writes nothing
        empty = ix.posterior_stats(torch.zeros((0, 65), device="cuda"))
        assert all(t.shape == (0,) for t in empty[:4]) and all(t.shape == (0,) for t in empty.log_partition)
        # `out`: the four words land in the caller's tensors
        mine = tuple(torch.empty(5, device="cuda") for _ in range(4))
        st = ix.posterior_stats(qd, out=mine)
        assert st.mean_rel is mine[2] and st.var_score is mine[3] and st.log_partition.max_score is mine[0]
        # after all that the index still searches, and the call still works
        sc, _ = ix.search(qd, 3)
        np.testing.assert_array_equal(sc.cpu().numpy(), np.sort(s[:5, :300], axis=1)[:, ::-1][:, :3].astype(np.float32))
        _check_int(_ps(ix, q[:5], 1.0), s[:5, :300], 1.0, what="after the refusals")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="posterior_stats is not supported on an L2 index"):
            ix.posterior_stats(qd)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            ix.posterior_stats(qd)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        e = nx.posterior_stats(np.array(q[:5]))  # empty
        assert np.isneginf(e.log_partition.max_score).all() and np.isnan(e.mean_rel).all() and np.isnan(e.var_score).all() and np.isnan(e.entropy).all()
        nx.add(x[:600].astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            nx.posterior_stats(np.array(q[:5]), temperature=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.posterior_stats(np.array(q[:5]), subset=np.zeros((5, 2), dtype=np.int32))
        assert nx.posterior_stats(np.zeros((0, 65), dtype=np.float32)).mean_rel.shape == (0,)
        _check_int(_words(nx.posterior_stats(np.array(q[:5]))), s[:5, :600], 1.0, what="node after the refusals", node=True)
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.posterior_stats(np.array(q[:5]))
