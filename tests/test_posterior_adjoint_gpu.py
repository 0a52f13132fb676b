"""`posterior_adjoint` / `row_mass` / `read_out` of both indexes on the GPU against the float64 restatement
(tests/readout_adjoint_ref.py); every element of every case is compared against `readout_adjoint_ref.device_bound`, which is derived,
not fitted, and the worst err / bound is printed.

Integer data (rows and queries in [-8, 8], W integers in [-4, 4] times 2^-10: everything exact in fp16 and bf16, every score an exact
integer in float32, so the bound's dot-product part is dropped): stores of 1, 63, 64, 65, 511, 513 and 1029 rows (the edges of a 64-row
workgroup, 8 / 9 workgroups across the XCD padding), batches of 1, 64, 255, 256, 257, 513 (the 256-query tile edges) and 1024 + 65 (a
second slice adds), widths 1, 64, 65, 129, 193, 256 (every NSL), dims 1, 64, 65, 129, 768, beta 1, 1/64, 4, both store dtypes.  Then
masked positions and dead queries, reproducibility, subset labels, the non-finite contract, the column scaling, identities on the
device, Gaussian data within the full bound, autograd through `read_out`, the node index, refusals.
Measured maxima (MI355X): DESIGN.md 4 "Read-out adjoint" and profiles/posterior_adjoint.json.
"""
import ctypes
import functools

import numpy as np
import pytest

import partition_ref as P
import posterior_ref as PM
import readout_adjoint_ref as A
import readout_grad_ref as G
import readout_ref as R
from test_l2_cpu import GAUSS_CASES, gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
STORES = [1, 63, 64, 65, 511, 513, 1029]
BATCHES = [1, 64, 255, 256, 257, 513, 1024 + 65]
WIDTHS = [1, 64, 65, 129, 193, 256]
DIMS = [1, 64, 65, 129, 768]
BETAS = [1.0, 1.0 / 64.0, 4.0]
N_MAX, NQ_MAX = 1029, 1024 + 65


def _index(x, dtype="float16", capacity=None, dim=None, **kw):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, **kw)
    if len(x):
        ix.add(x)
    return ix


@functools.lru_cache(maxsize=None)
def _int_case(d, n=N_MAX, nq=NQ_MAX):
    """integer rows / queries / table and a 16-bit-exact W; the same for both store dtypes"""
    rng = np.random.default_rng(9000 + d + n)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    v = rng.integers(-8, 9, size=(n, 256)).astype(np.float32)
    w = (rng.integers(-4, 5, size=(nq, 256)) * 2.0 ** -10).astype(np.float32)
    for a in (q, x, v, w):
        a.setflags(write=False)
    return q, x, v, w


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _adj(ix, q, w, beta=1.0, lp=None, **kw):
    """the adjoint as NumPy float32 [ntotal, n_cols], and the forward words it was given"""
    qd = _dev(q)
    sub = kw.get("subset")
    lp = ix.log_partition(qd, temperature=1.0 / beta, subset=sub) if lp is None else lp
    out = ix.posterior_adjoint(qd, _dev(w), lp, temperature=1.0 / beta, **kw)
    n_cols = 1 if np.ndim(w) == 1 else np.shape(w)[1]
    assert out.dtype == torch.float32 and out.shape == (ix.ntotal, n_cols) and out.is_cuda
    return out.cpu().numpy(), lp


def _check(got, q, x, w, dtype, beta, eligible=None, dot=False, what="", **kw):
    """every (row, column) within the derived bound"""
    ref, _, _ = A.posterior_adjoint(q, x, w, dtype, beta, eligible)
    bound = A.device_bound(q, x, w, dtype, beta, eligible, dot=dot, **kw)
    assert got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max() if err.size else 0.0
    print(f"{what}: max |adjoint - float64| = {err.max() if err.size else 0.0:.3e}, max err / bound = {ratio:.3e}")
    assert not np.isnan(err).any(), what
    assert (err <= bound).all(), (what, ratio)
    return ratio


def _bits_equal(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# ---- sizes, batches, widths, dims, betas on integer data ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_with_every_width(n, dtype):
    i = STORES.index(n)
    d = DIMS[i % 5]
    q, x, _, w = _int_case(d)
    x = x[:n]
    with _index(x, dtype) as ix:
        for k, c in enumerate(WIDTHS):
            beta, nq = BETAS[(k + i) % 3], BATCHES[(k + i) % 6]
            got, _ = _adj(ix, q[:nq], w[:nq, :c], beta)
            _check(got, q[:nq], x, w[:nq, :c], dtype, beta, what=f"n {n} d {d} w {c} nq {nq} {dtype} beta {beta:g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", BATCHES)
def test_batch_sizes_across_the_query_tile_and_the_slice(nq, dtype):
    i = BATCHES.index(nq)
    d = DIMS[(i + 2) % 5]
    q, x, _, w = _int_case(d)
    with _index(x, dtype) as ix:  # 1029 rows: 17 workgroups, 24 launched
        for k in range(2):
            c, beta = WIDTHS[(2 * i + k) % 6], BETAS[(i + k) % 3]
            got, _ = _adj(ix, q[:nq], w[:nq, :c], beta)
            _check(got, q[:nq], x, w[:nq, :c], dtype, beta, what=f"nq {nq} d {d} w {c} {dtype} beta {beta:g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_dims_with_every_beta(d, dtype):
    i = DIMS.index(d)
    q, x, _, w = _int_case(d)
    x, q = x[:513], q[:257]
    with _index(x, dtype) as ix:
        for k, beta in enumerate(BETAS):
            c = WIDTHS[(i + 2 * k) % 6]
            got, _ = _adj(ix, q, w[:257, :c], beta)
            _check(got, q, x, w[:257, :c], dtype, beta, what=f"d {d} w {c} {dtype} beta {beta:g}")


# ---- masked positions and dead queries -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_past_ntotal_never_leak(dtype):
    q, x, _, w = _int_case(65)
    q, w = q[:257], w[:257, :65]
    stale = np.array(x[:600]) * 4  # larger scores than any live row: a leak would dominate
    stale[130:256:3] = np.nan      # and NaN among the stale rows of the last live tile
    canary = 123.0
    with _index(stale, dtype, capacity=600) as ix:
        ix.reset()
        ix.add(x[:130])
        assert ix.ntotal == 130
        buf = torch.full((131, 65), canary, device="cuda")
        lp = ix.log_partition(_dev(q), temperature=64.0)
        out = ix.posterior_adjoint(_dev(q), _dev(w), lp, temperature=64.0, out=buf[:130])
        assert out.shape == (130, 65) and out.data_ptr() == buf.data_ptr()
        torch.cuda.synchronize()
        assert (buf[130] == canary).all()  # the row behind `out` is untouched
        _check(buf[:130].cpu().numpy(), q, x[:130], w, dtype, 1.0 / 64.0, what=f"stale rows past ntotal {dtype}")
        got, _ = _adj(ix, q, w, 1.0 / 64.0)
        assert got.shape == (130, 65)
        _bits_equal(got, buf[:130].cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_stored_row_with_a_nan_component_weighs_nothing(dtype):
    q, x, _, w = _int_case(65)
    q, w = q[:130], w[:130, :70]
    xn = np.array(x[:300])
    xn[[7, 64, 299], 3] = np.nan
    with _index(xn, dtype) as ix:
        got, _ = _adj(ix, q, w, 1.0 / 64.0)
    assert (got[[7, 64, 299]].view(np.uint32) == 0).all() and np.isfinite(got).all()
    _check(got, q, xn, w, dtype, 1.0 / 64.0, what=f"NaN rows {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dead_queries_contribute_nothing(dtype):
    q, x, _, w = _int_case(65)
    x, w = x[:300], w[:, :70]
    beta = 1.0 / 64.0
    # (a) dead by labels: every fourth query asks for a label no row has
    labels = (np.arange(len(x)) % 3).astype(np.int32)
    nq = 130
    sub = np.where(np.arange(nq)[:, None] % 4 == 3, 9, -1).astype(np.int32)
    elig = np.broadcast_to((np.arange(nq) % 4 != 3)[:, None], (nq, len(x)))
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        got, lp = _adj(ix, q[:nq], w[:nq], beta, subset=sub)
        assert torch.isneginf(lp.max_score[3::4]).all()
        _check(got, q[:nq], x, w[:nq], dtype, beta, elig, what=f"dead by labels {dtype}")
        # dead queries appended behind the batch, with any W that leaves the column exponents alone: not one bit moves
        more = 200
        sub2 = np.concatenate([sub, np.full((more, 1), 9, dtype=np.int32)])
        got2, lp2 = _adj(ix, q[: nq + more], w[: nq + more], beta, subset=sub2)
        assert torch.isneginf(lp2.max_score[nq:]).all()
        _bits_equal(got2, got)
    # (b) dead by a +inf score: row 5 holds +inf in column 0; a query with a positive entry there scores +inf
    xi = np.array(x)
    xi[5, 0] = np.inf
    with _index(xi, dtype) as ix:
        got, lp = _adj(ix, q[:nq], w[:nq], beta)
    dead = q[:nq, 0] > 0
    assert dead.any() and (~dead).any() and torch.equal(torch.isposinf(lp.max_score).cpu(), torch.from_numpy(dead))
    assert np.isfinite(got).all() and (got[5].view(np.uint32) == 0).all()
    # the reference rounds with saturation (an infinity becomes the largest finite value), so the case is restated for it: the queries
    # that score +inf are dead, and row 5 weighs nothing for the others (a score of -inf, or 0 * inf = NaN)
    elig = np.broadcast_to(~dead[:, None], (nq, len(x))) & (np.arange(len(x)) != 5)[None, :]
    _check(got, q[:nq], x, w[:nq], dtype, beta, elig, what=f"dead by a +inf score {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,more", [(100, 30), (250, 50), (1000, 89)])
def test_appended_queries_with_zero_w_rows_change_no_bit(nq, more, dtype):
    """behind the batch: inside the last tile, into a further tile, into a further slice"""
    q, x = gauss_case(65, 31, n=300, nq=nq + more)
    w = np.random.default_rng(3).standard_normal((nq + more, 70)).astype(np.float32)
    w[nq:] = 0
    beta = 1.0 / 8.0
    with _index(x, dtype) as ix:
        base, _ = _adj(ix, q[:nq], w[:nq], beta)
        got, _ = _adj(ix, q, w, beta)
    _bits_equal(got, base)
    assert np.abs(base).max() > 0


# ---- reproducibility -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,c,nq", [(65, 64, 300), (768, 193, NQ_MAX)])
def test_repeats_and_accumulate_give_the_same_bits(d, c, nq, dtype):
    q, x = gauss_case(d, 41, n=1029, nq=nq)  # inexact sums: the order matters
    w = np.random.default_rng(d).standard_normal((nq, c)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(x, dtype) as ix:
        a, lp = _adj(ix, q, w, beta)
        _bits_equal(a, _adj(ix, q, w, beta, lp=lp)[0], "repeat")
        _bits_equal(a, _adj(ix, q, w, beta)[0], "repeat behind its own log_partition")
        _bits_equal(a, ix.posterior_adjoint(_dev(q), _dev(w), None, temperature=1.0 / beta).cpu().numpy(), "log_partition=None")
        buf = torch.zeros((1029, c), device="cuda")
        acc = ix.posterior_adjoint(_dev(q), _dev(w), lp, temperature=1.0 / beta, out=buf, accumulate=True)
        _bits_equal(a, acc.cpu().numpy(), "accumulate on a zeroed buffer")
        twice = ix.posterior_adjoint(_dev(q), _dev(w), lp, temperature=1.0 / beta, out=buf, accumulate=True).cpu().numpy()
        if nq <= 1024:  # one slice: (a + a) exactly; with two the second call adds slice by slice, ((a + s1) + s2), a different rounding
            _bits_equal(twice, a + a, "accumulate adds")
    assert not np.isnan(a).any()


def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x, _, w = _int_case(768)
    qd, wd = _dev(q[:257]), _dev(w[:257, :129])
    with _index(x, "float16") as ix:
        serial_s, serial_i = ix.search(qd, 100)
        lp = ix.log_partition(qd, temperature=64.0)
        serial = ix.posterior_adjoint(qd, wd, lp, temperature=64.0)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            got = ix.posterior_adjoint(qd, wd, lp, temperature=64.0)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert torch.equal(got.view(torch.int32), serial.view(torch.int32))
        assert ix.get_stat("last_overflow") == 0
    _check(got.cpu().numpy(), q[:257], x, w[:257, :129], "float16", 1.0 / 64.0, what="beside a search in flight")


# ---- subset labels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 300])
def test_subset_labels(nq, dtype):
    q, x, _, w = _int_case(65)
    x, w = x[:513], w[:nq, :70]
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        for beta in (1.0, 1.0 / 64.0):
            got, _ = _adj(ix, q[:nq], w, beta, subset=sub)
            _check(got, q[:nq], x, w, dtype, beta, elig, what=f"subset nq {nq} {dtype} beta {beta:g}")
        _check(_adj(ix, q[:nq], w, 1.0)[0], q[:nq], x, w, dtype, 1.0, what="row labels without query labels")


# ---- the non-finite contract and the column scaling --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_finite_w_entry_poisons_its_column_alone(dtype):
    q, x, _, w = _int_case(65)
    q, x, w = q[:300], x[:513], w[:300, :130]
    with _index(x, dtype) as ix:
        clean, lp = _adj(ix, q, w, 1.0 / 64.0)
        wb = np.array(w)
        wb[3, 5] = np.nan
        wb[257, 129] = np.inf
        wb[299, 64] = -np.inf
        got, _ = _adj(ix, q, wb, 1.0 / 64.0, lp=lp)
    bad = np.zeros(130, dtype=bool)
    bad[[5, 64, 129]] = True
    assert np.isnan(got[:, bad]).all()
    _bits_equal(np.ascontiguousarray(got[:, ~bad]), np.ascontiguousarray(clean[:, ~bad]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaling_a_column_by_a_power_of_two_scales_it_exactly_and_small_columns_do_not_flush(dtype):
    q, x, _, _ = _int_case(65)
    q, x = q[:300], x[:513]
    w = np.random.default_rng(2).standard_normal((300, 70)).astype(np.float32)
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:
        base, lp = _adj(ix, q, w, beta)
        scale = np.ones(70, dtype=np.float32)
        scale[[0, 7, 64, 69]] = np.float32(2.0) ** np.array([-20, 7, -40, 30], dtype=np.float32)
        scaled, _ = _adj(ix, q, w * scale[None, :], beta, lp=lp)
        _bits_equal(scaled, base * scale[None, :])
        tiny_w = w * np.float32(1e-6)
        tiny, _ = _adj(ix, q, tiny_w, beta, lp=lp)  # a loss gradient of 1e-6 does not flush, fp16 included
    assert (np.abs(tiny).max(axis=0) > 0).all() and np.abs(tiny).max() < 1e-3
    _check(tiny, q, x, tiny_w, dtype, beta, what=f"W of 1e-6 {dtype}")
    _check(base, q, x, w, dtype, beta, what=f"gaussian W {dtype}")


# ---- identities on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_mass_sums_to_the_live_queries(dtype):
    q, x, _, _ = _int_case(65)
    q, x = q[:300], x[:513]
    labels = (np.arange(len(x)) % 3).astype(np.int32)
    sub = np.where(np.arange(300)[:, None] % 5 == 4, 9, -1).astype(np.int32)
    elig = np.broadcast_to((np.arange(300) % 5 != 4)[:, None], (300, len(x)))
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        mass = ix.row_mass(_dev(q), temperature=1.0 / beta, subset=sub)
        assert mass.shape == (513,) and mass.dtype == torch.float32
        weighted = ix.row_mass(_dev(q), temperature=1.0 / beta, query_weights=torch.arange(300.0), subset=sub).cpu().numpy()
    mass = mass.cpu().numpy()
    ones = np.ones(300, dtype=np.float32)
    tol = A.device_bound(q, x, ones, dtype, beta, elig, dot=False).sum()
    print(f"row mass {dtype}: sum {mass.astype(np.float64).sum():.9f} of 240 live queries, tolerance {tol:.3e}")
    assert (mass >= 0).all() and abs(mass.astype(np.float64).sum() - 240.0) <= tol
    _check(mass[:, None], q, x, ones, dtype, beta, elig, what=f"row mass {dtype}")
    _check(weighted[:, None], q, x, np.arange(300, dtype=np.float32), dtype, beta, elig, what=f"weighted row mass {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_adjoint_identity_against_the_read_out(dtype):
    q, x, v, w = _int_case(65)
    q, x, v, w = q[:300], x[:513], v[:513, :70], w[:300, :70]
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        pe = ix.posterior_expectation(_dev(q), temperature=1.0 / beta)
        adj, _ = _adj(ix, q, w, beta, lp=pe.log_partition)
    y = pe.values.cpu().numpy().astype(np.float64)
    lhs = (w.astype(np.float64) * y).sum()                       # <g, P V>
    rhs = (adj.astype(np.float64) * v.astype(np.float64)).sum()  # <P^T g, V~> (v is exact in 16 bits)
    tol = (np.abs(w) * R.device_bound(q, x, v, dtype, beta, dot=False)).sum() + (A.device_bound(q, x, w, dtype, beta, dot=False) * np.abs(v)).sum()
    print(f"adjoint identity {dtype}: <g, P V> = {lhs:.9e}, <P^T g, V> = {rhs:.9e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_query_with_unit_weight_gives_its_posterior(dtype):
    q, x, _, _ = _int_case(65)
    q, x = q[7:8], x[:513]
    for beta in (1.0 / 64.0, 1.0 / 8.0):
        with _index(x, dtype) as ix:
            got, _ = _adj(ix, q, np.ones(1, dtype=np.float32), beta)
        s = P.scores(q, x, dtype)
        m, r = P.from_scores(s, beta)
        want = np.exp(beta * (s[0] - m[0]) - r[0])  # exp(beta s - log Z)
        bound = A.device_bound(q, x, np.ones(1, dtype=np.float32), dtype, beta, dot=False)[:, 0]
        assert (np.abs(got[:, 0] - want) <= bound).all() and abs(got.astype(np.float64).sum() - 1) <= bound.sum()


# ---- Gaussian data: the full bound, every element -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    w = np.random.default_rng(seed).standard_normal((len(q), 100)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(dim)))  # the float32 the call receives
    with _index(x, dtype) as ix:
        got, _ = _adj(ix, q, w, beta)
    _check(got, q, x, w, dtype, beta, dot=True, what=f"gaussian dim {dim} {dtype}")


# ---- autograd through read_out ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_read_out_autograd_in_the_queries_and_in_the_values(dtype):
    q, x, v, w = _int_case(65)
    q, x, v, g = q[:257], x[:513], v[:513, :70], w[:257, :70]
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:
        qd = _dev(q).requires_grad_(True)
        vd = _dev(v).requires_grad_(True)
        y = ix.read_out(qd, vd, temperature=1.0 / beta)
        assert ix.row_values_shape == (513, 70)
        pe = ix.posterior_expectation(_dev(q), temperature=1.0 / beta)
        assert y.dtype == torch.float32 and y.requires_grad and torch.equal(y.detach().view(torch.int32), pe.values.view(torch.int32))
        y.backward(_dev(g))
        assert vd.grad.dtype == torch.float32 and vd.grad.shape == (513, 70) and qd.grad.shape == (257, 65)
        explicit, _ = _adj(ix, q, g, beta, lp=pe.log_partition)
        _bits_equal(vd.grad.cpu().numpy(), explicit, "V.grad is the explicit call")
        q2 = _dev(q).requires_grad_(True)
        ix.expected_values(q2, temperature=1.0 / beta).backward(_dev(g))
        _bits_equal(qd.grad.cpu().numpy(), q2.grad.cpu().numpy(), "q.grad is expected_values'")
        # a 16-bit table gets a gradient of its dtype: the float32 result rounded once
        vh = _dev(v).to(TDT[dtype]).requires_grad_(True)
        ix.read_out(_dev(q), vh, temperature=1.0 / beta).backward(_dev(g))
        assert vh.grad.dtype == TDT[dtype] and torch.equal(vh.grad, torch.from_numpy(explicit).cuda().to(TDT[dtype]))
        # a `values` that does not require grad runs no adjoint scan; queries that do not, no query-gradient scan
        calls = {"adjoint": 0, "backward": 0}
        real_adj, real_bw = ix.posterior_adjoint, ix.posterior_expectation_backward

        def count_adj(*a, **k):
            calls["adjoint"] += 1
            return real_adj(*a, **k)

        def count_bw(*a, **k):
            calls["backward"] += 1
            return real_bw(*a, **k)

        ix.posterior_adjoint, ix.posterior_expectation_backward = count_adj, count_bw
        q3 = _dev(q).requires_grad_(True)
        ix.read_out(q3, _dev(v), temperature=1.0 / beta).backward(_dev(g))
        assert calls == {"adjoint": 0, "backward": 1} and q3.grad is not None
        v3 = _dev(v).requires_grad_(True)
        ix.read_out(_dev(q), v3, temperature=1.0 / beta).backward(_dev(g))
        assert calls == {"adjoint": 1, "backward": 1}
        _bits_equal(v3.grad.cpu().numpy(), explicit)
        with pytest.raises(RuntimeError):  # once differentiable
            v4 = _dev(v).requires_grad_(True)
            (g4,) = torch.autograd.grad(ix.read_out(_dev(q), v4, temperature=1.0 / beta).sum(), v4, create_graph=True)
            g4.sum().backward()
        del ix.posterior_adjoint, ix.posterior_expectation_backward
        # a trainable table over a frozen key store: one SGD step lowers a squared loss
        table = torch.zeros((513, 4), device="cuda", requires_grad=True)
        target = _dev(np.eye(4, dtype=np.float32)[np.arange(257) % 4])
        loss0 = ((ix.read_out(_dev(q), table, temperature=1.0 / beta) - target) ** 2).sum()
        loss0.backward()
        with torch.no_grad():
            table -= table.grad / 257  # (stable: the largest eigenvalue of P^T P is below the largest row mass, at most 257)
        loss1 = ((ix.read_out(_dev(q), table, temperature=1.0 / beta) - target) ** 2).sum()
        assert loss1 < loss0
    # float64 dense softmax autograd on the GPU over the same rows
    xr = _dev(x).double()
    q64 = _dev(q).double().requires_grad_(True)
    v64 = _dev(v).double().requires_grad_(True)
    (torch.softmax(beta * (q64 @ xr.T), dim=1) @ v64 * _dev(g).double()).sum().backward()
    vb = A.device_bound(q, x, g, dtype, beta, dot=False)
    verr = np.abs(explicit.astype(np.float64) - v64.grad.cpu().numpy())
    qb = G.device_bound(q, x, v, g, dtype, beta, dot=False)
    qerr = np.abs(qd.grad.cpu().numpy().astype(np.float64) - q64.grad.cpu().numpy())
    print(f"autograd {dtype}: V.grad max err / bound = {(verr / np.maximum(vb, 1e-300)).max():.3e}, q.grad max err / bound = {(qerr / qb).max():.3e}")
    assert (verr <= vb + 1e-13 * np.abs(explicit)).all()
    assert (qerr <= qb + 1e-13 * np.abs(qd.grad.cpu().numpy())).all()


# ---- node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [1029, 4000])
def test_node_index_concatenates_the_shards(capacity):
    from vod_amd.index import HipNodeIndex, LogPartition

    q, x, v, w = _int_case(65)
    nq, beta = 300, 1.0 / 64.0
    q, w, v = q[:nq], w[:nq, :70], v[:, :70]
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, "float16") as ix:
        ix.set_row_labels(labels)
        flat, flat_lp = _adj(ix, q, w, beta)
        flat_sub, flat_lp_sub = _adj(ix, q, w, beta, subset=sub)
    host = lambda lp: LogPartition(*(t.cpu().numpy() for t in lp))  # noqa: E731
    with HipNodeIndex(65, capacity, [0, 0]) as nx:  # two shards on device 0; capacity 4000: shard 0 holds every row, shard 1 none
        nx.add(x.astype(np.float32))
        own_lp = nx.log_partition(np.array(q), temperature=1.0 / beta)
        got = nx.posterior_adjoint(np.array(q), np.array(w), own_lp, temperature=1.0 / beta)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (len(x), 70)
        # an element depends on its row, the queries and their words alone: handed the flat index's words, the flat index's bits
        _bits_equal(nx.posterior_adjoint(np.array(q), np.array(w), host(flat_lp), temperature=1.0 / beta), flat, capacity)
        nx.set_row_labels(labels)
        own_lp_sub = nx.log_partition(np.array(q), temperature=1.0 / beta, subset=sub)
        got_sub = nx.posterior_adjoint(np.array(q), np.array(w), own_lp_sub, temperature=1.0 / beta, subset=sub)
        _bits_equal(nx.posterior_adjoint(np.array(q), np.array(w), host(flat_lp_sub), temperature=1.0 / beta, subset=sub), flat_sub, capacity)
        _bits_equal(nx.posterior_adjoint(np.array(q), np.array(w), None, temperature=1.0 / beta, subset=sub), got_sub, "log_partition=None")
        mass = nx.row_mass(np.array(q), temperature=1.0 / beta, subset=sub)
        assert mass.shape == (len(x),) and abs(float(mass.astype(np.float64).sum()) - 225.0) < 1e-2
        # autograd through the host
        qt = torch.from_numpy(np.array(q)).requires_grad_(True)
        vt = torch.from_numpy(np.array(v)).requires_grad_(True)
        nx.read_out(qt, vt, temperature=1.0 / beta, subset=sub).backward(torch.from_numpy(np.array(w)))
        _bits_equal(vt.grad.numpy(), got_sub)
        assert qt.grad.shape == (nq, 65) and torch.isfinite(qt.grad).all()
    # within the bound with the node's own forward words: log_rel is the host fold of the shards' pairs (its error: `fold`, as derived
    # for the read-out's node test)
    for res, e in ((got, None), (got_sub, elig)):
        n = len(x) if e is None else e.sum(axis=1)
        fold = 2 * (P.device_bound(np.zeros((nq, 1)), None, None, beta, n, dot=False) + 4 * P.U * (1 + np.log(len(x)))) + 2 * P.U
        _check(res, q, x, w, "float16", beta, e, what=f"node capacity {capacity}", rel_extra=fold)
        assert not np.isnan(res).any()


# ---- refusals and empty cases ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex, LogPartition

    lib = _native.load_library()
    q, x, _, w = _int_case(65)
    x, w = x[:600], w[:5, :5]
    qd, wd = _dev(q[:5]), _dev(w)
    words = torch.zeros((2, 5), device="cuda")
    out = torch.full((600, 5), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    opt = lambda t: None if t is None else ptr(t)  # noqa: E731

    def raw(h, queries=qd, code=2, nq=5, beta=1.0, lab=None, n_lab=0, m=words[0], r=words[1], wv=wd, n_cols=5, acc=0, o=out):
        return lib.vodhip_index_posterior_adjoint(h, opt(queries), code, nq, ctypes.c_float(beta), opt(lab), n_lab, opt(m), opt(r), opt(wv), n_cols, acc,
                                                  opt(o), None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    fake = LogPartition(words[0], words[0], words[1])
    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x, "float16") as ix:
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        refused(raw(ix._h, m=None), "invalid query / output pointers")
        refused(raw(ix._h, r=None), "invalid query / output pointers")
        refused(raw(ix._h, wv=None), "weights is NULL")
        refused(raw(ix._h, o=None), "out is NULL")
        refused(raw(ix._h, nq=-1), "invalid query / output pointers")
        refused(raw(ix._h, code=3), "invalid q_dtype 3")
        refused(raw(ix._h, n_cols=0), "n_cols must be in [1, 256]")
        refused(raw(ix._h, n_cols=257), "n_cols must be in [1, 256]")
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            refused(raw(ix._h, beta=beta), "beta must be finite and > 0")
        refused(raw(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=2), "set the row labels first")
        with pytest.raises(_native.NativeLibraryError, match=r"n_cols must be in \[1, 256\]"):
            ix.posterior_adjoint(qd, torch.zeros((5, 257), device="cuda"), fake)
        with pytest.raises(_native.NativeLibraryError, match=r"n_cols must be in \[1, 256\]"):
            ix.posterior_adjoint(qd, torch.zeros((5, 0), device="cuda"), fake)
        for bad in (wd[:4], torch.zeros((4,), device="cuda"), torch.zeros((5, 2, 2), device="cuda")):  # mis-shaped weights
            with pytest.raises(ValueError, match="weights"):
                ix.posterior_adjoint(qd, bad, fake)
        with pytest.raises(ValueError, match="max_score"):
            ix.posterior_adjoint(qd, wd, LogPartition(words[0, :4], words[0, :4], words[1, :4]))
        with pytest.raises(ValueError, match="out"):
            ix.posterior_adjoint(qd, wd, fake, out=torch.zeros((599, 5), device="cuda"))
        with pytest.raises(ValueError, match="accumulate"):
            ix.posterior_adjoint(qd, wd, fake, accumulate=True)
        torch.cuda.synchronize()
        assert (out == 123.0).all()  # a refused call writes nothing
        # nq == 0: accumulating leaves `out` alone, the plain call zero-fills it
        assert raw(ix._h, queries=None, nq=0, m=None, r=None, wv=None, acc=1) == 0
        torch.cuda.synchronize()
        assert (out == 123.0).all()
        assert raw(ix._h, queries=None, nq=0, m=None, r=None, wv=None) == 0
        torch.cuda.synchronize()
        assert (out.view(torch.int32) == 0).all()
        empty = ix.posterior_adjoint(torch.zeros((0, 65), device="cuda"), torch.zeros((0, 3), device="cuda"))
        assert empty.shape == (600, 3) and (empty == 0).all()
        got, _ = _adj(ix, q[:5], w, 1.0 / 64.0)
        _check(got, q[:5], x, w, "float16", 1.0 / 64.0, what="after the refusals")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        refused(raw(ix._h), "posterior_adjoint is not supported on an L2 index")
        with pytest.raises(_native.NativeLibraryError, match="posterior_adjoint is not supported on an L2 index"):
            ix.posterior_adjoint(qd, wd, fake)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        refused(raw(ix._h), "VODHIP_EXACT_F32")
        assert "posterior_adjoint" in lib.vodhip_last_error().decode()
        with pytest.raises(_native.NativeLibraryError, match="posterior_adjoint.*VODHIP_EXACT_F32"):
            ix.row_mass(qd, log_partition=fake)
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty index: a no-op that returns no rows
        assert raw(ix._h) == 0
        assert ix.posterior_adjoint(qd, wd).shape == (0, 5)
    torch.cuda.synchronize()
    host_fake = LogPartition(np.zeros(5, np.float32), np.zeros(5, np.float32), np.zeros(5, np.float32))
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        nx.add(x.astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            nx.posterior_adjoint(np.array(q[:5]), np.array(w), host_fake, temperature=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.posterior_adjoint(np.array(q[:5]), np.array(w), host_fake, subset=np.zeros((5, 2), dtype=np.int32))
        with pytest.raises(_native.NativeLibraryError, match=r"n_cols must be in \[1, 256\]"):
            nx.posterior_adjoint(np.array(q[:5]), np.zeros((5, 257), np.float32), host_fake)
        with pytest.raises(ValueError, match="weights"):
            nx.posterior_adjoint(np.array(q[:5]), np.array(w[:4]), host_fake)
        empty = nx.posterior_adjoint(np.zeros((0, 65), dtype=np.float32), np.zeros((0, 3), dtype=np.float32))
        assert empty.shape == (600, 3) and (empty == 0).all()
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:  # (a node index is never an L2 index: its constructor refuses the metric)
        with pytest.raises(_native.NativeLibraryError, match="posterior_adjoint.*VODHIP_EXACT_F32"):
            nx.posterior_adjoint(np.array(q[:5]), np.array(w), host_fake)
