"""`key_gradient` of both indexes and the `keys` keyword of `log_z` / `read_out` on the GPU against the float64 restatement
(tests/key_grad_ref.py); every element of every case is compared against `key_grad_ref.device_bound`, which is derived, not fitted, and
the worst err / bound is printed.

Integer data (rows, queries and table in [-8, 8], a and G integers in [-4, 4] times 2^-10: everything exact in fp16 and bf16, every score
an exact integer in float32, so the bound's dot-product part is dropped): stores of 1, 63, 64, 65, 513 and 1029 rows, batches of 1, 255,
256, 257 and 1024 + 65 (a second slice adds), dims 1, 64, 65, 191, 192, 193, 256, 257, 449, 768 (either chunk width at, below and above
its edge, a partial last chunk), no table (log Z only) and tables of 1, 64, 65 and 256 columns with a alone, G alone and both, beta 1,
1/64, 4, both store dtypes.  Then the four identities, masked positions, dead and zero-gradient queries, subset labels, the non-finite
contract, reproducibility, accumulate, the slice edge, a call beside a search in flight, appended rows, the node index, autograd,
refusals.  Measured maxima (MI355X): DESIGN.md 4 "Key gradient".
"""
import ctypes
import functools

import numpy as np
import pytest

import key_grad_ref as K
import partition_ref as P
import posterior_ref as PM
import readout_adjoint_ref as A
import readout_grad_ref as G_
import readout_ref as R
from l2_ref import round_store
from test_l2_cpu import gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
STORES = [1, 63, 64, 65, 513, 1029]
BATCHES = [1, 255, 256, 257, 1024 + 65]
DIMS = [1, 64, 65, 191, 192, 193, 256, 257, 449, 768]
TABLES = [None, 1, 64, 65, 256]
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
    """integer rows / queries / table and 16-bit-exact gradients; the same for both store dtypes"""
    rng = np.random.default_rng(7000 + d + n)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    v = rng.integers(-8, 9, size=(n, 256)).astype(np.float32)
    a = (rng.integers(-4, 5, size=nq) * 2.0 ** -10).astype(np.float32)
    g = (rng.integers(-4, 5, size=(nq, 256)) * 2.0 ** -10).astype(np.float32)
    for t in (q, x, v, a, g):
        t.setflags(write=False)
    return q, x, v, a, g


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _kg(ix, q, beta, a=None, g=None, fwd=None, **kw):
    """the key gradient as NumPy float32 [ntotal, dim], and the forward it was given (a PosteriorExpectation with g, else a LogPartition)"""
    qd = _dev(q)
    t = 1.0 / beta
    sub = kw.get("subset")
    if fwd is None:
        fwd = ix.posterior_expectation(qd, temperature=t, subset=sub) if g is not None else ix.log_partition(qd, temperature=t, subset=sub)
    out = ix.key_gradient(qd, grad_log_z=None if a is None else _dev(a), grad_values=None if g is None else _dev(g),
                          expectation=fwd if g is not None else None, log_partition=None if g is not None else fwd, temperature=t, **kw)
    assert out.dtype == torch.float32 and out.shape == (ix.ntotal, ix.dim) and out.is_cuda
    return out.cpu().numpy(), fwd


def _check(got, q, x, dtype, beta, a=None, g=None, v=None, eligible=None, dot=False, what="", **kw):
    """every (row, column) within the derived bound"""
    ref, _, _, _ = K.key_gradient(q, x, dtype, beta, a, g, v, eligible)
    bound = K.device_bound(q, x, dtype, beta, a, g, v, eligible, dot=dot, **kw)
    assert got.shape == ref.shape, what
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max() if err.size else 0.0
    print(f"{what}: max |key gradient - float64| = {err.max() if err.size else 0.0:.3e}, max err / bound = {ratio:.3e}")
    assert not np.isnan(err).any(), what
    assert (err <= bound).all(), (what, ratio)
    return ratio


def _bits_equal(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def _run(ix, q, x, v, a, g, dtype, beta, table, mode, what):
    """one (table width, mode) case on an index that holds x: `mode` a | g | ag"""
    aa = a if "a" in mode else None
    gg = vv = None
    if table is not None:
        ix.set_row_values(v[:len(x), :table])
        if "g" in mode:
            gg, vv = g[:len(q), :table], v[:len(x), :table]
    elif ix.row_values_shape is not None:
        ix.set_row_values(None)
    got, _ = _kg(ix, q, beta, aa, gg)
    return _check(got, q, x, dtype, beta, aa, gg, vv, what=f"{what} table {table} mode {mode} {dtype} beta {beta:g}")


def _mode(table, k):
    return "a" if table is None else ("g", "ag", "a")[k % 3]


# ---- sizes, batches, dims, tables, modes, betas on integer data ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_with_every_table(n, dtype):
    i = STORES.index(n)
    d = DIMS[(3 * i + 1) % 10]
    q, x, v, a, g = _int_case(d)
    x = x[:n]
    with _index(x, dtype) as ix:
        for k, table in enumerate(TABLES):
            beta, nq = BETAS[(k + i) % 3], BATCHES[(k + i) % 4]
            _run(ix, q[:nq], x, v, a[:nq], g, dtype, beta, table, _mode(table, k + i), f"n {n} d {d} nq {nq}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", BATCHES)
def test_batch_sizes_across_the_query_tile_and_the_slice(nq, dtype):
    i = BATCHES.index(nq)
    d = DIMS[(2 * i + 2) % 10]
    q, x, v, a, g = _int_case(d)
    with _index(x, dtype) as ix:  # 1029 rows: 17 row tiles, 24 launched per chunk
        for k in range(3):
            table, beta = TABLES[(2 * i + 2 * k) % 5], BETAS[(i + k) % 3]
            _run(ix, q[:nq], x, v, a[:nq], g, dtype, beta, table, _mode(table, i + k), f"nq {nq} d {d}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_dims_with_every_beta_and_mode(d, dtype):
    i = DIMS.index(d)
    q, x, v, a, g = _int_case(d)
    x, q, a = x[:513], q[:257], a[:257]
    with _index(x, dtype) as ix:
        for k, beta in enumerate(BETAS):
            table = TABLES[(i + 2 * k + 1) % 5]
            _run(ix, q, x, v, a, g, dtype, beta, table, _mode(table, k), f"d {d}")
        _run(ix, q, x, v, a, g, dtype, 1.0 / 64.0, None, "a", f"d {d}")  # (both chunk widths at every dim)
        _run(ix, q, x, v, a, g, dtype, 1.0 / 64.0, 65, "ag", f"d {d}")


# ---- identities: none relies on the code under test for its own yardstick ------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 256])
def test_identity_i_log_z_only_agrees_with_the_adjoint(d, dtype):
    q, x, _, a, _ = _int_case(d)
    q, x, a = q[:300], x[:513], a[:300]
    beta = 1.0 / 64.0
    w = a[:, None] * q  # (exact: small integers times 2^-10)
    with _index(x, dtype) as ix:
        got, lp = _kg(ix, q, beta, a)
        adj = ix.posterior_adjoint(_dev(q), _dev(w), lp, temperature=1.0 / beta).cpu().numpy()
    tol = K.device_bound(q, x, dtype, beta, a, dot=False) + beta * A.device_bound(q, x, w, dtype, beta, dot=False)
    err = np.abs(got.astype(np.float64) - beta * adj.astype(np.float64))
    print(f"identity (i) d {d} {dtype}: max err / (sum of the two bounds) = {(err / tol).max():.3e}")
    assert (err <= tol).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_ii_the_rows_sum_to_the_log_z_term(dtype):
    q, x, v, a, g = _int_case(193)
    q, x, v, a, g = q[:300], x[:513], v[:513, :65], a[:300], g[:300, :65]
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        for aa in (a, None):
            got, _ = _kg(ix, q, beta, aa, g)
            want = np.zeros(193) if aa is None else beta * (aa.astype(np.float64)[:, None] * q.astype(np.float64)).sum(axis=0)
            tol = K.device_bound(q, x, dtype, beta, aa, g, v, dot=False).sum(axis=0)
            err = np.abs(got.astype(np.float64).sum(axis=0) - want)
            print(f"identity (ii) {dtype} a {aa is not None}: max err / tolerance = {(err / tol).max():.3e}")
            assert (err <= tol).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_iii_duality_with_the_query_gradients(dtype):
    q, x, v, a, g = _int_case(65)
    q, x, v, a, g = q[:300], x[:513], v[:513, :70], a[:300], g[:300, :70]
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        got, pe = _kg(ix, q, beta, a, g)
        gq = ix.posterior_expectation_backward(_dev(q), _dev(g), pe, temperature=1.0 / beta).cpu().numpy().astype(np.float64)
        mean = ix.posterior_mean(_dev(q), temperature=1.0 / beta).mean.cpu().numpy().astype(np.float64)
    gq = gq + beta * a.astype(np.float64)[:, None] * mean
    lhs = (got.astype(np.float64) * x).sum()      # sum_zd out x~ (x, q exact in 16 bits)
    rhs = (gq * q).sum()                          # sum_qd grad_q q~
    tol = (K.device_bound(q, x, dtype, beta, a, g, v, dot=False) * np.abs(x)).sum()
    tol += ((G_.device_bound(q, x, v, g, dtype, beta, dot=False) + beta * np.abs(a)[:, None] * PM.device_bound(q, x, dtype, beta, dot=False)) * np.abs(q)).sum()
    print(f"identity (iii) {dtype}: <out, x> = {lhs:.9e}, <grad_q, q> = {rhs:.9e}, tolerance {tol:.3e}")
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("dtype", DTYPES)
def test_identity_iv_a_column_of_ones_adds_nothing(dtype):
    q, x, v, a, g = _int_case(65)
    q, x, a = q[:300], x[:513], a[:300]
    beta = 1.0 / 64.0
    v1 = np.array(v[:513, :65])
    v1[:, 64] = 1
    g1 = np.array(g[:300, :65])
    g1[:, 64] = (np.random.default_rng(4).integers(-4, 5, size=300) * 2.0 ** -10).astype(np.float32)  # arbitrary, as large as the rest
    with _index(x, dtype) as ix:
        ix.set_row_values(v1)
        with_ones, _ = _kg(ix, q, beta, a, g1)
        ix.set_row_values(v1[:, :64])
        without, _ = _kg(ix, q, beta, a, g1[:, :64])
    tol = K.device_bound(q, x, dtype, beta, a, g1, v1, dot=False) + K.device_bound(q, x, dtype, beta, a, g1[:, :64], v1[:, :64], dot=False)
    err = np.abs(with_ones.astype(np.float64) - without.astype(np.float64))
    print(f"identity (iv) {dtype}: max err / (sum of the two bounds) = {(err / tol).max():.3e}")
    assert (err <= tol).all()
    # the column alone: u - ubar = g (1 - sum_z p_z): within the bound of a zero result
    only = np.zeros((300, 65), dtype=np.float32)
    only[:, 64] = g1[:, 64]
    with _index(x, dtype) as ix:
        ix.set_row_values(v1)
        got, _ = _kg(ix, q, beta, None, only)
    assert (np.abs(got) <= K.device_bound(q, x, dtype, beta, None, only, v1, dot=False)).all()


# ---- masked positions, dead and zero-gradient queries --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_past_ntotal_never_leak(dtype):
    q, x, v, a, g = _int_case(65)
    q, a, g = q[:257], a[:257], g[:257, :65]
    stale = np.array(x[:600]) * 4  # larger scores than any live row: a leak would dominate
    stale[130:256:3] = np.nan      # and NaN among the stale rows of the last live tile
    canary = 123.0
    with _index(stale, dtype, capacity=600) as ix:
        ix.reset()
        ix.add(x[:130])
        ix.set_row_values(v[:130, :65])
        assert ix.ntotal == 130
        buf = torch.full((131, 65), canary, device="cuda")
        pe = ix.posterior_expectation(_dev(q), temperature=64.0)
        out = ix.key_gradient(_dev(q), grad_log_z=_dev(a), grad_values=_dev(g), expectation=pe, temperature=64.0, out=buf[:130])
        assert out.shape == (130, 65) and out.data_ptr() == buf.data_ptr()
        torch.cuda.synchronize()
        assert (buf[130] == canary).all()  # the row behind `out` is untouched
        _check(buf[:130].cpu().numpy(), q, x[:130], dtype, 1.0 / 64.0, a, g, v[:130, :65], what=f"stale rows past ntotal {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_stored_row_with_a_nan_component_receives_plus_zero(dtype):
    q, x, v, a, g = _int_case(65)
    q, a, g, v = q[:130], a[:130], g[:130, :70], v[:300, :70]
    xn = np.array(x[:300])
    xn[[7, 64, 299], 3] = np.nan
    with _index(xn, dtype) as ix:
        ix.set_row_values(v)
        for aa, gg in ((a, None), (a, g)):
            got, _ = _kg(ix, q, 1.0 / 64.0, aa, gg)
            assert (got[[7, 64, 299]].view(np.uint32) == 0).all() and np.isfinite(got).all()
            _check(got, q, xn, dtype, 1.0 / 64.0, aa, gg, None if gg is None else v, what=f"NaN rows {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,more", [(100, 30), (250, 50), (1000, 89)])
def test_dead_and_zero_gradient_queries_behind_a_batch_change_no_bit(nq, more, dtype):
    """behind the batch: inside the last tile, into a further tile, into a further slice"""
    q, x = gauss_case(65, 31, n=300, nq=nq + more)
    rng = np.random.default_rng(3)
    v = rng.standard_normal((300, 70)).astype(np.float32)
    a, g = rng.standard_normal(nq + more).astype(np.float32), rng.standard_normal((nq + more, 70)).astype(np.float32)
    beta = 1.0 / 8.0
    labels = np.zeros(300, dtype=np.int32)
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        ix.set_row_labels(labels)
        sub = np.full((nq + more, 1), -1, dtype=np.int32)
        for aa, gg in ((a, None), (a, g)):
            base, _ = _kg(ix, q[:nq], beta, aa[:nq], None if gg is None else gg[:nq], subset=sub[:nq])
            assert np.abs(base).max() > 0
            # zero gradients behind the batch
            az, gz = np.array(aa), None if gg is None else np.array(gg)
            az[nq:] = 0
            if gz is not None:
                gz[nq:] = 0
            _bits_equal(_kg(ix, q, beta, az, gz, subset=sub)[0], base, "zero-gradient queries")
            # dead queries behind the batch (a label no row has), with gradients LARGER than the batch's: they enter no scale
            sd = np.array(sub)
            sd[nq:] = 9
            got, fwd = _kg(ix, q, beta, aa * np.where(np.arange(nq + more) >= nq, 64, 1).astype(np.float32),
                           None if gg is None else gg * np.where(np.arange(nq + more) >= nq, 64, 1).astype(np.float32)[:, None], subset=sd)
            lp = fwd if gg is None else fwd.log_partition
            assert torch.isneginf(lp.max_score[nq:]).all()
            _bits_equal(got, base, "dead queries")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 300])
def test_subset_labels(nq, dtype):
    q, x, v, a, g = _int_case(65)
    x, v, a, g = x[:513], v[:513, :70], a[:nq], g[:nq, :70]
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        ix.set_row_values(v)
        for beta in (1.0, 1.0 / 64.0):
            got, _ = _kg(ix, q[:nq], beta, a, g, subset=sub)
            _check(got, q[:nq], x, dtype, beta, a, g, v, elig, what=f"subset nq {nq} {dtype} beta {beta:g}")
        got, _ = _kg(ix, q[:nq], 1.0 / 64.0, a, subset=sub)
        _check(got, q[:nq], x, dtype, 1.0 / 64.0, a, eligible=elig, what=f"subset nq {nq} {dtype} log Z only")


# ---- the non-finite contract, the batch scale --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_finite_gradient_makes_the_whole_result_nan(dtype):
    q, x, v, a, g = _int_case(65)
    q, x, v, a, g = q[:300], x[:513], v[:513, :70], a[:300], g[:300, :70]
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        _, pe = _kg(ix, q, 1.0 / 64.0, a, g)
        for where, bad in (("a", np.nan), ("a", np.inf), ("g", np.nan), ("g", -np.inf)):
            ab, gb = np.array(a), np.array(g)
            if where == "a":
                ab[257] = bad
            else:
                gb[3, 69] = bad
            got, _ = _kg(ix, q, 1.0 / 64.0, ab, gb, fwd=pe)
            assert np.isnan(got).all(), (where, bad)
        ab = np.array(a)
        ab[7] = np.nan
        assert np.isnan(_kg(ix, q, 1.0 / 64.0, ab)[0]).all()
        # a non-finite forward value under a non-zero gradient entry
        yb = pe.values.clone()
        yb[5, 2] = float("inf")
        gb = np.array(g)
        gb[5, 2] = 2.0 ** -10
        got, _ = _kg(ix, q, 1.0 / 64.0, a, gb, fwd=type(pe)(yb, pe.log_partition))
        assert np.isnan(got).all()
        gb[5, 2] = 0  # under a zero entry it is not used
        got, _ = _kg(ix, q, 1.0 / 64.0, a, gb, fwd=type(pe)(yb, pe.log_partition))
        _check(got, q, x, dtype, 1.0 / 64.0, a, gb, v, what=f"unused non-finite y {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaling_the_gradients_by_a_power_of_two_scales_exactly_and_small_gradients_do_not_flush(dtype):
    q, x = gauss_case(65, 17, n=513, nq=300)
    rng = np.random.default_rng(2)
    v = rng.standard_normal((513, 70)).astype(np.float32)
    a, g = rng.standard_normal(300).astype(np.float32), rng.standard_normal((300, 70)).astype(np.float32)
    beta = 1.0 / 8.0
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        base, pe = _kg(ix, q, beta, a, g)
        for s in (2.0 ** -20, 2.0 ** 9):
            scaled, _ = _kg(ix, q, beta, a * np.float32(s), g * np.float32(s), fwd=pe)
            _bits_equal(scaled, base * np.float32(s), s)
        tiny, _ = _kg(ix, q, beta, a * np.float32(1e-6), g * np.float32(1e-6), fwd=pe)  # a loss gradient of 1e-6 does not flush, fp16 included
        # one query far below the batch's largest: relative precision is lost, absolute precision (the bound's floor) is not
        a2, g2 = np.array(a), np.array(g)
        a2[11] *= np.float32(2.0 ** -22)
        g2[11] *= np.float32(2.0 ** -22)
        mixed, _ = _kg(ix, q, beta, a2, g2, fwd=pe)
    assert np.abs(tiny).max() > 0 and np.abs(tiny).max() < 1e-3
    _check(tiny, q, x, dtype, beta, a * np.float32(1e-6), g * np.float32(1e-6), v, dot=True, what=f"gradients of 1e-6 {dtype}")
    _check(base, q, x, dtype, beta, a, g, v, dot=True, what=f"gaussian gradients {dtype}")
    _check(mixed, q, x, dtype, beta, a2, g2, v, dot=True, what=f"one small query {dtype}")


# ---- reproducibility, accumulate, the slice edge --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,c,nq", [(65, 64, 300), (449, 193, NQ_MAX)])
def test_repeats_and_accumulate_give_the_same_bits(d, c, nq, dtype):
    q, x = gauss_case(d, 41, n=1029, nq=nq)  # inexact sums: the order matters
    rng = np.random.default_rng(d)
    v = rng.standard_normal((1029, c)).astype(np.float32)
    a, g = rng.standard_normal(nq).astype(np.float32), rng.standard_normal((nq, c)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        first, pe = _kg(ix, q, beta, a, g)
        _bits_equal(first, _kg(ix, q, beta, a, g, fwd=pe)[0], "repeat")
        _bits_equal(first, _kg(ix, q, beta, a, g)[0], "repeat behind its own forward")
        auto = ix.key_gradient(_dev(q), grad_log_z=_dev(a), grad_values=_dev(g), temperature=1.0 / beta)
        _bits_equal(first, auto.cpu().numpy(), "no forward handed in")
        buf = torch.zeros((1029, d), device="cuda")
        kw = dict(grad_log_z=_dev(a), grad_values=_dev(g), expectation=pe, temperature=1.0 / beta, out=buf, accumulate=True)
        _bits_equal(first, ix.key_gradient(_dev(q), **kw).cpu().numpy(), "accumulate on a zeroed buffer")
        twice = ix.key_gradient(_dev(q), **kw).cpu().numpy()
        if nq <= 1024:  # one slice: (a + a) exactly; with two the second call adds slice by slice, a different rounding
            _bits_equal(twice, first + first, "accumulate adds")
        la, _ = _kg(ix, q, beta, a)
        _bits_equal(la, _kg(ix, q, beta, a)[0], "log Z only repeat")
    assert not np.isnan(first).any()
    _check(first, q, x, dtype, beta, a, g, v, dot=True, what=f"gaussian d {d} c {c} nq {nq} {dtype}")
    _check(la, q, x, dtype, beta, a, dot=True, what=f"gaussian d {d} nq {nq} {dtype} log Z only")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [1023, 1024, 1025])
def test_the_slice_edge_at_1024(nq, dtype):
    q, x, v, a, g = _int_case(65)
    q, x, v, a, g = q[:nq], x[:130], v[:130, :1], a[:nq], g[:nq, :1]
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        got, _ = _kg(ix, q, 1.0 / 64.0, a, g)
    _check(got, q, x, dtype, 1.0 / 64.0, a, g, v, what=f"nq {nq} {dtype}")


def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x, v, a, g = _int_case(768)
    qd, ad, gd = _dev(q[:257]), _dev(a[:257]), _dev(g[:257, :65])
    with _index(x, "float16") as ix:
        ix.set_row_values(v[:, :65])
        serial_s, serial_i = ix.search(qd, 100)
        pe = ix.posterior_expectation(qd, temperature=64.0)
        kw = dict(grad_log_z=ad, grad_values=gd, expectation=pe, temperature=64.0)
        serial = ix.key_gradient(qd, **kw)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            got = ix.key_gradient(qd, **kw)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert torch.equal(got.view(torch.int32), serial.view(torch.int32))
        assert ix.get_stat("last_overflow") == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_appended_to_the_store_leave_the_earlier_rows_bits(dtype):
    """given the same forward words and scales an element depends on its own row alone"""
    q, x = gauss_case(193, 23, n=513, nq=300)
    rng = np.random.default_rng(5)
    v = rng.uniform(-1, 1, size=(513, 65)).astype(np.float32)
    v[0] = 1  # the column maxima sit in the first rows: the table's scales do not move when rows are appended
    a, g = rng.standard_normal(300).astype(np.float32), rng.standard_normal((300, 65)).astype(np.float32)
    beta = 1.0 / 16.0
    with _index(x[:300], dtype, capacity=600) as ix:
        ix.set_row_values(v[:300])
        with_table, pe = _kg(ix, q, beta, a, g)
        log_z_only, lp = _kg(ix, q, beta, a)
        ix.add(x[300:])
        ix.set_row_values(v)
        assert ix.ntotal == 513
        _bits_equal(_kg(ix, q, beta, a, g, fwd=pe)[0][:300], with_table, "table term")
        _bits_equal(_kg(ix, q, beta, a, fwd=lp)[0][:300], log_z_only, "log Z only")


# ---- node index ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [1029, 4000])
def test_node_index_concatenates_the_shards(capacity):
    from vod_amd.index import HipNodeIndex, LogPartition, PosteriorExpectation

    q, x, v, a, g = _int_case(65)
    nq, beta = 300, 1.0 / 64.0
    q, a, g, v = q[:nq], a[:nq], g[:nq, :70], v[:, :70]
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, "float16") as ix:
        ix.set_row_labels(labels)
        ix.set_row_values(v)
        flat, flat_pe = _kg(ix, q, beta, a, g)
        flat_sub, flat_pe_sub = _kg(ix, q, beta, a, g, subset=sub)
        flat_a, flat_lp = _kg(ix, q, beta, a)
    host_lp = lambda lp: LogPartition(*(t.cpu().numpy() for t in lp))  # noqa: E731
    host_pe = lambda pe: PosteriorExpectation(pe.values.cpu().numpy(), host_lp(pe.log_partition))  # noqa: E731
    qh, ah, gh = np.array(q), np.array(a), np.array(g)
    with HipNodeIndex(65, capacity, [0, 0]) as nx:  # two shards on device 0; capacity 4000: shard 0 holds every row, shard 1 none
        nx.add(x.astype(np.float32))
        # log Z only needs no table
        _bits_equal(nx.key_gradient(qh, grad_log_z=ah, log_partition=host_lp(flat_lp), temperature=1.0 / beta), flat_a, capacity)
        nx.set_row_values(np.array(v))
        got = nx.key_gradient(qh, grad_log_z=ah, grad_values=gh, temperature=1.0 / beta)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (len(x), 65)
        # an element depends on its row, the queries, their words and the batch-wide scales alone - the scales on the column maxima over
        # ALL the shards: handed the flat index's words, the flat index's bits
        _bits_equal(nx.key_gradient(qh, grad_log_z=ah, grad_values=gh, expectation=host_pe(flat_pe), temperature=1.0 / beta), flat, capacity)
        nx.set_row_labels(labels)
        _bits_equal(nx.key_gradient(qh, grad_log_z=ah, grad_values=gh, expectation=host_pe(flat_pe_sub), temperature=1.0 / beta, subset=sub), flat_sub,
                    capacity)
        got_sub = nx.key_gradient(qh, grad_log_z=ah, grad_values=gh, temperature=1.0 / beta, subset=sub)
        acc = np.ones_like(got_sub)
        assert nx.key_gradient(qh, grad_log_z=ah, grad_values=gh, temperature=1.0 / beta, subset=sub, out=acc, accumulate=True) is acc
        _bits_equal(acc, got_sub + np.float32(1), "accumulate on the host")
        # autograd through the host
        qt = torch.from_numpy(qh).requires_grad_(True)
        vt = torch.from_numpy(np.array(v)).requires_grad_(True)
        kt = torch.zeros((len(x), 65), requires_grad=True)
        nx.read_out(qt, vt, temperature=1.0 / beta, subset=sub, keys=kt).backward(torch.from_numpy(gh))
        _bits_equal(kt.grad.numpy(), nx.key_gradient(qh, grad_values=gh, temperature=1.0 / beta, subset=sub), "K.grad through the host")
        assert qt.grad.shape == (nq, 65) and vt.grad.shape == (len(x), 70)
    # within the bound with the node's own forward words: log_rel and the values are the host fold of the shards' (their error: `fold`
    # and `vb`, as derived for the read-out gradient's node test)
    for res, e in ((got, None), (got_sub, elig)):
        n = len(x) if e is None else e.sum(axis=1)
        fold = 2 * (P.device_bound(np.zeros((nq, 1)), None, None, beta, n, dot=False) + 4 * P.U * (1 + np.log(len(x)))) + 2 * P.U
        Sv = PM.weights(q.astype(np.float64) @ x.astype(np.float64).T, beta, e)[0] @ np.abs(v).astype(np.float64)
        vb = R.device_bound(q, x, v, "float16", beta, e, dot=False) * (1 + fold[:, None]) + fold[:, None] * Sv
        _check(res, q, x, "float16", beta, a, g, v, e, what=f"node capacity {capacity}", values_bound=vb, rel_extra=fold)


# ---- autograd: log_z and read_out with keys --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_fills_the_keys_gradient(dtype):
    q, x = gauss_case(65, 13, n=300, nq=257)
    rng = np.random.default_rng(6)
    v = rng.standard_normal((300, 70)).astype(np.float32)
    a, g = rng.standard_normal(257).astype(np.float32), rng.standard_normal((257, 70)).astype(np.float32)
    beta = 1.0 / 8.0
    xr, qr, vr = (torch.from_numpy(round_store(t, dtype)).cuda().double() for t in (x, q, v))
    with _index(x, dtype) as ix:
        keys = torch.from_numpy(round_store(x, dtype)).float().cuda().requires_grad_()  # the caller states that this is the store
        # log_z
        qd = _dev(q).requires_grad_(True)
        ix.log_z(qd, 1.0 / beta, keys=keys).backward(_dev(a))
        q0 = _dev(q).requires_grad_(True)
        ix.log_z(q0, 1.0 / beta).backward(_dev(a))
        _bits_equal(qd.grad.cpu().numpy(), q0.grad.cpu().numpy(), "q.grad of log_z is what it was")
        k_logz = keys.grad.cpu().numpy()
        _bits_equal(k_logz, _kg(ix, q, beta, a)[0], "K.grad of log_z is the explicit call")
        x64 = xr.clone().requires_grad_(True)
        (torch.logsumexp(beta * (qr @ x64.T), dim=1) * _dev(a).double()).sum().backward()
        err = np.abs(k_logz.astype(np.float64) - x64.grad.cpu().numpy())
        bound = K.device_bound(q, x, dtype, beta, a, dot=True)
        print(f"autograd log_z {dtype}: K.grad max err / bound = {(err / bound).max():.3e}")
        assert (err <= bound).all()
        # read_out
        keys.grad = None
        qd, vd = _dev(q).requires_grad_(True), _dev(v).requires_grad_(True)
        ix.read_out(qd, vd, 1.0 / beta, keys=keys).backward(_dev(g))
        q0, v0 = _dev(q).requires_grad_(True), _dev(v).requires_grad_(True)
        ix.read_out(q0, v0, 1.0 / beta).backward(_dev(g))
        _bits_equal(qd.grad.cpu().numpy(), q0.grad.cpu().numpy(), "q.grad of read_out is what it was")
        _bits_equal(vd.grad.cpu().numpy(), v0.grad.cpu().numpy(), "V.grad of read_out is what it was")
        k_ro = keys.grad.cpu().numpy()
        x64 = xr.clone().requires_grad_(True)
        ((torch.softmax(beta * (qr @ x64.T), dim=1) @ vr) * _dev(g).double()).sum().backward()
        err = np.abs(k_ro.astype(np.float64) - x64.grad.cpu().numpy())
        bound = K.device_bound(q, x, dtype, beta, None, g, v, dot=True)
        print(f"autograd read_out {dtype}: K.grad max err / bound = {(err / bound).max():.3e}")
        assert (err <= bound).all()
        # keys that do not require grad run no key-gradient scan; a 16-bit `keys` gets a gradient of its dtype
        calls = {"n": 0}
        real = ix.key_gradient

        def counted(*args, **kw):
            calls["n"] += 1
            return real(*args, **kw)

        ix.key_gradient = counted
        q3 = _dev(q).requires_grad_(True)
        ix.log_z(q3, 1.0 / beta, keys=keys.detach()).backward(_dev(a))
        ix.read_out(q3, _dev(v), 1.0 / beta, keys=keys.detach()).backward(_dev(g))
        assert calls["n"] == 0
        kh = keys.detach().to(TDT[dtype]).requires_grad_()
        ix.log_z(_dev(q), 1.0 / beta, keys=kh).backward(_dev(a))
        assert calls["n"] == 1 and kh.grad.dtype == TDT[dtype] and torch.equal(kh.grad, torch.from_numpy(k_logz).cuda().to(TDT[dtype]))
        del ix.key_gradient
        with pytest.raises(ValueError, match="tensor temperature"):
            ix.log_z(_dev(q), torch.tensor(8.0, device="cuda"), keys=keys)
        with pytest.raises(ValueError, match="keys"):
            ix.log_z(_dev(q), 8.0, keys=keys[:299])
        with pytest.raises(ValueError, match="keys"):
            ix.read_out(_dev(q), _dev(v), 8.0, keys=np.zeros((300, 65), dtype=np.float32))


# ---- refusals and empty cases ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex, LogPartition, PosteriorExpectation

    lib = _native.load_library()
    q, x, v, a, g = _int_case(65)
    x, v, a, g = x[:600], v[:600, :5], a[:5], g[:5, :5]
    qd, ad, gd = _dev(q[:5]), _dev(a), _dev(g)
    words = torch.zeros((2, 5), device="cuda")
    yd = torch.zeros((5, 5), device="cuda")
    out = torch.full((600, 65), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    opt = lambda t: None if t is None else ptr(t)  # noqa: E731

    def raw(h, queries=qd, code=2, nq=5, beta=1.0, lab=None, n_lab=0, m=words[0], r=words[1], av=ad, y=None, gv=None, acc=0, o=out):
        return lib.vodhip_index_posterior_key_gradient(h, opt(queries), code, nq, ctypes.c_float(beta), opt(lab), n_lab, opt(m), opt(r), opt(av), opt(y),
                                                       opt(gv), acc, opt(o), None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    fake = LogPartition(words[0], words[0], words[1])
    fake_pe = PosteriorExpectation(yd, fake)
    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x, "float16") as ix:
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        refused(raw(ix._h, m=None), "invalid query / output pointers")
        refused(raw(ix._h, r=None), "invalid query / output pointers")
        refused(raw(ix._h, av=None), "grad_log_z and grad_values are both NULL")
        refused(raw(ix._h, av=None, y=yd), "grad_log_z and grad_values are both NULL")
        refused(raw(ix._h, gv=gd), "grad_values without values")
        refused(raw(ix._h, y=yd, gv=gd), "grad_values needs a value table")
        refused(raw(ix._h, o=None), "out is NULL")
        refused(raw(ix._h, nq=-1), "invalid query / output pointers")
        refused(raw(ix._h, code=3), "invalid q_dtype 3")
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            refused(raw(ix._h, beta=beta), "beta must be finite and > 0")
        refused(raw(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=2), "set the row labels first")
        with pytest.raises(_native.NativeLibraryError, match="both NULL"):
            ix.key_gradient(qd, log_partition=fake)
        with pytest.raises(_native.NativeLibraryError, match="grad_values needs a value table"):
            ix.key_gradient(qd, grad_values=gd, log_partition=fake)
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            ix.key_gradient(qd, grad_log_z=ad, log_partition=fake, temperature=float("nan"))
        with pytest.raises(ValueError, match="grad_log_z"):
            ix.key_gradient(qd, grad_log_z=ad[:4], log_partition=fake)
        with pytest.raises(ValueError, match="max_score"):
            ix.key_gradient(qd, grad_log_z=ad, log_partition=LogPartition(words[0, :4], words[0, :4], words[1, :4]))
        with pytest.raises(ValueError, match="out"):
            ix.key_gradient(qd, grad_log_z=ad, log_partition=fake, out=torch.zeros((599, 65), device="cuda"))
        with pytest.raises(ValueError, match="accumulate"):
            ix.key_gradient(qd, grad_log_z=ad, log_partition=fake, accumulate=True)
        ix.set_row_values(v)
        with pytest.raises(ValueError, match="grad_values"):
            ix.key_gradient(qd, grad_values=gd[:, :4], expectation=fake_pe)
        torch.cuda.synchronize()
        assert (out == 123.0).all()  # a refused call writes nothing
        # nq == 0 follows the adjoint: accumulating leaves `out` alone, the plain call zero-fills it
        assert raw(ix._h, queries=None, nq=0, m=None, r=None, acc=1) == 0
        torch.cuda.synchronize()
        assert (out == 123.0).all()
        assert raw(ix._h, queries=None, nq=0, m=None, r=None) == 0
        torch.cuda.synchronize()
        assert (out.view(torch.int32) == 0).all()
        empty = ix.key_gradient(torch.zeros((0, 65), device="cuda"), grad_log_z=torch.zeros((0,), device="cuda"))
        assert empty.shape == (600, 65) and (empty == 0).all()
        got, _ = _kg(ix, q[:5], 1.0 / 64.0, a, g)
        _check(got, q[:5], x, "float16", 1.0 / 64.0, a, g, v, what="after the refusals")
    with _index(x[:300], "float16", capacity=600) as ix:
        ix.set_row_values(v[:300])
        ix.add(x[300:303])  # the table no longer matches the rows
        with pytest.raises(_native.NativeLibraryError, match="set the table again"):
            ix.key_gradient(qd, grad_values=gd, expectation=fake_pe)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        refused(raw(ix._h), "posterior_key_gradient is not supported on an L2 index")
        with pytest.raises(_native.NativeLibraryError, match="posterior_key_gradient is not supported on an L2 index"):
            ix.key_gradient(qd, grad_log_z=ad, log_partition=fake)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        refused(raw(ix._h), "VODHIP_EXACT_F32")
        assert "posterior_key_gradient" in lib.vodhip_last_error().decode()
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty index: a no-op that returns no rows
        assert raw(ix._h) == 0
        assert ix.key_gradient(qd, grad_log_z=ad).shape == (0, 65)
    torch.cuda.synchronize()
    host_fake = LogPartition(np.zeros(5, np.float32), np.zeros(5, np.float32), np.zeros(5, np.float32))
    qh, ah, gh = np.array(q[:5]), np.array(a), np.array(g)
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        nx.add(x.astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            nx.key_gradient(qh, grad_log_z=ah, log_partition=host_fake, temperature=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.key_gradient(qh, grad_log_z=ah, log_partition=host_fake, subset=np.zeros((5, 2), dtype=np.int32))
        with pytest.raises(_native.NativeLibraryError, match="both NULL"):
            nx.key_gradient(qh, log_partition=host_fake)
        with pytest.raises(_native.NativeLibraryError, match="grad_values needs a value table"):
            nx.key_gradient(qh, grad_values=gh, log_partition=host_fake)
        empty = nx.key_gradient(np.zeros((0, 65), dtype=np.float32), grad_log_z=np.zeros(0, dtype=np.float32))
        assert empty.shape == (600, 65) and (empty == 0).all()
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:  # (a node index is never an L2 index: its constructor refuses the metric)
        with pytest.raises(_native.NativeLibraryError, match="posterior_key_gradient.*VODHIP_EXACT_F32"):
            nx.key_gradient(qh, grad_log_z=ah, log_partition=host_fake)
