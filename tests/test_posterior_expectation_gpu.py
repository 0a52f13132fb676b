"""`HipFlatIndex.posterior_expectation` / `HipNodeIndex.posterior_expectation` on the GPU against the float64 restatement
(tests/readout_ref.py); every element of every case is compared against `readout_ref.device_bound`, which is derived, not fitted.

Integer data (values in [-8, 8]: exact in fp16 and bf16, every score an exact integer in float32, so the bound's dot-product part is
dropped): stores of 1, 5, 255, 256, 257 and 1500 rows and one on each side of a group boundary (RGR = VODHIP_READOUT_GROUP_ROWS) and
two groups plus a partial tile, dims 1, 64, 65, 768, value widths at every slice count and its edges, batches 1, 64, 65, 129, 300,
beta 1, 1/64, 4; `max_score` and `log_rel` carry the bits of `log_partition` on the same index in every call.  Then: one-hot
posteriors (the row order of the transposed reads on the value table), the running maximum (rising, falling, dead tiles, underflowing
gamma, -inf and +inf scores), a column of ones, one-hot class tables, the stored rows as values against `posterior_mean`, subset labels,
Gaussian data within the full bound, a NaN in the table, batch independence, a call beside a search in flight, the node index, refusals.
Measured maxima (MI355X): DESIGN.md 4 "Posterior read-out" and profiles/posterior_expectation.json.
"""
import ctypes
import functools

import numpy as np
import pytest

import posterior_ref as PM
import readout_ref as R
from test_l2_cpu import GAUSS_CASES, gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
RGR = R.GROUP_ROWS
STORES = [1, 5, 255, 256, 257, 1500, RGR - 1, RGR + 1, 2 * RGR + 5]
DIMS = [1, 64, 65, 768]
WIDTHS = [1, 63, 64, 65, 128, 129, 192, 193, 256]
BATCHES = [1, 64, 65, 129, 300]
BETAS = [1.0, 1.0 / 64.0, 4.0]
N_MAX = 2 * RGR + 5


def _index(x, dtype="float16", capacity=None, dim=None, **kw):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, **kw)
    if len(x):
        ix.add(x)
    return ix


@functools.lru_cache(maxsize=None)
def _int_case(d, n=N_MAX, nq=300):
    """integer rows / queries / values; the same for both store dtypes (both hold the values exactly); every score is exact in float32"""
    rng = np.random.default_rng(9000 + d + n)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    v = rng.integers(-8, 9, size=(n, 256)).astype(np.float32)
    for a in (q, x, v):
        a.setflags(write=False)
    return q, x, v


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _pe(ix, q, beta=1.0, **kw):
    """(values, log_z, max_score, log_rel) as NumPy, and the bits of log_partition on the same index are asserted equal"""
    qd = _dev(q)
    r = ix.posterior_expectation(qd, temperature=1.0 / beta, **kw)
    lp = ix.log_partition(qd, temperature=1.0 / beta, **kw)
    assert r.values.dtype == torch.float32 and r.values.shape == (len(q), ix.row_values_shape[1]) and r.values.is_cuda
    for a, b in zip(r.log_partition, lp):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return (r.values.cpu().numpy(),) + tuple(t.cpu().numpy() for t in r.log_partition)


def _check(got, q, x, v, dtype, beta, eligible=None, dot=False, what="", cols=None):
    """every (query, column) within the derived bound; queries without a finite log Z: the zero row"""
    val = got[0]
    ref, rm, _ = R.posterior_expectation(q, x, v, dtype, beta, eligible)
    bound = R.device_bound(q, x, v, dtype, beta, eligible, dot=dot)
    live = np.isfinite(rm)
    assert np.array_equal(np.isfinite(got[2]), live), what
    assert (val[~live] == 0).all(), what
    err = np.abs(val.astype(np.float64) - ref)
    if cols is not None:
        err, bound = err[:, cols], bound[:, cols]
    ratio = np.divide(err[live], bound[live], out=np.zeros_like(err[live]), where=bound[live] > 0).max() if live.any() else 0.0
    print(f"{what}: max |value - float64| = {err[live].max() if live.any() else 0.0:.3e}, max err / bound = {ratio:.3e}")
    assert not np.isnan(err[live]).any(), what
    assert (err[live] <= bound[live]).all(), (what, ratio)
    return ratio


def _bits_equal(a, b, what=""):
    for u, w in zip(a, b):
        assert np.array_equal(u.view(np.uint32), w.view(np.uint32)), what


# ---- sizes, dims, widths, batches, betas on integer data ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_with_every_width(n, dtype):
    d = DIMS[STORES.index(n) % len(DIMS)]
    q, x, v = _int_case(d)
    x, v = x[:n], v[:n]
    with _index(x, dtype) as ix:
        for k, w in enumerate(WIDTHS):
            beta = BETAS[(k + STORES.index(n)) % 3]
            ix.set_row_values(v[:, :w])
            assert ix.row_values_shape == (n, w)
            full = _pe(ix, q, beta)
            _check(full, q, x, v[:, :w], dtype, beta, what=f"n {n} d {d} w {w} {dtype} beta {beta:g}")
            nq = BATCHES[k % 4]
            _bits_equal(_pe(ix, q[:nq], beta), [a[:nq] for a in full], (n, w, nq))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_dims_with_every_width_batch_and_beta(d, dtype):
    q, x, v = _int_case(d)
    x, v = x[:1500], v[:1500]
    with _index(x, dtype) as ix:
        for k, w in enumerate(WIDTHS):
            ix.set_row_values(v[:, :w])
            full = {}
            for beta in BETAS if k % 4 == 0 else [BETAS[k % 3]]:
                full[beta] = _pe(ix, q, beta)
                _check(full[beta], q, x, v[:, :w], dtype, beta, what=f"d {d} w {w} {dtype} beta {beta:g}")
            beta = next(iter(full))
            for nq in BATCHES[:-1] if k % 4 == 0 else [BATCHES[k % 4]]:
                _bits_equal(_pe(ix, q[:nq], beta), [a[:nq] for a in full[beta]], (d, w, nq))


# ---- one-hot posteriors: the row order of the transposed reads on the value table ---------------------------------------------------
TOPS = [1, 5, 70, 78 + 4, 147, 154 + 36, 200, 252, 256 + 9, 256 + 64 + 13, 256 + 128 + 50, 256 + 192 + 31, 512 + 3, 512 + 22, 512 + 47, 599]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("w", [65, 256])
def test_one_hot_posterior_returns_the_top_rows_values(w, dtype):
    assert {((t % 256) // 64, (t % 8) // 4) for t in TOPS} == {(a, h) for a in range(4) for h in range(2)}  # 4 row waves x 2 lane halves
    d, n = 65, 600
    rng = np.random.default_rng(w)
    x = rng.integers(-1, 2, size=(n, d)).astype(np.float32)
    q = rng.integers(-1, 2, size=(len(TOPS), d)).astype(np.float32)
    v = rng.integers(-8, 9, size=(n, w)).astype(np.float32)
    v[:, 0] = np.arange(n) % 17  # a column that tells neighbouring rows apart
    x[:, : len(TOPS)] = 0
    q[:, : len(TOPS)] = 0
    for i, t in enumerate(TOPS):  # query i scores row t 2048 + .., every other row at most d: a margin above 512
        x[t, i] = 8
        q[i, i] = 256
    s = q.astype(np.float64) @ x.astype(np.float64).T
    assert (np.argmax(s, axis=1) == TOPS).all() and (np.sort(s, axis=1)[:, -1] - np.sort(s, axis=1)[:, -2] >= 512).all()
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        got = _pe(ix, q, 64.0)
    tol = n * np.exp(-64.0) * 16 + 2.0 ** -22 * np.abs(v[TOPS])
    np.testing.assert_array_less(np.abs(got[0] - v[TOPS]), tol + 1e-30)
    _check(got, q, x, v, dtype, 64.0, what=f"one-hot w {w} {dtype}")


# ---- the running maximum ----------------------------------------------------------------------------------------------------------------
N_RUN = RGR + 3 * 256 + 40  # group 0 (RGR / 256 tiles), then three full tiles and a partial one of group 1
T_RUN = (N_RUN + 255) // 256


def _run_case(offsets, seed=3):
    """rows whose score against every query is offsets[tile] + a small integer: column 0 carries the tile's offset, q[:, 0] = 1"""
    rng = np.random.default_rng(seed)
    d = 8
    x = rng.integers(-1, 2, size=(N_RUN, d)).astype(np.float32)
    q = rng.integers(-1, 2, size=(70, d)).astype(np.float32)
    q[:, 0] = 1
    x[:, 0] = np.repeat(np.asarray(offsets, dtype=np.float32), 256)[:N_RUN]
    v = rng.integers(-8, 9, size=(N_RUN, 129)).astype(np.float32)
    return q, x, v


RUN_CASES = {
    "rising": [2.0 * t for t in range(T_RUN)],                      # every tile raises the maximum: a rescale per tile
    "falling": [-2.0 * t for t in range(T_RUN)],                    # gamma < 1 in every tile behind the first of a group
    "zigzag": [(-7.0) ** (t % 3) for t in range(T_RUN)],
    "gamma underflows": [0.0, 0.0, -200.0, 0.0, -120.0] + [0.0] * (T_RUN - 7) + [-300.0, 0.0],   # more than 104 / beta below M
    "a late tile towers": [0.0] * (T_RUN - 2) + [150.0, 0.0],       # the rescale factor underflows: what came before vanishes
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(RUN_CASES))
def test_running_maximum(case, dtype):
    assert T_RUN >= RGR // 256 + 3
    q, x, v = _run_case(RUN_CASES[case])
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        for beta in (1.0, 0.25):
            got = _pe(ix, q, beta)
            assert np.isfinite(got[0]).all()
            _check(got, q, x, v, dtype, beta, what=f"running maximum, {case}, {dtype} beta {beta:g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dead", [(0,), (0, 1), (3,), (RGR // 256,), (2, RGR // 256 + 1), tuple(range(RGR // 256))])
def test_tiles_without_an_eligible_row(dead, dtype):
    """dead tiles by subset labels (no eligible row) and, in a second store, by -inf scores (eligible rows, a maximum of -inf)"""
    q, x, v = _run_case([float(t % 3) for t in range(T_RUN)])
    tile = np.arange(N_RUN) // 256
    is_dead = np.isin(tile, dead)
    labels = np.where(is_dead, 1, 0).astype(np.int32)
    sub = np.zeros((len(q), 1), dtype=np.int32)
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        ix.set_row_labels(labels)
        got = _pe(ix, q, 1.0, subset=sub)
        assert np.isfinite(got[0]).all()
        _check(got, q, x, v, dtype, 1.0, np.broadcast_to(~is_dead, (len(q), N_RUN)), what=f"dead tiles {dead} by labels, {dtype}")
    xi = np.array(x)
    xi[is_dead, 0] = -np.inf
    with _index(xi, dtype) as ix:
        ix.set_row_values(v)
        got = _pe(ix, q, 1.0)
        assert np.isfinite(got[0]).all()
        _check(got, q, xi, v, dtype, 1.0, what=f"dead tiles {dead} by -inf scores, {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_rows_minus_inf_and_a_plus_inf_score(dtype):
    q, x, v = _run_case([0.0] * T_RUN)
    xm = np.array(x)
    xm[:, 0] = -np.inf
    with _index(xm, dtype) as ix:
        ix.set_row_values(v)
        val, log_z, m, r = _pe(ix, q, 1.0)
    assert np.isneginf(m).all() and np.isneginf(r).all() and (val == 0).all()
    for row in (5, RGR + 300):
        xp = np.array(x)
        xp[row, 0] = np.inf
        with _index(xp, dtype) as ix:
            ix.set_row_values(v)
            val, log_z, m, r = _pe(ix, q, 1.0)
        assert np.isposinf(m).all() and np.isposinf(r).all() and (val == 0).all()


# ---- consistency -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_of_ones_reads_one(dtype):
    q, x, _ = _int_case(65)
    x = x[:3000]
    ones = np.ones((len(x), 1), dtype=np.float32)
    for beta in (1.0 / 64.0, 1.0):
        with _index(x, dtype) as ix:
            ix.set_row_values(ones[:, 0])  # a vector is one column
            assert ix.row_values_shape == (3000, 1)
            got = _pe(ix, q[:129], beta)
        bound = R.device_bound(q[:129], x, ones, dtype, beta, dot=False)[:, 0]
        assert (np.abs(got[0][:, 0].astype(np.float64) - 1.0) <= bound).all()
        _check(got, q[:129], x, ones, dtype, beta, what=f"ones column {dtype} beta {beta:g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_classes", [3, 64, 200])
def test_one_hot_class_table_reads_the_class_masses(n_classes, dtype):
    q, x, _ = _int_case(65)
    x, q = x[:3000], q[:129]
    cls = np.random.default_rng(n_classes).integers(0, n_classes, size=len(x))
    table = np.eye(n_classes, dtype=np.float32)[cls]
    beta = 1.0 / 16.0
    p, _, _ = PM.weights(q.astype(np.float64) @ x.astype(np.float64).T, beta)
    mass = np.stack([p[:, cls == c].sum(axis=1) for c in range(n_classes)], axis=1)
    with _index(x, dtype) as ix:
        ix.set_row_values(table)
        got = _pe(ix, q, beta)
    bound = R.device_bound(q, x, table, dtype, beta, dot=False)
    assert (np.abs(got[0].astype(np.float64) - mass) <= bound).all()
    assert (np.abs(got[0].astype(np.float64).sum(axis=1) - 1.0) <= bound.sum(axis=1)).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 256])
def test_the_stored_rows_as_values_agree_with_posterior_mean(d, dtype):
    rng = np.random.default_rng(d)
    x = rng.integers(-8, 9, size=(3000, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(129, d)).astype(np.float32)
    for beta in (1.0 / 64.0, 1.0):
        with _index(x, dtype) as ix:
            ix.set_row_values(x)
            got = _pe(ix, q, beta)
            mean = ix.posterior_mean(_dev(q), temperature=1.0 / beta).mean.cpu().numpy()
        both = R.device_bound(q, x, x, dtype, beta, dot=False) + PM.device_bound(q, x, dtype, beta, dot=False)
        assert (np.abs(got[0].astype(np.float64) - mean.astype(np.float64)) <= both).all()
        _check(got, q, x, x, dtype, beta, what=f"rows as values d {d} {dtype} beta {beta:g}")


# ---- masks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 132])
def test_subset_labels(nq, dtype):
    q, x, v = _int_case(65)
    x, v = x[:3000], v[:3000, :70]
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        ix.set_row_values(v)
        for beta in (1.0, 1.0 / 64.0):
            got = _pe(ix, q[:nq], beta, subset=sub)
            _check(got, q[:nq], x, v, dtype, beta, elig, what=f"subset nq {nq} {dtype} beta {beta:g}")
            assert (got[0][3::4] == 0).all() and np.isneginf(got[1][3::4]).all()  # no eligible row: the zero row
        _check(_pe(ix, q[:nq], 1.0), q[:nq], x, v, dtype, 1.0, what="row labels without query labels")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_in_the_table_poisons_its_column_alone(dtype):
    q, x, v = _int_case(65)
    q, x = q[:70], x[:3000]
    v = np.array(v[:3000, :130])
    labels = np.zeros(len(x), dtype=np.int32)
    labels[[7, 2500]] = 1  # the two rows are excluded for every query
    v[7, 3] = np.nan
    v[2500, 129] = np.inf
    sub = np.zeros((len(q), 1), dtype=np.int32)
    elig = np.broadcast_to(labels == 0, (len(q), len(x)))
    clean = np.ones(130, dtype=bool)
    clean[[3, 129]] = False
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        ix.set_row_values(v)
        got = _pe(ix, q, 1.0 / 64.0, subset=sub)  # (the two scalar words: log_partition's bits, asserted inside)
    assert np.isnan(got[0][:, ~clean]).all() and np.isfinite(got[0][:, clean]).all()
    _check(got, q, x, np.where(np.isfinite(v), v, 0), dtype, 1.0 / 64.0, elig, what=f"NaN in the table {dtype}", cols=clean)


# ---- one order -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,w", [(65, 64), (768, 193)])
def test_a_query_has_the_same_bits_in_any_batch_and_on_every_repeat(d, w, dtype):
    q, x, v = _int_case(d)
    rng = np.random.default_rng(d)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)  # inexact sums: the order matters
    qg = (q + rng.standard_normal(q.shape)).astype(np.float32)
    vg = (v[:, :w] + rng.standard_normal((len(v), w))).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(xg, dtype) as ix:
        ix.set_row_values(vg)
        a = _pe(ix, qg, beta)
        _bits_equal(a, _pe(ix, qg, beta))
        _bits_equal([u[:64] for u in a], _pe(ix, qg[:64], beta))
        _bits_equal([u[:65] for u in a], _pe(ix, qg[:65], beta))
        for j in (0, 63, 64, 217, 299):
            _bits_equal([u[j : j + 1] for u in a], _pe(ix, qg[j : j + 1], beta), j)
    assert not np.isnan(a[0]).any()


# ---- Gaussian data: the full bound, every element -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    v = np.random.default_rng(seed).standard_normal((len(x), 100)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(dim)))  # the float32 the call receives
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        got = _pe(ix, q, beta)
    _check(got, q, x, v, dtype, beta, dot=True, what=f"gaussian dim {dim} {dtype}")


# ---- table sources -----------------------------------------------------------------------------------------------------------------------
def test_tables_from_numpy_and_torch_on_host_and_device_read_the_same():
    q, x, v = _int_case(65)
    q, x, v = q[:65], x[:700], v[:700, :66]
    with _index(x, "float16") as ix:
        results = []
        for table in (v, v.astype(np.float16), torch.from_numpy(np.array(v)), _dev(v), _dev(v).half(), _dev(v).bfloat16(), _dev(v).double()):
            ix.set_row_values(table)
            results.append(_pe(ix, q, 1.0 / 64.0))
        for other in results[1:]:
            _bits_equal(results[0], other)
        ix.set_row_values(None)
        assert ix.row_values_shape is None


# ---- beside searches ---------------------------------------------------------------------------------------------------------------------
def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x, v = _int_case(768)
    qd = _dev(q[:129])
    with _index(x[:3000], "float16") as ix:
        ix.set_row_values(v[:3000, :129])
        serial_s, serial_i = ix.search(qd, 100)
        serial = ix.posterior_expectation(qd, temperature=64.0)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            pe = ix.posterior_expectation(qd, temperature=64.0)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert torch.equal(pe.values.view(torch.int32), serial.values.view(torch.int32))
        for a, b in zip(pe.log_partition, serial.log_partition):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert ix.get_stat("last_overflow") == 0


# ---- node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards,capacity", [(2, 3000), (3, 3000), (3, 12000)])
def test_node_index_folds_the_shards(n_shards, capacity):
    import partition_ref as P
    from vod_amd.index import HipNodeIndex

    q, x, v = _int_case(65)
    x, v = x[:3000], v[:3000, :70]
    nq, beta = 129, 1.0 / 64.0
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, "float16") as ix:
        ix.set_row_values(v)
        flat = _pe(ix, q[:nq], beta)
        ix.set_row_labels(labels)
        flat_sub = _pe(ix, q[:nq], beta, subset=sub)
    with HipNodeIndex(65, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        nx.add(x.astype(np.float32))
        assert nx.row_values_shape is None
        nx.set_row_values(v)
        assert nx.row_values_shape == (3000, 70)
        got = nx.posterior_expectation(np.array(q[:nq]), temperature=1.0 / beta)
        nx.set_row_labels(labels)
        got_sub = nx.posterior_expectation(np.array(q[:nq]), temperature=1.0 / beta, subset=sub)
    for res, ref, e in ((got, flat, None), (got_sub, flat_sub, elig)):
        val, lp = res
        assert isinstance(val, np.ndarray) and val.dtype == np.float32 and val.shape == (nq, 70)
        assert np.array_equal(lp.max_score.view(np.uint32), ref[2].view(np.uint32))  # max_score: the flat index's bits
        want, rm, _ = R.posterior_expectation(q[:nq], x, v, "float16", beta, e)
        live = np.isfinite(rm)
        # every shard is within the flat bound of its own rows (each shard's S adds up to the store's); the fold's weights use float32
        # (max, log_rel) pairs - log_rel within PB + 4 u (1 + log n) of the truth, as in the partition fold - and the result rounds once
        n = len(x) if e is None else e.sum(axis=1)
        fold = 2 * (P.device_bound(np.zeros((nq, 1)), None, None, beta, n, dot=False) + 4 * P.U * (1 + np.log(len(x)))) + 2 * P.U
        S = PM.weights(q[:nq].astype(np.float64) @ x.astype(np.float64).T, beta, e)[0] @ np.abs(v).astype(np.float64)
        bound = R.device_bound(q[:nq], x, v, "float16", beta, e, dot=False) * (1 + fold[:, None]) + fold[:, None] * S
        err = np.abs(val.astype(np.float64) - want)
        assert (err[live] <= bound[live]).all(), (err[live] / bound[live]).max()
        assert (val[~live] == 0).all() and np.isneginf(lp.log_z[~live]).all() and not np.isnan(val).any()


# ---- refusals and empty cases ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    q, x, v = _int_case(65)
    x, v = x[:600], v[:600, :5]
    qd = _dev(q[:5])
    out = torch.full((2, 5), 123.0, device="cuda")
    out_val = torch.full((5, 5), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(h, queries=qd, code=2, nq=5, beta=1.0, lab=None, n_lab=0, om=out[0], ol=out[1], val=out_val):
        return lib.vodhip_index_posterior_expectation(h, None if queries is None else ptr(queries), code, nq, ctypes.c_float(beta),
                                                      None if lab is None else ptr(lab), n_lab, None if om is None else ptr(om),
                                                      None if ol is None else ptr(ol), None if val is None else ptr(val), None)

    def set_raw(h, table, n_rows, n_cols, code=2, location=0):
        return lib.vodhip_index_set_row_values(h, table.ctypes.data, n_rows, n_cols, code, location, None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    wide = np.zeros((300, 257), dtype=np.float32)
    with _index(x[:300], "float16", capacity=600) as ix:
        refused(raw(ix._h), "no value table")
        with pytest.raises(_native.NativeLibraryError, match="no value table"):
            ix.posterior_expectation(qd)
        refused(set_raw(ix._h, wide, 300, 257), "n_cols=257")
        refused(set_raw(ix._h, wide, 300, 0), "n_cols=0")
        refused(set_raw(ix._h, wide, 299, 5), "n_rows=299, ntotal=300")
        refused(set_raw(ix._h, wide, 301, 5), "n_rows=301, ntotal=300")
        refused(set_raw(ix._h, wide, 300, 5, code=3), "invalid src_dtype 3")
        refused(set_raw(ix._h, wide, 300, 5, location=2), "invalid location 2")
        refused(lib.vodhip_index_set_row_values(None, wide.ctypes.data, 300, 5, 2, 0, None), "index is NULL")
        assert ix.row_values_shape is None
        with pytest.raises(_native.NativeLibraryError, match="n_rows=600, ntotal=300"):
            ix.set_row_values(v)
        ix.set_row_values(v[:300])
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        refused(raw(ix._h, om=None), "invalid query / output pointers")
        refused(raw(ix._h, ol=None), "invalid query / output pointers")
        refused(raw(ix._h, val=None), "invalid query / output pointers")
        refused(raw(ix._h, nq=-1), "invalid query / output pointers")
        refused(raw(ix._h, code=3), "invalid q_dtype 3")
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            refused(raw(ix._h, beta=beta), "beta must be finite and > 0")
        refused(raw(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=2), "set the row labels first")
        ix.add(x[300:])  # rows behind the table: it is short now
        refused(raw(ix._h), "the value table holds 300 rows, the index 600")
        with pytest.raises(_native.NativeLibraryError, match="holds 300 rows, the index 600"):
            ix.posterior_expectation(qd)
        torch.cuda.synchronize()
        assert (out == 123.0).all() and (out_val == 123.0).all()  # a refused call writes nothing
        ix.set_row_values(v)
        assert raw(ix._h, queries=None, nq=0, om=None, ol=None, val=None) == 0  # nq == 0: returns 0, needs nothing, writes nothing
        torch.cuda.synchronize()
        assert (out == 123.0).all() and (out_val == 123.0).all()
        empty = ix.posterior_expectation(torch.zeros((0, 65), device="cuda"))
        assert empty.values.shape == (0, 5) and all(t.shape == (0,) for t in empty.log_partition)
        _check(_pe(ix, q[:5], 1.0), q[:5], x, v, "float16", 1.0, what="after the refusals")
        ix.reset()  # drops the table
        assert ix.row_values_shape is None
        ix.add(x)
        refused(raw(ix._h), "no value table")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        ix.set_row_values(v[:300])
        refused(raw(ix._h), "L2 index")
        with pytest.raises(_native.NativeLibraryError, match="L2 index"):
            ix.posterior_expectation(qd)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        ix.set_row_values(v[:300])
        refused(raw(ix._h), "VODHIP_EXACT_F32")
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            ix.posterior_expectation(qd)
    torch.cuda.synchronize()
    assert (out == 123.0).all() and (out_val == 123.0).all()  # the two refusals by index kind wrote nothing either
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty index with a table of no rows
        ix.set_row_values(np.zeros((0, 3), dtype=np.float32))
        val, log_z, m, r = _pe(ix, q[:5], 1.0)
        assert np.isneginf(m).all() and np.isneginf(r).all() and (val == 0).all() and val.shape == (5, 3)
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        nx.add(x.astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="no value table"):
            nx.posterior_expectation(np.array(q[:5]))
        with pytest.raises(_native.NativeLibraryError, match="n_rows=300, ntotal=600"):
            nx.set_row_values(v[:300])
        with pytest.raises(_native.NativeLibraryError, match="n_cols=257"):
            nx.set_row_values(np.zeros((600, 257), dtype=np.float32))
        nx.set_row_values(v)
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            nx.posterior_expectation(np.array(q[:5]), temperature=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.posterior_expectation(np.array(q[:5]), subset=np.zeros((5, 2), dtype=np.int32))
        assert nx.posterior_expectation(np.zeros((0, 65), dtype=np.float32)).values.shape == (0, 5)
        got = nx.posterior_expectation(np.array(q[:5]))
        s = q[:5].astype(np.float64) @ x.astype(np.float64).T
        np.testing.assert_array_equal(got.log_partition.max_score, s.max(axis=1).astype(np.float32))
        nx.reset()
        assert nx.row_values_shape is None
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.posterior_expectation(np.array(q[:5]))
