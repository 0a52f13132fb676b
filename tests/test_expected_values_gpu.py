"""`posterior_expectation_backward` / `expected_values` of both indexes on the GPU against the float64 restatement
(tests/readout_grad_ref.py); every element of every case is compared against `readout_grad_ref.device_bound`, which is derived, not
fitted.

Integer data (rows, queries and table in [-8, 8], g integers in [-4, 4] times 2^-10: everything exact in fp16 and bf16, every score
an exact integer in float32, so the bound's dot-product part is dropped): stores of 1, 255, 257, RG + 1 and 2 RG + 5 rows (RG =
VODHIP_READOUT_GROUP_ROWS), table widths 1, 64, 65, 256, dims 1, 64, 65, 192, 193, 256, 257, 768 (the 192-column chunk and its narrow
last instantiations), batches 1, 64, 65, 129, 300, beta 1, 1/64, 4.  Then the running maximum (the read-out's cases), dead tiles and
infinite scores, a column of ones, zero gradient rows, the power-of-two scaling of g, subset labels, the three clauses of the
non-finite contract, batch invariance, Gaussian data within the full bound, autograd against the explicit call and against a float64
dense softmax, a call beside a search in flight, the node index, refusals.
Measured maxima (MI355X): DESIGN.md 4 "Read-out gradient" and profiles/expected_values.json.
"""
import ctypes
import functools

import numpy as np
import pytest

import partition_ref as P
import posterior_ref as PM
import readout_grad_ref as G
import readout_ref as R
from test_l2_cpu import GAUSS_CASES, gauss_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
DTYPES = ["float16", "bfloat16"]
RGR = R.GROUP_ROWS
STORES = [1, 255, 257, RGR + 1, 2 * RGR + 5]
WIDTHS = [1, 64, 65, 256]
DIMS = [1, 64, 65, 192, 193, 256, 257, 768]
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
    """integer rows / queries / table and a 16-bit-exact g; the same for both store dtypes"""
    rng = np.random.default_rng(7000 + d + n)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    v = rng.integers(-8, 9, size=(n, 256)).astype(np.float32)
    g = (rng.integers(-4, 5, size=(nq, 256)) * 2.0 ** -10).astype(np.float32)
    for a in (q, x, v, g):
        a.setflags(write=False)
    return q, x, v, g


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bw(ix, q, g, beta=1.0, expectation=None, **kw):
    """the gradient as NumPy float32 [nq, dim], and the forward it was given"""
    qd = _dev(q)
    pe = ix.posterior_expectation(qd, temperature=1.0 / beta, **kw) if expectation is None else expectation
    grad = ix.posterior_expectation_backward(qd, _dev(g), pe, temperature=1.0 / beta, **kw)
    assert grad.dtype == torch.float32 and grad.shape == (len(q), ix.dim) and grad.is_cuda
    return grad.cpu().numpy(), pe


def _check(got, q, x, v, g, dtype, beta, eligible=None, dot=False, what="", cols=None, **kw):
    """every (query, column) within the derived bound; queries without a finite log Z: the zero row"""
    ref, _, rm, _ = G.expected_values_grad(q, x, v, g, dtype, beta, eligible)
    bound = G.device_bound(q, x, v, g, dtype, beta, eligible, dot=dot, **kw)
    live = np.isfinite(rm)
    assert (got[~live].view(np.uint32) == 0).all(), what
    err = np.abs(got.astype(np.float64) - ref)
    if cols is not None:
        err, bound = err[:, cols], bound[:, cols]
    ratio = np.divide(err[live], bound[live], out=np.zeros_like(err[live]), where=bound[live] > 0).max() if live.any() else 0.0
    print(f"{what}: max |grad - float64| = {err[live].max() if live.any() else 0.0:.3e}, max err / bound = {ratio:.3e}")
    assert not np.isnan(err[live]).any(), what
    assert (err[live] <= bound[live]).all(), (what, ratio)
    return ratio


def _bits_equal(a, b, what=""):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# ---- sizes, widths, dims, batches, betas on integer data ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_with_every_width(n, dtype):
    d = [65, 193, 1, 768, 64][STORES.index(n)]
    q, x, v, g = _int_case(d)
    x, v = x[:n], v[:n]
    with _index(x, dtype) as ix:
        for k, w in enumerate(WIDTHS):
            beta = BETAS[(k + STORES.index(n)) % 3]
            ix.set_row_values(v[:, :w])
            full, _ = _bw(ix, q, g[:, :w], beta)
            _check(full, q, x, v[:, :w], g[:, :w], dtype, beta, what=f"n {n} d {d} w {w} {dtype} beta {beta:g}")
            nq = BATCHES[k]
            _bits_equal(_bw(ix, q[:nq], g[:nq, :w], beta)[0], full[:nq], (n, w, nq))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", DIMS)
def test_dims_with_every_width_batch_and_beta(d, dtype):
    q, x, v, g = _int_case(d)
    x, v = x[:1500], v[:1500]
    with _index(x, dtype) as ix:
        for k, w in enumerate(WIDTHS):
            ix.set_row_values(v[:, :w])
            full = {}
            for beta in BETAS if k == DIMS.index(d) % 4 else [BETAS[k % 3]]:
                full[beta], _ = _bw(ix, q, g[:, :w], beta)
                _check(full[beta], q, x, v[:, :w], g[:, :w], dtype, beta, what=f"d {d} w {w} {dtype} beta {beta:g}")
            beta = next(iter(full))
            for nq in BATCHES[:-1] if k == DIMS.index(d) % 4 else [BATCHES[(k + 1) % 4]]:
                _bits_equal(_bw(ix, q[:nq], g[:nq, :w], beta)[0], full[beta][:nq], (d, w, nq))


# ---- the running maximum: the read-out's cases ------------------------------------------------------------------------------------------
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
    g = (rng.integers(-4, 5, size=(70, 129)) * 2.0 ** -10).astype(np.float32)
    return q, x, v, g


RUN_CASES = {
    "rising": [2.0 * t for t in range(T_RUN)],                      # every tile raises the maximum: a rescale per tile
    "falling": [-2.0 * t for t in range(T_RUN)],                    # gamma < 1 in every tile behind the first of a group
    "zigzag": [(-7.0) ** (t % 3) for t in range(T_RUN)],
    "repeated": [float(3 * (t % 2)) for t in range(T_RUN)],         # the same maximum again and again: rescales by exactly 1
    "gamma underflows": [0.0, 0.0, -200.0, 0.0, -120.0] + [0.0] * (T_RUN - 7) + [-300.0, 0.0],   # more than 104 / beta below M
    "a late tile towers": [0.0] * (T_RUN - 2) + [150.0, 0.0],       # the rescale factor underflows: what came before vanishes
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(RUN_CASES))
def test_running_maximum(case, dtype):
    assert T_RUN >= RGR // 256 + 3
    q, x, v, g = _run_case(RUN_CASES[case])
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        for beta in (1.0, 0.25):
            got, _ = _bw(ix, q, g, beta)
            assert np.isfinite(got).all()
            _check(got, q, x, v, g, dtype, beta, what=f"running maximum, {case}, {dtype} beta {beta:g}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dead", [(0,), (0, 1), (3,), (RGR // 256,), (2, RGR // 256 + 1), tuple(range(RGR // 256))])
def test_tiles_without_an_eligible_row(dead, dtype):
    """dead tiles by subset labels (no eligible row) and, in a second store, by -inf scores (eligible rows, a maximum of -inf)"""
    q, x, v, g = _run_case([float(t % 3) for t in range(T_RUN)])
    tile = np.arange(N_RUN) // 256
    is_dead = np.isin(tile, dead)
    labels = np.where(is_dead, 1, 0).astype(np.int32)
    sub = np.zeros((len(q), 1), dtype=np.int32)
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        ix.set_row_labels(labels)
        got, _ = _bw(ix, q, g, 1.0, subset=sub)
        assert np.isfinite(got).all()
        _check(got, q, x, v, g, dtype, 1.0, np.broadcast_to(~is_dead, (len(q), N_RUN)), what=f"dead tiles {dead} by labels, {dtype}")
    xi = np.array(x)
    xi[is_dead, 0] = -np.inf
    xi[is_dead, 1:] = 0  # (a -inf entry makes the whole column NaN - H2m's contract - so the dead rows are the last word on column 0 only)
    with _index(xi, dtype) as ix:
        ix.set_row_values(v)
        got, _ = _bw(ix, q, g, 1.0)
        assert np.isnan(got[:, 0]).all() and np.isfinite(got[:, 1:]).all()  # column 0 holds the stored infinities
        _check(got, q, xi, v, g, dtype, 1.0, what=f"dead tiles {dead} by -inf scores, {dtype}", cols=np.arange(8) > 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_rows_minus_inf_and_a_plus_inf_score(dtype):
    q, x, v, g = _run_case([0.0] * T_RUN)
    xm = np.array(x)
    xm[:, 0] = -np.inf
    with _index(xm, dtype) as ix:
        ix.set_row_values(v)
        got, pe = _bw(ix, q, g, 1.0)
    assert torch.isneginf(pe.log_partition.max_score).all() and (got.view(np.uint32) == 0).all()
    for row in (5, RGR + 300):
        xp = np.array(x)
        xp[row, 0] = np.inf
        with _index(xp, dtype) as ix:
            ix.set_row_values(v)
            got, pe = _bw(ix, q, g, 1.0)
        assert torch.isposinf(pe.log_partition.max_score).all() and (got.view(np.uint32) == 0).all()  # no NaN anywhere


# ---- cancellation, zero rows, scaling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_column_of_ones_cancels(dtype):
    q, x, _, _ = _int_case(65)
    x, q = x[:3000], q[:129]
    ones = np.ones((len(x), 1), dtype=np.float32)
    g = np.random.default_rng(1).standard_normal((129, 1)).astype(np.float32)  # not exact in 16 bits
    for beta in (1.0 / 64.0, 1.0):
        with _index(x, dtype) as ix:
            ix.set_row_values(ones)
            got, _ = _bw(ix, q, g, beta)
        _check(got, q, x, ones, g, dtype, beta, what=f"ones column {dtype} beta {beta:g}")
        # against zero itself (the reference is zero up to float64 rounding): what is left is the forward's own error in y
        bound = G.device_bound(q, x, ones, g, dtype, beta, dot=False)
        assert (np.abs(got) <= bound + 1e-12).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_zero_gradient_row_gives_exact_zero_bits(dtype):
    q, x, v, g = _int_case(65)
    x, v, q = x[:3000], v[:3000, :70], q[:130]
    g = np.array(g[:130, :70])
    zero_rows = [0, 63, 64, 129]
    g[zero_rows] = 0
    g[5] = -0.0
    xn = np.array(x)
    xn[17, 3] = np.nan  # a stored NaN makes column 3 NaN for every scanned query: a zero g row is not scanned
    with _index(xn, dtype) as ix:
        ix.set_row_values(v)
        got, _ = _bw(ix, q, g, 1.0 / 64.0)
    assert (got[zero_rows + [5]].view(np.uint32) == 0).all()
    others = np.setdiff1d(np.arange(130), zero_rows + [5])
    assert np.isnan(got[others, 3]).all() and np.isfinite(np.delete(got[others], 3, axis=1)).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_scaling_g_by_a_power_of_two_scales_the_gradient_exactly(dtype):
    q, x = gauss_case(65, 21, n=3000, nq=70)
    rng = np.random.default_rng(2)
    v = rng.standard_normal((3000, 70)).astype(np.float32)
    g = rng.standard_normal((70, 70)).astype(np.float32)
    beta = 1.0 / 8.0
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        base, pe = _bw(ix, q, g, beta)
        for e in (-20, 7):
            scaled, _ = _bw(ix, q, g * np.float32(2.0 ** e), beta, expectation=pe)
            _bits_equal(scaled, base * np.float32(2.0 ** e), e)
        tiny, _ = _bw(ix, q, g * np.float32(1e-6), beta, expectation=pe)  # a loss gradient of 1e-6 does not flush, fp16 included
    _check(tiny, q, x, v, g * np.float32(1e-6), dtype, beta, dot=True, what=f"g of 1e-6 {dtype}")


# ---- masks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 132])
def test_subset_labels(nq, dtype):
    q, x, v, g = _int_case(65)
    x, v, g = x[:3000], v[:3000, :70], g[:, :70]
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        ix.set_row_values(v)
        for beta in (1.0, 1.0 / 64.0):
            got, _ = _bw(ix, q[:nq], g[:nq], beta, subset=sub)
            _check(got, q[:nq], x, v, g[:nq], dtype, beta, elig, what=f"subset nq {nq} {dtype} beta {beta:g}")
            assert (got[3::4].view(np.uint32) == 0).all()  # no eligible row: the zero row
        _check(_bw(ix, q[:nq], g[:nq], 1.0)[0], q[:nq], x, v, g[:nq], dtype, 1.0, what="row labels without query labels")


# ---- the non-finite contract, clause by clause ------------------------------------------------------------------------------------------
def _contract_case():
    q, x, v, g = _int_case(65)
    q, x, v, g = q[:70], x[:3000], np.array(v[:3000, :130]), g[:70, :130]
    labels = np.zeros(len(x), dtype=np.int32)
    labels[[7, 2500]] = 1  # the two rows are excluded for every query
    return q, x, v, g, labels, np.zeros((len(q), 1), dtype=np.int32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_a_non_finite_table_entry(dtype):
    q, x, v, g, labels, sub = _contract_case()
    bad = np.array(v)
    bad[7, 3] = np.nan
    bad[2500, 129] = np.inf
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        ix.set_row_values(v)
        clean, pe = _bw(ix, q, g, beta, subset=sub)
        ix.set_row_values(bad)
        # in INELIGIBLE rows, with the forward of the clean table: nothing spreads through u - the bits of the clean call
        got, _ = _bw(ix, q, g, beta, expectation=pe, subset=sub)
        _bits_equal(got, clean)
        # the forward of the bad table returns NaN in columns 3 and 129 (H2e): a row whose g is not zero there is NaN, the others are clean
        g0 = np.array(g)
        g0[::2, [3, 129]] = 0
        g0[1::2, 3] = 2.0 ** -10
        got, pe_bad = _bw(ix, q, g0, beta, subset=sub)
        assert torch.isnan(pe_bad.values[:, [3, 129]]).all()
        assert np.isnan(got[1::2]).all()
        _bits_equal(got[::2], _bw(ix, q, g0, beta, expectation=pe, subset=sub)[0][::2])
        # in an ELIGIBLE row: every query's gradient row is NaN
        got, _ = _bw(ix, q, g, beta, expectation=pe)
        assert np.isnan(got).all()
    _check(clean, q, x, v, g, dtype, beta, np.broadcast_to(labels == 0, (len(q), len(x))), what=f"the clean table {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_a_stored_non_finite_value_poisons_its_column_alone(dtype):
    q, x, v, g, labels, sub = _contract_case()
    xb = np.array(x)
    xb[7, 3] = np.nan      # (both rows are excluded by their labels, and row 7 by its NaN score too)
    xb[2500, 64] = np.inf
    clean = np.ones(65, dtype=bool)
    clean[[3, 64]] = False
    with _index(xb, dtype) as ix:
        ix.set_row_labels(labels)
        ix.set_row_values(v)
        got, _ = _bw(ix, q, g, 1.0 / 64.0, subset=sub)
    assert np.isnan(got[:, ~clean]).all() and np.isfinite(got[:, clean]).all()
    _check(got, q, np.where(np.isfinite(xb), xb, 0), v, g, dtype, 1.0 / 64.0, np.broadcast_to(labels == 0, (len(q), len(x))),
           what=f"NaN in the store {dtype}", cols=clean)


@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_a_non_finite_g_row_is_nan_and_alone(dtype):
    q, x, v, g, _, _ = _contract_case()
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        clean, pe = _bw(ix, q, g, 1.0 / 64.0)
        gb = np.array(g)
        gb[3, 5] = np.nan
        gb[64, 129] = np.inf
        gb[69, 0] = -np.inf
        got, _ = _bw(ix, q, gb, 1.0 / 64.0, expectation=pe)
    bad = [3, 64, 69]
    assert np.isnan(got[bad]).all()
    rest = np.setdiff1d(np.arange(70), bad)
    _bits_equal(got[rest], clean[rest])


# ---- one order -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,w", [(65, 64), (768, 193)])
def test_a_query_has_the_same_bits_in_any_batch_and_on_every_repeat(d, w, dtype):
    q, x, v, _ = _int_case(d)
    rng = np.random.default_rng(d)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)  # inexact sums: the order matters
    qg = (q + rng.standard_normal(q.shape)).astype(np.float32)
    vg = (v[:, :w] + rng.standard_normal((len(v), w))).astype(np.float32)
    gg = rng.standard_normal((len(q), w)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(xg, dtype) as ix:
        ix.set_row_values(vg)
        a, _ = _bw(ix, qg, gg, beta)
        _bits_equal(a, _bw(ix, qg, gg, beta)[0])
        _bits_equal(a[:64], _bw(ix, qg[:64], gg[:64], beta)[0])
        _bits_equal(a[:65], _bw(ix, qg[:65], gg[:65], beta)[0])
        for j in (0, 63, 64, 217, 299):
            _bits_equal(a[j : j + 1], _bw(ix, qg[j : j + 1], gg[j : j + 1], beta)[0], j)
    assert not np.isnan(a).any()


# ---- Gaussian data: the full bound, every element -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((len(x), 100)).astype(np.float32)
    g = rng.standard_normal((len(q), 100)).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(dim)))  # the float32 the call receives
    with _index(x, dtype) as ix:
        ix.set_row_values(v)
        got, _ = _bw(ix, q, g, beta)
    _check(got, q, x, v, g, dtype, beta, dot=True, what=f"gaussian dim {dim} {dtype}")


# ---- autograd --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_equals_the_explicit_call_and_a_float64_dense_softmax(dtype):
    q, x, v, g = _int_case(65)
    q, v, g = q[:129], v[:, :70], g[:129, :70]
    beta = 1.0 / 64.0
    with _index(x, dtype) as ix:  # 2 RG + 5 rows
        ix.set_row_values(v)
        explicit, pe = _bw(ix, q, g, beta)
        qd = _dev(q).requires_grad_(True)
        out = ix.expected_values(qd, temperature=1.0 / beta)
        assert out.dtype == torch.float32 and out.requires_grad and torch.equal(out.detach().view(torch.int32), pe.values.view(torch.int32))
        out.backward(_dev(g))
        assert qd.grad.dtype == torch.float32
        _bits_equal(qd.grad.cpu().numpy(), explicit)
        with pytest.raises(RuntimeError):  # once differentiable
            q2 = _dev(q).requires_grad_(True)
            (g2,) = torch.autograd.grad(ix.expected_values(q2, temperature=1.0 / beta).sum(), q2, create_graph=True)
            g2.sum().backward()
        # 16-bit queries get a gradient of their dtype: the float32 result rounded once
        qh = _dev(q).to(TDT[dtype]).requires_grad_(True)
        ix.expected_values(qh, temperature=1.0 / beta).backward(_dev(g))
        assert qh.grad.dtype == TDT[dtype] and torch.equal(qh.grad, torch.from_numpy(explicit).cuda().to(TDT[dtype]))
        # a class-mass cross-entropy trains through it
        ql = _dev(q).requires_grad_(True)
        ix.set_row_values(np.eye(4, dtype=np.float32)[np.arange(len(x)) % 4])
        loss = -torch.log(ix.expected_values(ql, temperature=1.0 / beta)[torch.arange(129), torch.arange(129) % 4]).mean()
        loss.backward()
        assert torch.isfinite(ql.grad).all() and ql.grad.abs().max() > 0
    # float64 dense softmax autograd on the GPU over the same rows
    xr, vr = _dev(x).double(), _dev(v).double()
    q64 = _dev(q).double().requires_grad_(True)
    (torch.softmax(beta * (q64 @ xr.T), dim=1) @ vr * _dev(g).double()).sum().backward()
    bound = G.device_bound(q, x, v, g, dtype, beta, dot=False)
    err = np.abs(explicit.astype(np.float64) - q64.grad.cpu().numpy())
    print(f"autograd {dtype}: max err / bound = {(err / bound).max():.3e}")
    assert (err <= bound + 1e-13 * np.abs(explicit)).all()


# ---- beside searches ---------------------------------------------------------------------------------------------------------------------
def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x, v, g = _int_case(768)
    qd, gd = _dev(q[:129]), _dev(g[:129, :129])
    with _index(x[:3000], "float16") as ix:
        ix.set_row_values(v[:3000, :129])
        serial_s, serial_i = ix.search(qd, 100)
        pe = ix.posterior_expectation(qd, temperature=64.0)
        serial = ix.posterior_expectation_backward(qd, gd, pe, temperature=64.0)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            grad = ix.posterior_expectation_backward(qd, gd, pe, temperature=64.0)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert torch.equal(grad.view(torch.int32), serial.view(torch.int32))
        assert ix.get_stat("last_overflow") == 0


# ---- node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards,capacity", [(2, 3000), (3, 3000), (3, 12000)])
def test_node_index_adds_the_shards(n_shards, capacity):
    from vod_amd.index import HipNodeIndex

    q, x, v, g = _int_case(65)
    x, v, g = x[:3000], v[:3000, :70], g[:129, :70]
    nq, beta = 129, 1.0 / 64.0
    q = q[:nq]
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    rps = (capacity + n_shards - 1) // n_shards
    with HipNodeIndex(65, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        nx.add(x.astype(np.float32))
        nx.set_row_values(v)
        pe = nx.posterior_expectation(np.array(q), temperature=1.0 / beta)
        got = nx.posterior_expectation_backward(np.array(q), np.array(g), pe, temperature=1.0 / beta)
        nx.set_row_labels(labels)
        pe_sub = nx.posterior_expectation(np.array(q), temperature=1.0 / beta, subset=sub)
        got_sub = nx.posterior_expectation_backward(np.array(q), np.array(g), pe_sub, temperature=1.0 / beta, subset=sub)
        qt = torch.from_numpy(np.array(q)).requires_grad_(True)  # autograd through the host
        nx.expected_values(qt, temperature=1.0 / beta, subset=sub).backward(torch.from_numpy(np.array(g)))
        _bits_equal(qt.grad.numpy(), got_sub)
    for res, fwd, e, s_ in ((got, pe, None, None), (got_sub, pe_sub, elig, sub)):
        assert isinstance(res, np.ndarray) and res.dtype == np.float32 and res.shape == (nq, 65)
        # the host fold of the per-shard flat calls with the GLOBAL forward: bit for bit
        total = np.zeros((nq, 65), dtype=np.float64)
        for s in range(n_shards):
            lo, hi = min(len(x), s * rps), min(len(x), (s + 1) * rps)
            if lo == hi:
                continue  # (a shard that holds no row returns zeros)
            with _index(x[lo:hi], "float16", capacity=max(hi - lo, 1), dim=65) as ix:
                ix.set_row_values(v[lo:hi])
                kw = {}
                if e is not None:
                    ix.set_row_labels(labels[lo:hi])
                    kw["subset"] = s_
                dev_pe = type(fwd)(_dev(fwd.values), type(fwd.log_partition)(*(_dev(t) for t in fwd.log_partition)))
                total += _bw(ix, q, g, beta, expectation=dev_pe, **kw)[0].astype(np.float64)
        _bits_equal(res, total.astype(np.float32), (n_shards, capacity))
        # and within the bound of the float64 reference: the forward values and log_rel are the node's folded words (the read-out's
        # node test derives their error: `fold`), the shard rows add in double and round once (inside the bound's slack rounding)
        n = len(x) if e is None else e.sum(axis=1)
        fold = 2 * (P.device_bound(np.zeros((nq, 1)), None, None, beta, n, dot=False) + 4 * P.U * (1 + np.log(len(x)))) + 2 * P.U
        Sv = PM.weights(q.astype(np.float64) @ x.astype(np.float64).T, beta, e)[0] @ np.abs(v).astype(np.float64)
        vb = R.device_bound(q, x, v, "float16", beta, e, dot=False) * (1 + fold[:, None]) + fold[:, None] * Sv
        _check(res, q, x, v, g, "float16", beta, e, what=f"node {n_shards} shards capacity {capacity}", values_bound=vb, rel_extra=fold)
        assert not np.isnan(res).any()


# ---- refusals and empty cases ------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex, LogPartition, PosteriorExpectation

    lib = _native.load_library()
    q, x, v, g = _int_case(65)
    x, v, g = x[:600], v[:600, :5], g[:5, :5]
    qd, gd = _dev(q[:5]), _dev(g)
    words = torch.zeros((2, 5), device="cuda")
    yd = torch.zeros((5, 5), device="cuda")
    out = torch.full((5, 65), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    opt = lambda t: None if t is None else ptr(t)  # noqa: E731

    def raw(h, queries=qd, code=2, nq=5, beta=1.0, lab=None, n_lab=0, m=words[0], r=words[1], y=yd, gv=gd, o=out):
        return lib.vodhip_index_posterior_expectation_backward(h, opt(queries), code, nq, ctypes.c_float(beta), opt(lab), n_lab, opt(m), opt(r), opt(y),
                                                               opt(gv), opt(o), None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    fake = PosteriorExpectation(yd, LogPartition(words[0], words[0], words[1]))
    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x[:300], "float16", capacity=600) as ix:
        refused(raw(ix._h), "no value table")
        with pytest.raises(_native.NativeLibraryError, match="no value table"):
            ix.posterior_expectation_backward(qd, gd, fake)
        ix.set_row_values(v[:300])
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        refused(raw(ix._h, m=None), "invalid query / output pointers")
        refused(raw(ix._h, r=None), "invalid query / output pointers")
        refused(raw(ix._h, o=None), "invalid query / output pointers")
        refused(raw(ix._h, y=None), "values is NULL")
        refused(raw(ix._h, gv=None), "grad_values is NULL")
        refused(raw(ix._h, nq=-1), "invalid query / output pointers")
        refused(raw(ix._h, code=3), "invalid q_dtype 3")
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            refused(raw(ix._h, beta=beta), "beta must be finite and > 0")
        refused(raw(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=2), "set the row labels first")
        for bad in (gd[:, :4], gd[:4], gd[0]):  # a mis-shaped g
            with pytest.raises(ValueError, match="grad_values"):
                ix.posterior_expectation_backward(qd, bad, fake)
        ix.add(x[300:])  # rows behind the table: it is short now
        refused(raw(ix._h), "the value table holds 300 rows, the index 600")
        with pytest.raises(_native.NativeLibraryError, match="holds 300 rows, the index 600"):
            ix.posterior_expectation_backward(qd, gd, fake)
        torch.cuda.synchronize()
        assert (out == 123.0).all()  # a refused call writes nothing
        ix.set_row_values(v)
        assert raw(ix._h, queries=None, nq=0, m=None, r=None, y=None, gv=None, o=None) == 0  # nq == 0: returns 0, needs nothing, writes nothing
        torch.cuda.synchronize()
        assert (out == 123.0).all()
        pe0 = ix.posterior_expectation(torch.zeros((0, 65), device="cuda"))
        assert ix.posterior_expectation_backward(torch.zeros((0, 65), device="cuda"), torch.zeros((0, 5), device="cuda"), pe0).shape == (0, 65)
        ix.set_row_values(v / 4096)
        small, _ = _bw(ix, q[:5], g, 1.0 / 64.0)
        ix.set_row_values(v)  # a new table drops the cached column maxima: with the old ones (4096 times too small) fp16 weights would overflow
        first, pe = _bw(ix, q[:5], g, 1.0 / 64.0)
        assert np.abs(first).max() > 1e-6
        _bits_equal(first, small * np.float32(4096))
        _check(first, q[:5], x, v, g, "float16", 1.0 / 64.0, what="after the refusals")
        ix.reset()  # drops the table
        ix.add(x)
        refused(raw(ix._h), "no value table")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        ix.set_row_values(v[:300])
        refused(raw(ix._h), "L2 index")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        ix.set_row_values(v[:300])
        refused(raw(ix._h), "VODHIP_EXACT_F32")
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            ix.posterior_expectation_backward(qd, gd, fake)
    torch.cuda.synchronize()
    assert (out == 123.0).all()
    with _index(x[:0], "float16", capacity=8, dim=65) as ix:  # an empty index with a table of no rows
        ix.set_row_values(np.zeros((0, 5), dtype=np.float32))
        got, pe = _bw(ix, q[:5], g, 1.0)
        assert torch.isneginf(pe.log_partition.max_score).all() and (got.view(np.uint32) == 0).all()
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        nx.add(x.astype(np.float32))
        host_fake = PosteriorExpectation(np.zeros((5, 5), np.float32), LogPartition(np.zeros(5, np.float32), np.zeros(5, np.float32), np.zeros(5, np.float32)))
        with pytest.raises(_native.NativeLibraryError, match="no value table"):
            nx.posterior_expectation_backward(np.array(q[:5]), np.array(g), host_fake)
        nx.set_row_values(v)
        with pytest.raises(_native.NativeLibraryError, match="beta must be finite"):
            nx.posterior_expectation_backward(np.array(q[:5]), np.array(g), host_fake, temperature=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.posterior_expectation_backward(np.array(q[:5]), np.array(g), host_fake, subset=np.zeros((5, 2), dtype=np.int32))
        with pytest.raises(ValueError, match="grad_values"):
            nx.posterior_expectation_backward(np.array(q[:5]), np.array(g[:, :4]), host_fake)
        pe0 = nx.posterior_expectation(np.zeros((0, 65), dtype=np.float32))
        assert nx.posterior_expectation_backward(np.zeros((0, 65), dtype=np.float32), np.zeros((0, 5), dtype=np.float32), pe0).shape == (0, 65)
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.posterior_expectation_backward(np.array(q[:5]), np.array(g), host_fake)
