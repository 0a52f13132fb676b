"""The fused inner-product top-k and the exact-f32 mode across embedding widths (the tables of tests/test_dim_edges_cpu.py, which
proves on the CPU which kernel and how many corpus tiles per workgroup every shape below runs).

Scan kernels: integer data in -8 .. 8 (every partial sum exact in fp32 up to dim 16384), ids and scores equal to
`oracle.flat_ip.flat_ip_topk` bit for bit.  The oracle runs once per data set at k = 100; a smaller k compares with the first k columns
(the order - score descending, id ascending - is total, so the top-k is a prefix of the top-100).  Widths with an odd number of K-tiles
(nk = 3, 5, 7, 13, 17) on stores whose persistent workgroups walk two and three corpus tiles, widths of 24 to 256 K-tiles, fp16 and bf16.

Exact-f32 mode: every `NI` of `exact_dot_preload` (dim_pad <= 1024), the first width of the generic `exact_dot` and two well inside it,
on Gaussian float32 inputs (the contract of tests/test_exact_gpu.py) and on integer inputs (bit for bit); path, batch and shard
independence of the score bits; the two planes read back; the documented limit, dim 16384, and its refusal one above.

The tie gap on Gaussian inputs.  tests/test_exact_gpu.py allows two rows to swap when their float64 scores are closer than TIE_TOL =
1e-4, sized for |score| of 100-200.  At dim 1088 and above a float32 brute force in NumPy already deviates from float64 by that much
(|score| reaches 330 at dim 4096), so here the gap is max(TIE_TOL, 4 * dev32), dev32 = max |float32(q @ x.T) - float64| on the case's
own inputs - four times the float32 reference's own error, the scheme of tests/vod_ref.py.  Every case prints dev32, the gap, its
largest score deviation and the share of positions whose id differs; that share may not exceed 1 % (the oracle alone has 0.1-0.2 % of
its adjacent top-100 gaps inside the gap at dims 1088 to 4096).  Measured on an MI355X (20,000 rows, 130 queries, k = 100):

      dim  store     dev32     tie gap   max |score - oracle|  max |score|  positions differing (largest float64 gap at one)
       64  float16   1.52e-05  1.00e-04  3.81e-06                46         0
      256  float16   5.98e-05  2.39e-04  7.63e-06                82         0
      257  float16   6.34e-05  2.54e-04  7.63e-06                78         0
      512  float16   7.98e-05  3.19e-04  1.53e-05               113         0
      513  float16   7.00e-05  2.80e-04  1.53e-05               107         0
      768  float16   9.60e-05  3.84e-04  1.53e-05               153         0
      769  float16   1.00e-04  4.02e-04  1.53e-05               139         0.0154 % (8.95e-07)
     1024  float16   1.08e-04  4.33e-04  1.53e-05               162         0
     1025  both      1.03e-04  4.11e-04  1.53e-05               160         0
     1536  float16   1.23e-04  4.90e-04  3.05e-05               213         0.0154 % (1.33e-06)
     4096  both      1.76e-04  7.05e-04  3.05e-05               340         0

The two swaps seen are between rows 1e-6 apart in float64: the derived gap is two orders of magnitude wider than what the kernel needs,
and the 1 % cap and the 1e-3 score bound are what keep it from hiding a wrong kernel (a generic `exact_dot` that skips its last 256-column
block fails every case from 1025 up, the integer cases, the path and shard cases and the case at 16384, while tests/test_exact_gpu.py
stays green).
"""
import functools

import numpy as np
import pytest

import test_dim_edges_cpu as T
from test_exact_gpu import SCORE_TOL, TIE_TOL, _gauss
from test_exact_gpu import _index as _exact_index
from test_mips_gpu import _index, _oracle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _case_id(c):
    return f"{c[0]}-tile{c[1]}-dim{c[2]}-{c[3]}"


def _dev(a):
    """a device tensor of a (read-only) NumPy array"""
    return torch.from_numpy(np.array(a)).cuda()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _int_rows(rng, n, d, lim=8):
    """uniform integers in -lim .. lim, the draw of test_mips_gpu._int_data (int8 draws: no int64 copy of a 100 M element store)"""
    return rng.integers(-lim, lim + 1, size=(n, d), dtype=np.int8)


@functools.lru_cache(maxsize=2)
def _scan_reference(n, d, nq):
    """(q, x, oracle scores, oracle ids at k = 100) of one integer data set: computed once, shared by every case on it, read-only"""
    rng = np.random.default_rng([n, d, nq])
    x, q = _int_rows(rng, n, d).astype(np.float16), _int_rows(rng, nq, d).astype(np.float16)
    return _frozen(q, x, *_oracle(q, x, 100))


def _assert_scan(case, q, x, rs, ri, check_overflow=True):
    _fam, tile, d, dt, n, nq, ks, why = case
    assert x.shape == (n, d) and len(q) >= nq
    tq = _dev(q[:nq])
    with _index(x, dtype=getattr(torch, dt), tile=tile) as ix:
        for k in ks:
            s, i = ix.search(tq, k)
            np.testing.assert_array_equal(i.cpu().numpy(), ri[:nq, :k], err_msg=f"ids, k = {k}: {why}")
            np.testing.assert_array_equal(s.cpu().numpy(), rs[:nq, :k], err_msg=f"scores, k = {k}: {why}")
            if check_overflow:
                assert ix.get_stat("last_overflow") == 0


# ---- scan kernels ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", T.WIDE_CASES, ids=_case_id)
def test_wide_batches_are_bit_exact_at_every_width(case):
    """Tiles 8, 9 and 14 forced, and the auto tile, on 1,024 (auto: also 300) queries: the workgroups of the persistent kernels walk two
    or three corpus tiles, so with an odd nk the second tile starts on the other operand-buffer parity / ring slot.  (At dim 1 and 7
    thousands of rows tie with the k-th score - every row, for an all-zero query: candidate lists may overflow and recover, as
    test_mips_gpu.test_overflow_recovery_stays_exact covers; from dim 65 on no list may overflow.)"""
    d, n = case[2], case[4]
    _assert_scan(case, *_scan_reference(n, d, 1024), check_overflow=d >= 65)


@pytest.mark.parametrize("case", T.SMALL_CASES, ids=_case_id)
def test_small_batch_kernels_are_bit_exact_at_every_width(case):
    """The 128x128 kernel (1) and the ring kernels (42, 46): slice `ks % NSTAGE` of a three-slot ring at nk = 1, 2, 3, 5, 7, 13, 17 .. 64."""
    d, n = case[2], case[4]
    _assert_scan(case, *_scan_reference(n, d, 100), check_overflow=d >= 65)


@functools.lru_cache(maxsize=2)
def _marker_reference(n, d, nq):
    """Rows and queries are zero except in column dim - 1.  Rows: every integer fp16 holds exactly (-2048 .. 2048), each once per 4097
    consecutive rows (1237 is coprime to 4097 = 17 * 241); queries: distinct non-zero integers.  One product per score, below 2^21."""
    x, q = np.zeros((n, d), dtype=np.float16), np.zeros((nq, d), dtype=np.float16)
    x[:, d - 1] = (np.arange(n) * 1237 % 4097 - 2048).astype(np.float16)
    v = np.arange(nq) - nq // 2
    q[:, d - 1] = np.where(v >= 0, v + 1, v).astype(np.float16)
    return _frozen(q, x, *_oracle(q, x, 100))


@pytest.mark.parametrize("case", T.MARKER_CASES, ids=_case_id)
def test_the_last_column_alone_decides_every_score(case):
    _fam, _tile, d, _dt, n, nq, _ks, _why = case
    q, x, rs, ri = _marker_reference(n, d, nq)
    assert np.all(rs[:, 0] >= 2047.0) and np.all(rs[:, :10] > 0)  # every query has a row of its sign with |x| >= 2047: no score is 0
    _assert_scan(case, q, x, rs, ri, check_overflow=False)


@functools.lru_cache(maxsize=1)
def _subset_reference(n, d, nq, k):
    """the labels, per-query allowed labels and masked oracle of test_mips_gpu.test_subset_filtered_search, on this module's data"""
    from oracle.flat_ip import topk_desc_tiebreak

    q, x, _rs, _ri = _scan_reference(n, d, nq)
    rng = np.random.default_rng(77)
    labels = rng.integers(0, 12, size=n).astype(np.int32)
    subset = np.full((nq, 3), -1, dtype=np.int32)
    for r in range(nq):
        m = rng.integers(0, 4)                       # 0 -> unrestricted query
        subset[r, :m] = rng.choice(12, size=m, replace=False)
    subset[5] = [99, -1, -1]                         # a label nobody carries -> no hits at all
    masked = q.astype(np.float64) @ x.astype(np.float64).T
    for r in range(nq):
        allowed = subset[r][subset[r] >= 0]
        if allowed.size:
            masked[r, ~np.isin(labels, allowed)] = np.nan            # NaN scores never enter the oracle's result
    return _frozen(q, x, labels, subset, *topk_desc_tiebreak(masked, k))


@pytest.mark.parametrize("case", T.SUBSET_CASES, ids=_case_id)
def test_subset_filter_at_an_odd_k_tile_count(case):
    _fam, tile, d, _dt, n, nq, (k,), _why = case
    q, x, labels, subset, rs, ri = _subset_reference(n, d, nq, k)
    with _index(x, tile=tile) as ix:
        ix.set_row_labels(labels)
        s, i = ix.search(_dev(q), k, subset=np.array(subset))
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(s.cpu().numpy(), rs)
    assert np.all(ri[5] == -1)


@pytest.mark.parametrize("case", T.TOP_CASES, ids=_case_id)
def test_the_widest_store_is_bit_exact(case):
    """dim 16384, nk = 256, a row pitch of 32 KB.  vodhip_index_create states no width limit for a plain store (the limit of 16384 is
    the exact-f32 mode's): this documents that the scan kernels work at that width."""
    _assert_scan(case, *_scan_reference(case[4], case[2], 300))


# ---- exact-f32 mode ------------------------------------------------------------------------------------------------------------------

GAUSS_N, GAUSS_NQ, GAUSS_K = 20_000, 130, 100


@functools.lru_cache(maxsize=2)
def _gauss_reference(d):
    """float32 N(0, 1) inputs, their float64 score matrix, the float64 oracle, and dev32: the largest deviation of a NumPy float32
    brute force from float64 on these inputs"""
    q, x = _gauss(d, GAUSS_N, d, GAUSS_NQ)
    full64 = q.astype(np.float64) @ x.astype(np.float64).T
    dev32 = float(np.abs((q @ x.T).astype(np.float64) - full64).max())
    return (*_frozen(q, x, full64), dev32, *_frozen(*_oracle(q, x, GAUSS_K)))


def _compare_exact(s, i, ref, k, label, nq=None):
    """The contract of test_exact_gpu._compare with the derived tie gap (module docstring), plus: at most 1 % of the positions differ."""
    q, x, full64, dev32, rs, ri = ref
    s, i = s.cpu().numpy(), i.cpu().numpy()
    nq = len(q) if nq is None else nq
    rs, ri, full64 = rs[:nq, :k], ri[:nq, :k], full64[:nq]
    tie = max(TIE_TOL, 4.0 * dev32)
    rows = np.arange(nq)[:, None]
    assert np.all(i >= 0) and i.shape == ri.shape
    diff = float(np.abs(s - rs).max())
    differ = i != ri
    mine64, ref64 = full64[rows, i], full64[rows, ri]
    print(f"{label}: dev32 {dev32:.3g}  tie gap {tie:.3g}  max |score - oracle| {diff:.3g}  |score| max {np.abs(rs).max():.0f}  "
          f"positions differing {differ.mean():.4%}  largest gap at one {np.abs(mine64 - ref64)[differ].max() if differ.any() else 0.0:.3g}")
    assert np.all(s[:, 1:] <= s[:, :-1]), "scores not sorted"
    assert diff <= SCORE_TOL, f"max |score - oracle| = {diff}"
    assert np.all(mine64 >= ref64[:, -1:] - tie), "a returned row is not in the top-k"
    assert all(set(a) == set(b) for a, b in zip(i, ri)), "recall < 1"
    assert differ.mean() <= 0.01, f"{differ.mean():.2%} of the positions differ from the oracle"
    if differ.any():  # where the order differs, the two rows are tied at float32 level
        assert np.abs(mine64 - ref64)[differ].max() <= tie


GAUSS_CASES = [(d, "float16", w) for d, w in T.EXACT_WIDTHS] + [(d, "bfloat16", "bf16 scan: " + dict(T.EXACT_WIDTHS)[d]) for d in T.EXACT_BF16_WIDTHS]


GAUSS_CASES.sort(key=lambda c: c[0])


@pytest.mark.parametrize("d,dtype,why", GAUSS_CASES, ids=[f"dim{d}-{dt}" for d, dt, _ in GAUSS_CASES])
def test_exact_mode_on_float32_inputs_across_the_dispatch(d, dtype, why):
    ref = _gauss_reference(d)
    with _exact_index(ref[1], dtype=getattr(torch, dtype)) as ix:
        s, i = ix.search(_dev(ref[0]), GAUSS_K)
        assert ix.get_stat("exact") == 1 and ix.get_stat("last_overflow") == 0
    _compare_exact(s, i, ref, GAUSS_K, f"dim {d} {dtype}")


@functools.lru_cache(maxsize=1)
def _exact_int_reference(d):
    rng = np.random.default_rng([3, d])
    x, q = _int_rows(rng, 20_000, d, 3).astype(np.float32), _int_rows(rng, 300, d, 3).astype(np.float32)
    return _frozen(q, x, *_oracle(q, x, 100))


@pytest.mark.parametrize("d,tile", [(d, t) for d in T.EXACT_INT_WIDTHS for t in (1, 8, 14)])
def test_exact_mode_on_integer_inputs_is_bit_exact_in_the_generic_path(d, tile):
    """As test_exact_gpu.test_integer_inputs_are_bit_exact_ties_included, beyond 1024 columns: all arithmetic is exact, rows tie."""
    q, x, rs, ri = _exact_int_reference(d)
    nq = 70 if tile == 1 else 300
    with _exact_index(x, tile=tile) as ix:
        for k in (1, 25, 100):
            s, i = ix.search(_dev(q[:nq]), k)
            np.testing.assert_array_equal(i.cpu().numpy(), ri[:nq, :k])
            np.testing.assert_array_equal(s.cpu().numpy(), rs[:nq, :k])


@pytest.mark.parametrize("d", T.EXACT_PATH_WIDTHS)
def test_exact_scores_do_not_depend_on_the_path(d):
    """The list pass, the band pass (k' = k proves no list complete) and the band pass split by a tiny candidate capacity return the
    same bytes: "the score this mode returns, whatever path, shard or batch computed it" (kernels_exact.hip)."""
    ref = _gauss_reference(d)
    q, x = ref[0][:96], ref[1]
    k = 64
    with _exact_index(x) as ix:
        s0, i0 = ix.search(_dev(q), k)
        _compare_exact(s0, i0, ref, k, f"dim {d} paths", nq=96)
        ix.set_param("exact_expand", 1)  # k' = max(k, k / 100 + 16) = k
        s1, i1 = ix.search(_dev(q), k)
        assert ix.get_stat("last_exact_kx") == k and ix.get_stat("last_exact_band_queries") == len(q)
        assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
        ix.set_param("cand_cap", 256)
        s2, i2 = ix.search(_dev(q[:40]), k)
        assert torch.equal(i0[:40], i2) and torch.equal(s0[:40].view(torch.int32), s2.view(torch.int32))


@pytest.mark.parametrize("d", T.EXACT_PATH_WIDTHS)
def test_two_exact_shards_merged_equal_the_whole_index_bit_for_bit(d):
    from vod_amd.index import merge_topk

    ref = _gauss_reference(d)
    x, k, cut = ref[1], 40, 11_777
    qd = _dev(ref[0])
    with _exact_index(x) as whole, _exact_index(x[:cut]) as a, _exact_index(x[cut:]) as b:
        sw, iw = whole.search(qd, k)
        sa, ia = a.search(qd, k)
        sb, ib = b.search(qd, k, id_base=cut)
        sm, im = merge_topk(torch.stack([sa, sb]), torch.stack([ia, ib]))
        assert torch.equal(im, iw) and torch.equal(sm.view(torch.int32), sw.view(torch.int32))
        s1, i1 = whole.search(qd[17:18], k)  # ... nor on who else is in the batch
        assert torch.equal(i1[0], iw[17]) and torch.equal(s1[0], sw[17])


def _bits(t):
    a = t.cpu().contiguous()
    return a.view(torch.int32 if a.dtype == torch.float32 else torch.int16).numpy()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("d", T.EXACT_ROW_WIDTHS)
def test_both_planes_read_back_what_was_added(d, dtype):
    """Rows from host float32, device float32 and device fp16: the float32 plane returns them bit for bit, the scan plane torch's
    round-to-nearest-even cast of them, both unpadded (`ingest_exact_kernel` strides 512 columns per step: 3 to 8 steps here; at 1025 and
    1027 the scalar path, 1027 with a last 8-element group of three live columns)."""
    tdt = getattr(torch, dtype)
    x = torch.randn(600, d, generator=torch.Generator().manual_seed(d))
    x16 = x[400:].half()
    want = torch.cat([x[:400], x16.float()])
    with _exact_index(np.zeros((0, d), dtype=np.float32), dtype=tdt, capacity=600) as ix:
        ix.add(x[:200].numpy())
        ix.add(x[200:400].cuda())
        ix.add(x16.cuda())
        assert ix.ntotal == 600 and ix.get_stat("dim_pad") == T.nk_of(d) * 64
        f32, h = ix.stored_rows_f32(), ix.stored_rows()
        assert f32.shape == (600, d) and h.shape == (600, d) and h.dtype == tdt
        np.testing.assert_array_equal(_bits(f32), _bits(want))
        np.testing.assert_array_equal(_bits(h), _bits(want.to(tdt)))
        np.testing.assert_array_equal(_bits(ix.stored_rows_f32(399, 3)), _bits(want[399:402]))
        np.testing.assert_array_equal(_bits(ix.stored_rows(199, 3)), _bits(want[199:202].to(tdt)))


def test_exact_mode_at_its_widest():
    """dim 16384: 64 KB of query in LDS next to the keys (the dynamic-LDS opt-in), 64 blocks of the generic exact_dot per row."""
    d = T.EXACT_MAX_DIM
    rng = np.random.default_rng(d)
    x, q = _int_rows(rng, 2_000, d, 3).astype(np.float32), _int_rows(rng, 32, d, 3).astype(np.float32)
    rs, ri = _oracle(q, x, 100)
    with _exact_index(x) as ix:
        for k in (1, 10, 100):
            s, i = ix.search(_dev(q), k)
            np.testing.assert_array_equal(i.cpu().numpy(), ri[:, :k])
            np.testing.assert_array_equal(s.cpu().numpy(), rs[:, :k])
        np.testing.assert_array_equal(ix.stored_rows_f32(1_990, 10).cpu().numpy(), x[1_990:])


def test_exact_mode_refuses_a_wider_store_and_the_library_goes_on():
    from vod_amd._native import NativeLibraryError
    from vod_amd.index import HipFlatIndex

    rng = np.random.default_rng(5)
    x, q = _int_rows(rng, 3_000, 64, 3).astype(np.float32), _int_rows(rng, 8, 64, 3).astype(np.float32)
    rs, ri = _oracle(q, x, 10)
    with _exact_index(x) as ix:
        with pytest.raises(NativeLibraryError, match="VODHIP_EXACT_F32 stores take dim <= 16384"):
            HipFlatIndex(T.EXACT_MAX_DIM + 1, 16, dtype=torch.float16, device=0, exact_f32=True)
        s, i = ix.search(_dev(q), 10)  # the next call on a valid index still works
        np.testing.assert_array_equal(i.cpu().numpy(), ri)
        np.testing.assert_array_equal(s.cpu().numpy(), rs)
