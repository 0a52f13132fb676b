"""`HipFlatIndex.posterior_divergence` / `HipNodeIndex.posterior_divergence` and `kl_to` on the GPU against the float64 restatement
(tests/divergence_ref.py).  Every word of every pair is compared; the tolerance is the derived bound and nothing else.

Integer data (the sets of test_log_partition_gpu.py: values in [-8, 8], every score exact in float32, the dot-product part of the bound
dropped); side b is side a rolled by one, so a pair never sits in the column of its partner's original.  Stores of 1, 255, 256, 257 and
3000 rows, widths 1, 64, 65, 768, fp16 and bf16, (beta_a, beta_b) in {(1/64, 1/64), (1, 1/64), (4, 1)}, pair batches 1, 32 (the last
of the 64-query kernel), 33 (the first of the 128-query kernel), 64, 65 (across a query tile) and 150.

Then: identical pairs (cross_rel == mean_rel bit for bit, kl == 0.0), stale and padded rows, non-finite scores, batch independence and
repeatability, a high score in one tile for one side only, the finish's chunk edge (2049 tiles), subset labels, Gaussian data within
the full bound, `kl_to`, the node index, a call beside a search in flight, refusals and empty cases.
Measured shares of the bound (MI355X): DESIGN.md 5 and profiles/posterior_divergence.json.
"""
import ctypes

import numpy as np
import pytest

import divergence_ref as D
import partition_ref as P
import posterior_ref as PM
import stats_ref as S
from test_l2_cpu import GAUSS_CASES, gauss_case
from test_log_partition_gpu import _index, _int_case

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTYPES = ["float16", "bfloat16"]
STORES = [1, 255, 256, 257, 3000]
WIDTHS = [1, 64, 65, 768]
BATCHES = [1, 32, 33, 64, 65, 150]
BETAS = [(1.0 / 64.0, 1.0 / 64.0), (1.0, 1.0 / 64.0), (4.0, 1.0)]


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _words(r):
    """PosteriorDivergence -> the eight library words (order of D.WORDS), the six derived ones (order of D.DERIVED), the two log_z"""
    a, b = r.stats_a, r.stats_b
    t = (a.max_score, a.log_rel, a.mean_rel, r.cross_rel_ab, b.max_score, b.log_rel, b.mean_rel, r.cross_rel_ba,
         r.entropy_a, r.entropy_b, r.cross_entropy_ab, r.cross_entropy_ba, r.kl_ab, r.kl_ba, a.log_partition.log_z, b.log_partition.log_z)
    return tuple(_np(w) for w in t)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _pd(ix, qa, qb, beta_a=1.0, beta_b=None, **kw):
    return _words(ix.posterior_divergence(_dev(qa), _dev(qb), temperature_a=1.0 / beta_a, temperature_b=None if beta_b is None else 1.0 / beta_b, **kw))


def _ps3(ix, q, beta, **kw):
    r = ix.posterior_stats(_dev(q), temperature=1.0 / beta, **kw)
    return tuple(_np(t) for t in (r.log_partition.max_score, r.log_partition.log_rel, r.mean_rel))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _all_same_bits(a, b, n=None):
    return all(_same_bits(u if n is None else u[:n], v) for u, v in zip(a, b))


def _check(got, ref, b8, beta_a, beta_b, what=""):
    """the eight words of every pair within their bounds of the float64 words, the derived words formed from the eight as stated and
    within the sums of the bounds, the signs, and the words of a dead side.  Prints and returns the largest share of each bound."""
    assert all(w.dtype == np.float32 for w in got)
    w64 = ref.words
    live_a, live_b = np.isfinite(w64[0]), np.isfinite(w64[4])
    both = live_a & live_b
    shares = {}

    def within(name, g, want, b, mask):
        fin = mask & np.isfinite(want)
        err = np.abs(g[fin].astype(np.float64) - want[fin])
        bb = b[fin]
        share = float((err[bb > 0] / bb[bb > 0]).max()) if (bb > 0).any() else 0.0
        shares[name] = share
        print(f"{what}: {name}: max err {err.max() if err.size else 0.0:.3e}, largest share of the bound {share:.4f}")
        assert (err <= bb).all(), (what, name, float(err.max()), float(bb[err > bb].min()))
        odd = mask & ~np.isfinite(want)  # (-inf cross words: the same value)
        np.testing.assert_array_equal(g[odd], want[odd].astype(np.float32), err_msg=f"{what} {name}")

    for k, name in enumerate(D.WORDS):
        within(name, got[k], w64[k], b8[k], both if k in (3, 7) else (live_a if k < 4 else live_b))
    for k in (2, 3, 6, 7):
        assert (got[k][both] <= 0).all(), (what, D.WORDS[k])
    assert not np.signbit(got[1][live_a]).any() and not np.signbit(got[5][live_b]).any()
    # the derived words: float64 arithmetic on the eight float32 words in the stated grouping, rounded once
    formed = D.derived(tuple(w.astype(np.float64) for w in got[:8]), float(np.float32(beta_a)), float(np.float32(beta_b)))
    b6 = D.derived_bounds(beta_a, beta_b, w64, b8)
    for k, name in enumerate(D.DERIVED):
        np.testing.assert_array_equal(got[8 + k], formed[k].astype(np.float32), err_msg=f"{what} {name}")
        within(name, got[8 + k], D.derived(w64, beta_a, beta_b)[k], b6[k], (live_a if k == 0 else live_b if k == 1 else both))
        assert (got[8 + k][both] >= (0.0 if k >= 4 else -b6[k][both])).all(), (what, name)
    # a dead side: (max, log_rel) as log_partition states them, its mean_rel NaN, BOTH cross words (and what is derived from them) NaN
    for side, live in ((0, live_a), (4, live_b)):
        dead = ~live
        np.testing.assert_array_equal(got[side][dead], w64[side][dead].astype(np.float32))
        np.testing.assert_array_equal(got[side + 1][dead], w64[side + 1][dead].astype(np.float32))
        assert np.isnan(got[side + 2][dead]).all()
    for k in (3, 7, 10, 11, 12, 13):
        assert np.isnan(got[k][~both]).all(), (what, k)
    return shares


def _check_int(got, sa, sb, beta_a, beta_b, eligible=None, what="", node=False):
    """exact integer scores: max_* bit for bit, the other words within the bound without its dot-product part"""
    ref = D.from_scores(sa, sb, beta_a, beta_b, eligible)
    b8 = D.bounds(None, None, None, None, beta_a, beta_b, ref, dot=False, node=node)
    np.testing.assert_array_equal(got[0], ref.words[0].astype(np.float32), err_msg=what)
    np.testing.assert_array_equal(got[4], ref.words[4].astype(np.float32), err_msg=what)
    return _check(got, ref, b8, beta_a, beta_b, what)


def _pairs(d, nq=150):
    """side a = the first nq integer queries, side b = the same set rolled by one"""
    q, x, s = _int_case(d)
    qa, sa = q[:nq], s[:nq]
    return qa, np.roll(qa, 1, axis=0), x, sa, np.roll(sa, 1, axis=0)


# ---- 1. sizes, widths, batches, betas, both dtypes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("n", STORES)
def test_store_sizes_widths_batches_and_betas(n, d, dtype):
    qa, qb, x, sa, sb = _pairs(d)
    x, sa, sb = x[:n], sa[:, :n], sb[:, :n]
    with _index(x, dtype) as ix:
        full = {}
        for beta_a, beta_b in BETAS:
            got = full[beta_a] = _pd(ix, qa, qb, beta_a, beta_b)
            _check_int(got, sa, sb, beta_a, beta_b, what=f"int n {n} d {d} {dtype} betas {beta_a:g} {beta_b:g}")
            # no NaN score anywhere: each side's three words are the bits of posterior_stats for that side alone
            assert _all_same_bits(got[0:3], _ps3(ix, qa, beta_a)) and _all_same_bits(got[4:7], _ps3(ix, qb, beta_b))
        for i, nq in enumerate(BATCHES[:-1]):
            beta_a, beta_b = BETAS[i % 3]
            got = _pd(ix, qa[:nq], qb[:nq], beta_a, beta_b)
            assert _all_same_bits(full[beta_a], got, nq), (nq, beta_a)
            assert _all_same_bits(got[0:3], _ps3(ix, qa[:nq], beta_a)) and _all_same_bits(got[4:7], _ps3(ix, qb[:nq], beta_b))


# ---- 2. identical pairs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 768])
def test_identical_pairs_have_zero_kl_and_the_cross_word_is_mean_rel(d, dtype):
    q, x, _ = _int_case(d)
    rng = np.random.default_rng(d)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)  # inexact sums: the order matters
    qg = (q[:150] + rng.standard_normal((150, d))).astype(np.float32)
    beta = float(np.float32(1.0 / np.sqrt(d) / 8))
    with _index(xg, dtype) as ix:
        for nq in (150, 20):  # both instantiations
            got = _pd(ix, qg[:nq], qg[:nq], beta)
            assert _same_bits(got[3], got[2]) and _same_bits(got[7], got[6]) and _all_same_bits(got[0:3], got[4:7])
            assert (got[12] == 0.0).all() and (got[13] == 0.0).all()
            assert _same_bits(got[10], got[8]) and (got[2] < 0).all()
            assert _all_same_bits(got[0:3], _ps3(ix, qg[:nq], beta))


# ---- 3. stale and padded rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_past_ntotal_are_never_counted(dtype):
    qa, qb, x, sa, sb = _pairs(65)
    b = (1.0, 1.0 / 64.0)
    with _index(x, dtype, capacity=3000) as ix:
        ix.reset()
        ix.add(x[2300:])  # 700 rows; rows 700 .. 2999 of the store still hold the first ingest
        assert ix.ntotal == 700
        _check_int(_pd(ix, qa[:129], qb[:129], *b), sa[:129, 2300:], sb[:129, 2300:], *b, what=f"reset {dtype}")
    with _index(x[:700], dtype, capacity=3000) as ix:  # nothing beyond ntotal was ever written
        _check_int(_pd(ix, qa[:129], qb[:129], *b), sa[:129, :700], sb[:129, :700], *b, what=f"capacity > ntotal {dtype}")
    with _index(x[:300], dtype, capacity=300) as ix:  # the last tile reaches past the capacity
        _check_int(_pd(ix, qa[:20], qb[:20], *b), sa[:20, :300], sb[:20, :300], *b, what=f"tile padding {dtype}")


# ---- 4. non-finite scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_rows_are_left_out_and_infinite_scores_and_no_row_give_the_stated_words(dtype):
    q, x, _ = _int_case(65)
    qa = np.array(q[:70])
    qb = np.roll(qa, 1, axis=0)
    qa[:, 0], qb[:, 0] = 1.0, 1.0
    qa[:, 1], qb[:, 1] = 0.0, -1.0
    sa, sb = qa.astype(np.float64) @ x.astype(np.float64).T, qb.astype(np.float64) @ x.astype(np.float64).T
    xn = np.array(x)
    xn[7, 3] = np.nan      # every score of row 7 is NaN, on both sides
    xn[300, 0] = -np.inf   # every score of row 300 is -inf on both sides: a term of 0, and no 0 * -inf
    xn[9, 1] = np.inf      # side a: 0 * inf = NaN, side b: -inf.  NaN against ONE side: the row is out of BOTH
    keep = np.ones(len(x), dtype=bool)
    keep[[7, 9, 300]] = False
    with _index(xn, dtype) as ix:
        for betas in ((1.0 / 64.0, 1.0 / 64.0), (1.0, 1.0 / 64.0)):
            got = _pd(ix, qa, qb, *betas)
            assert not any(np.isnan(w).any() for w in got)
            _check_int(got, sa[:, keep], sb[:, keep], *betas, what=f"NaN rows and -inf score {dtype} betas {betas[0]:g} {betas[1]:g}")
    with _index(np.repeat(xn[300:301], 300, axis=0), dtype) as ix:  # every score -inf on both sides: counts as no row
        got = _pd(ix, qa, qb, 1.0)
        assert all(np.isneginf(got[k]).all() for k in (0, 1, 4, 5, 14, 15)) and all(np.isnan(got[k]).all() for k in (2, 3, 6, 7, 8, 9, 10, 11, 12, 13))
    with _index(x[:0], dtype, capacity=8, dim=65) as ix:  # an empty index: no eligible row
        got = _pd(ix, qa[:5], qb[:5], 1.0)
        assert all(np.isneginf(got[k]).all() for k in (0, 1, 4, 5)) and all(np.isnan(got[k]).all() for k in (2, 3, 6, 7, 12, 13))
    # +inf on side a alone: the same row scores -inf on side b (columns 2 are 1 and -1) and adds nothing there
    qa2, qb2 = np.array(qa), np.array(qb)
    qa2[:, 2], qb2[:, 2] = 1.0, -1.0
    xi = np.array(x)
    xi[2999, 2] = np.inf
    with _index(xi, dtype) as ix:
        got = _pd(ix, qa2, qb2, 1.0, 1.0 / 64.0)
        side_b = _ps3(ix, qb2, 1.0 / 64.0)
    assert np.isposinf(got[0]).all() and np.isposinf(got[1]).all() and np.isposinf(got[14]).all()      # side a: (+inf, +inf, NaN)
    assert all(np.isnan(got[k]).all() for k in (2, 3, 7, 8, 10, 11, 12, 13))                            # ... and BOTH cross words
    assert _all_same_bits(got[4:7], side_b) and all(np.isfinite(got[k]).all() for k in (4, 5, 6, 9))   # side b's three words intact
    ref_b = S.from_scores((qb2.astype(np.float64) @ x.astype(np.float64).T)[:, :2999], 1.0 / 64.0)
    np.testing.assert_array_equal(got[4], ref_b[0].astype(np.float32))


def test_minus_inf_on_one_side_under_mass_gives_an_infinite_kl_one_way():
    # bf16: x[0, 0] = -1e30, a[0] = 1e-30 (the product is about -1), b[0] = 1e30 (the product overflows to -inf): row 0 has mass under p
    # and r(row 0) = 0
    q, x, _ = _int_case(65)
    xr = np.array(x[:600])
    xr[:, 0] = 0.0
    xr[0, 0] = -1e30
    qa, qb = np.array(q[:70]), np.roll(np.array(q[:70]), 1, axis=0)
    qa[:, 0], qb[:, 0] = 1e-30, 1e30
    beta = 1.0 / 64.0
    sa, sb = P.scores(qa, xr, "bfloat16"), P.scores(qb, xr, "bfloat16")
    sb[:, 0] = -np.inf  # (the float32 accumulator overflows where float64 holds -1e60)
    ref = D.from_scores(sa, sb, beta, beta)
    assert np.isneginf(ref.words[3]).all() and np.isfinite(ref.words[7]).all()
    with _index(xr, "bfloat16") as ix:
        got = _pd(ix, qa, qb, beta, beta)
        side_a, side_b = _ps3(ix, qa, beta), _ps3(ix, qb, beta)
    assert not any(np.isnan(w).any() for w in got)
    assert np.isneginf(got[3]).all() and np.isposinf(got[10]).all() and np.isposinf(got[12]).all()  # cross_rel_ab, H(p, r), KL(p || r)
    assert np.isfinite(got[7]).all() and np.isfinite(got[13]).all() and (got[13] >= 0).all() and (got[7] <= 0).all()
    assert all(np.isfinite(got[k]).all() for k in (0, 1, 2, 4, 5, 6, 8, 9, 11))
    assert _all_same_bits(got[0:3], side_a) and _all_same_bits(got[4:7], side_b)  # no NaN score: each side is posterior_stats' bits


# ---- 5. batch independence and repeatability -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [65, 768])
def test_a_pair_has_the_same_bits_in_any_batch_at_any_position_and_on_every_repeat(d, dtype):
    q, x, _ = _int_case(d)
    rng = np.random.default_rng(d + 1)
    xg = (x + rng.standard_normal(x.shape)).astype(np.float32)
    qa = (q[:150] + rng.standard_normal((150, d))).astype(np.float32)
    qb = np.roll(qa, 1, axis=0)
    ba = float(np.float32(1.0 / np.sqrt(d) / 8))
    bb = float(np.float32(ba / 2))
    with _index(xg, dtype) as ix:
        a = _pd(ix, qa, qb, ba, bb)
        assert _all_same_bits(a, _pd(ix, qa, qb, ba, bb))
        assert _all_same_bits(a, _pd(ix, qa[:33], qb[:33], ba, bb), 33)
        one = _pd(ix, qa[77:78], qb[77:78], ba, bb)  # alone: the 64-query instantiation
        assert _all_same_bits([w[77:78] for w in a], one)
        for pos in (0, 31, 32, 63, 64, 149):  # pair 77 moved to every edge position of the layout
            pa, pb = np.array(qa), np.array(qb)
            pa[[pos, 77]], pb[[pos, 77]] = pa[[77, pos]], pb[[77, pos]]
            moved = _pd(ix, pa, pb, ba, bb)
            assert _all_same_bits([w[pos : pos + 1] for w in moved], one), pos
        assert (a[3] < 0).all() and (a[12] > 0).all()


# ---- 6. a high score in one tile, for one side only ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_high_score_in_one_tile_for_one_side_re_centres_that_side_only(dtype):
    q, x, _ = _int_case(65)
    qa = np.array(q[:70])
    qa[:, 0] = 1.0
    qb = np.roll(qa, 1, axis=0)
    qb[:, 0] = 0.0                         # side b does not see column 0
    rows = np.repeat(x[:1], 1200, axis=0)  # 5 tiles, the last one partial
    rows[800:810, 0] += 3.0                # tile 3: 10 rows score 3 higher for side a, the same for side b
    sa, sb = qa.astype(np.float64) @ rows.astype(np.float64).T, qb.astype(np.float64) @ rows.astype(np.float64).T
    with _index(rows, dtype) as ix:
        for betas in BETAS:
            got = _check_int(_pd(ix, qa, qb, *betas), sa, sb, *betas, what=f"two-valued {dtype} betas {betas[0]:g} {betas[1]:g}")
        g = _pd(ix, qa, qb, 1.0, 1.0)
    # side b is uniform over 1200 rows: E_r[s_a] - max_a = -3 * 1190 / 1200, KL(r || p) and KL(p || r) in closed form
    z = 10 + 1190 * np.exp(-3.0)
    np.testing.assert_allclose(g[7], -3.0 * 1190 / 1200, rtol=1e-6)
    np.testing.assert_allclose(g[13], np.log(z / 1200) + 3.0 * 1190 / 1200, rtol=1e-5)
    np.testing.assert_allclose(g[12], np.log(1200 / z) - 3.0 * 1190 * np.exp(-3.0) / z, rtol=1e-5)
    assert (g[3] == 0).all() and (g[6] == 0).all()


# ---- 7. the finish's chunk edge ------------------------------------------------------------------------------------------------------------
def test_2049_tiles_cross_the_finish_chunk_edge():
    n, d, nq = 524289, 64, 3  # 2049 tiles: whole chunks of the finish and one tile; the last tile holds one row
    rng = np.random.default_rng(5)
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    qa = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    qb = np.roll(qa, 1, axis=0)
    sa = qa.astype(np.float64) @ x.astype(np.float64).T
    sb = np.roll(sa, 1, axis=0)
    with _index(x, "float16") as ix:
        for betas in ((1.0 / 64.0, 1.0 / 64.0), (1.0, 1.0 / 64.0)):
            got = _pd(ix, qa, qb, *betas)
            _check_int(got, sa, sb, *betas, what=f"2049 tiles betas {betas[0]:g} {betas[1]:g}")
            assert _all_same_bits(got[0:3], _ps3(ix, qa, betas[0])) and _all_same_bits(got[4:7], _ps3(ix, qb, betas[1]))


# ---- 8. subset labels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq", [8, 132])
def test_subset_labels(nq, dtype):
    qa, qb, x, sa, sb = _pairs(65, nq)
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        for betas in ((1.0, 1.0 / 64.0), (1.0 / 64.0, 1.0 / 64.0)):
            got = _pd(ix, qa, qb, *betas, subset=sub)
            _check_int(got, sa, sb, *betas, elig, what=f"subset nq {nq} {dtype} betas {betas[0]:g} {betas[1]:g}")
            assert np.isneginf(got[0][3::4]).all() and np.isneginf(got[4][3::4]).all() and np.isnan(got[12][3::4]).all()
            assert not np.isnan(got[12][:3]).any()
            # ONE label row per pair serves both sides: each side is posterior_stats under the pair's labels
            assert _all_same_bits(got[0:3], _ps3(ix, qa, betas[0], subset=sub)) and _all_same_bits(got[4:7], _ps3(ix, qb, betas[1], subset=sub))
        _check_int(_pd(ix, qa, qb, 1.0, 1.0), sa, sb, 1.0, 1.0, what="row labels without query labels")


# ---- 9. Gaussian data: the full bound, every pair --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_data_is_within_the_derived_bound(dim, dtype, seed):
    qa, x = gauss_case(dim, seed)
    qb = np.roll(qa, 1, axis=0)
    ba = float(np.float32(1.0 / np.sqrt(dim)))  # the float32 values the call receives
    bb = float(np.float32(0.5 / np.sqrt(dim)))
    ref = D.posterior_divergence(qa, qb, x, dtype, ba, bb)
    b8 = D.bounds(qa, qb, x, dtype, ba, bb, ref)
    with _index(x, dtype) as ix:
        got = _pd(ix, qa, qb, ba, bb)
        st_a = ix.posterior_stats(_dev(qa), temperature=1.0 / ba)
        st_b = ix.posterior_stats(_dev(qb), temperature=1.0 / bb)
    _check(got, ref, b8, ba, bb, what=f"gaussian dim {dim} {dtype}")
    # KL(p || r) = H(p, r) - H(p) by another route: H(p) and log_rel_b from posterior_stats of each side, E_p[s_b] dense in float64
    ent_a, lr_b = _np(st_a.entropy).astype(np.float64), _np(st_b.log_partition.log_rel).astype(np.float64)
    route = (lr_b - bb * ref.words[3]) - ent_a
    b6 = D.derived_bounds(ba, bb, ref.words, b8)
    sa_b = S.bounds(qa, x, dtype, ba, len(x), (ref.words[0], ref.words[1], ref.words[2], ref.var_a))
    b_route = S.entropy_bound(ba, (ref.words[0], ref.words[1], ref.words[2], ref.var_a), sa_b[1], sa_b[2]) + b8[5]
    err = np.abs(got[12].astype(np.float64) - route)
    print(f"gaussian dim {dim} {dtype}: max |kl_ab - (H(p, r) - H(p))| = {err.max():.3e}, bounds >= {b6[4].min():.3e} + {b_route.min():.3e}")
    assert (err <= b6[4] + b_route).all()


# ---- 10. kl_to ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES[:2])
def test_kl_to(dim, dtype, seed):
    teacher_np, x = gauss_case(dim, seed)
    student_np = np.roll(teacher_np, 1, axis=0)
    t_s, t_t = float(np.float32(np.sqrt(dim))), float(np.float32(2 * np.sqrt(dim)))
    bs, bt = float(np.float32(1.0 / t_s)), float(np.float32(1.0 / t_t))
    w = np.random.default_rng(seed).standard_normal(len(teacher_np)).astype(np.float32)
    with _index(x, dtype) as ix:
        calls = []
        real_mean = ix.posterior_mean
        ix.posterior_mean = lambda *a, **k: (calls.append(1), real_mean(*a, **k))[1]
        teacher = _dev(teacher_np).requires_grad_(True)
        student = _dev(student_np).requires_grad_(True)
        out = ix.kl_to(teacher, student, temperature=t_s, temperature_teacher=t_t)
        assert len(calls) == 2
        (out * _dev(w)).sum().backward()
        plain = ix.posterior_divergence(teacher.detach(), student.detach(), temperature_a=t_t, temperature_b=t_s)
        assert out.dtype == torch.float32 and torch.equal(out.detach().view(torch.int32), plain.kl_ab.view(torch.int32))
        assert teacher.grad is None and student.grad is not None and student.grad.dtype == student.dtype
        # the student does not require grad: no posterior_mean call
        out2 = ix.kl_to(teacher.detach(), student.detach(), temperature=t_s, temperature_teacher=t_t)
        assert len(calls) == 2 and not out2.requires_grad and torch.equal(out2.view(torch.int32), plain.kl_ab.view(torch.int32))
        grad = student.grad.cpu().numpy().astype(np.float64)
    # grad = w beta_s (E_student[x~] - E_teacher[x~]): each mean within its posterior_mean bound, the formula's three float32 roundings
    mean_s, mean_t = PM.posterior_mean(student_np, x, dtype, bs)[0], PM.posterior_mean(teacher_np, x, dtype, bt)[0]
    want = w.astype(np.float64)[:, None] * bs * (mean_s - mean_t)
    tol = np.abs(w).astype(np.float64)[:, None] * bs * (PM.device_bound(student_np, x, dtype, bs) + PM.device_bound(teacher_np, x, dtype, bt))
    tol = tol + 4 * P.U * np.abs(w).astype(np.float64)[:, None] * bs * (np.abs(mean_s) + np.abs(mean_t)) + 2.0 ** -140
    err = np.abs(grad - want)
    print(f"kl_to dim {dim} {dtype}: max |grad - float64| = {err.max():.3e}, largest share of the bound {(err / tol).max():.4f}")
    assert (err <= tol).all()


# ---- 11. node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_shards,capacity", [(1, 3000), (2, 3000), (3, 3000), (3, 12000)])
def test_node_index_folds_the_shards(n_shards, capacity):
    from vod_amd.index import HipNodeIndex

    nq, betas = 129, (1.0, 1.0 / 64.0)
    qa, qb, x, sa, sb = _pairs(65, nq)
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, "float16") as ix:
        flat = _pd(ix, qa, qb, *betas)
    with HipNodeIndex(65, capacity, [0] * n_shards) as nx:  # capacity 12000 on 3 shards: shard 0 holds every row, two shards stay empty
        nx.add(x.astype(np.float32))
        got = _words(nx.posterior_divergence(np.array(qa), np.array(qb), temperature_a=1.0 / betas[0], temperature_b=1.0 / betas[1]))
        lp_a = nx.log_partition(np.array(qa), temperature=1.0 / betas[0])
        lp_b = nx.log_partition(np.array(qb), temperature=1.0 / betas[1])
        nx.set_row_labels(labels)
        got_sub = _words(nx.posterior_divergence(np.array(qa), np.array(qb), temperature_a=1.0 / betas[0], temperature_b=1.0 / betas[1], subset=sub))
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (nq,) for a in got + got_sub)
    assert _same_bits(got[0], flat[0]) and _same_bits(got[4], flat[4])  # max_*: the flat index's bits
    assert _same_bits(got[0], lp_a.max_score) and _same_bits(got[1], lp_a.log_rel) and _same_bits(got[4], lp_b.max_score) and _same_bits(got[5], lp_b.log_rel)
    _check_int(got, sa, sb, *betas, what=f"node {n_shards} shards", node=True)
    _check_int(got_sub, sa, sb, *betas, elig, what=f"node {n_shards} shards, subset", node=True)


# ---- 12. beside searches, refusals, empty cases ------------------------------------------------------------------------------------------------
def test_a_call_between_search_async_and_finish_on_another_stream():
    qa, qb, x, _, _ = _pairs(768, 129)
    qd, qe = _dev(qa), _dev(qb)
    with _index(x, "float16") as ix:
        serial_s, serial_i = ix.search(qd, 100)
        serial = _words(ix.posterior_divergence(qd, qe, temperature_a=64.0, temperature_b=16.0))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            dv = ix.posterior_divergence(qd, qe, temperature_a=64.0, temperature_b=16.0)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert _all_same_bits(_words(dv), serial)
        assert ix.get_stat("last_overflow") == 0


def test_refusals_and_empty_cases():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    qa, qb, x, sa, sb = _pairs(65, 5)
    qd, qe = _dev(qa), _dev(qb)
    out = torch.full((8, 5), 123.0, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(h, a=qd, b=qe, code=2, nq=5, beta_a=1.0, beta_b=1.0, lab=None, n_lab=0, outs=tuple(out)):
        return lib.vodhip_index_posterior_divergence(h, None if a is None else ptr(a), None if b is None else ptr(b), code, nq,
                                                     ctypes.c_float(beta_a), ctypes.c_float(beta_b), None if lab is None else ptr(lab), n_lab,
                                                     *[None if o is None else ptr(o) for o in outs], None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    lab = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with _index(x[:300], "float16") as ix:
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, a=None), "invalid query / output pointers")
        refused(raw(ix._h, b=None), "invalid query / output pointers")
        for k in range(8):  # each NULL output
            refused(raw(ix._h, outs=tuple(None if j == k else out[j] for j in range(8))), "invalid query / output pointers")
        refused(raw(ix._h, nq=-1), "invalid query / output pointers")
        refused(raw(ix._h, nq=(1 << 19) + 1), "invalid query / output pointers")
        refused(raw(ix._h, code=3), "invalid q_dtype 3")
        for beta in (0.0, -1.0, float("inf"), float("nan")):
            refused(raw(ix._h, beta_a=beta), "beta_a must be finite and > 0")
            refused(raw(ix._h, beta_b=beta), "beta_b must be finite and > 0")
        refused(raw(ix._h, lab=lab, n_lab=0), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=65), "n_per_query must be in [1, 64]")
        refused(raw(ix._h, lab=lab, n_lab=2), "set the row labels first")
        for bad in (0.0, -2.0, float("inf")):
            with pytest.raises(_native.NativeLibraryError, match="beta_a must be finite"):
                ix.posterior_divergence(qd, qe, temperature_a=bad, temperature_b=1.0)
            with pytest.raises(_native.NativeLibraryError, match="beta_b must be finite"):
                ix.posterior_divergence(qd, qe, temperature_a=1.0, temperature_b=bad)
        with pytest.raises(ValueError):
            ix.posterior_divergence(qd, qe[:4])
        torch.cuda.synchronize()
        assert (out == 123.0).all()  # a refused call writes nothing
        assert raw(ix._h, a=None, b=None, nq=0, outs=(None,) * 8) == 0  # nq == 0: returns 0, needs nothing, writes nothing
        empty = ix.posterior_divergence(torch.zeros((0, 65), device="cuda"), torch.zeros((0, 65), device="cuda"))
        assert all(t.shape == (0,) for t in empty[:8]) and all(t.shape == (0,) for t in empty.stats_a[:3])
        # `out`: the eight words land in the caller's tensors
        mine = tuple(torch.empty(5, device="cuda") for _ in range(8))
        dv = ix.posterior_divergence(qd, qe, out=mine)
        assert dv.stats_a.max_score is mine[0] and dv.stats_a.mean_rel is mine[2] and dv.cross_rel_ab is mine[3]
        assert dv.stats_b.log_rel is mine[5] and dv.cross_rel_ba is mine[7]
        # temperature_b=None means "as a"; mixed query dtypes are accepted
        assert _all_same_bits(_words(ix.posterior_divergence(qd, qe, temperature_a=8.0)), _words(ix.posterior_divergence(qd, qe.half(), 8.0, 8.0)))
        # after all that the index still searches, and the call still works
        sc, _ = ix.search(qd, 3)
        np.testing.assert_array_equal(sc.cpu().numpy(), np.sort(sa[:, :300], axis=1)[:, ::-1][:, :3].astype(np.float32))
        _check_int(_pd(ix, qa, qb, 1.0, 1.0), sa[:, :300], sb[:, :300], 1.0, 1.0, what="after the refusals")
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="posterior_divergence is not supported on an L2 index"):
            ix.posterior_divergence(qd, qe)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipFlatIndex(65, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x[:300])
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            ix.posterior_divergence(qd, qe)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipNodeIndex(65, 600, [0, 0]) as nx:
        e = nx.posterior_divergence(np.array(qa), np.array(qb))  # empty
        assert np.isneginf(e.stats_a.max_score).all() and np.isneginf(e.stats_b.log_rel).all() and np.isnan(e.kl_ab).all() and np.isnan(e.cross_rel_ba).all()
        nx.add(x[:600].astype(np.float32))
        with pytest.raises(_native.NativeLibraryError, match="beta_b must be finite"):
            nx.posterior_divergence(np.array(qa), np.array(qb), temperature_b=-1.0)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.posterior_divergence(np.array(qa), np.array(qb), subset=np.zeros((5, 2), dtype=np.int32))
        assert nx.posterior_divergence(np.zeros((0, 65), dtype=np.float32), np.zeros((0, 65), dtype=np.float32)).kl_ab.shape == (0,)
        _check_int(_words(nx.posterior_divergence(np.array(qa), np.array(qb))), sa[:, :600], sb[:, :600], 1.0, 1.0, what="node after the refusals", node=True)
    with HipNodeIndex(65, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.posterior_divergence(np.array(qa), np.array(qb))
