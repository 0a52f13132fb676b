"""`HipFlatIndex.sample_posterior` / `HipNodeIndex.sample_posterior` on the GPU against the float64 restatement
(tests/sample_posterior_ref.py).

BAND EQUALITY.  With a / b the k-th / (k+1)-th float64 keys of a query and tol the largest `device_key_bound` over the query's rows
(derived, not fitted): every returned id has a float64 key >= a - tol, every eligible row that was not returned has one <= b + tol, the
returned keys are descending and each within its own bound of the float64 key of its row, and log_p / log_tau / log_weight are within
bounds propagated from tol and `partition_ref.device_bound`.  (Strictly, two keys that each move by tol can swap across a gap of 2 tol;
the one-tol form asserted here is the stronger statement.)  Integer data in [-8, 8] with beta a power of two (every score exact in
float32: the dot part of the bound is dropped) and N(0, 1) data with beta = dim^-1/2 (the full bound), on stores of 1, 255, 256, 257,
300, 3000 and 20000 rows, widths 64, 765, 768, batches 1, 64, 65, 130, 300, k = 1, 4, 32, 255, fp16 and bf16: 3000 rows are 12 tiles
(k = 4: the threshold path, k = 32: theta = -inf), at 20000 rows k = 32 takes the threshold path.  Then the edges (k >= ntotal, an
empty store, subset labels, stale rows, NaN / -inf / +inf scores, a clustered head, a duplicated row), determinism (batch, repeat, seed,
id_base), consistency (`log_partition`'s bits, `score_ids`, the status words), the node index and the refusals.
Measured maxima (MI355X): profiles/sample_posterior.json.
"""
import ctypes
import functools

import numpy as np
import pytest

import partition_ref as P
import sample_posterior_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16}
U = P.U
SEED = 0x1234567890ABCDEF
PLANES = ("ids", "scores", "log_p", "log_weight", "log_tau", "keys", "max", "log_rel")


def _index(x, dtype="float16", capacity=None, dim=None, **kw):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(dim or x.shape[1], capacity or max(len(x), 1), dtype=TDT[dtype], device=0, **kw)
    if len(x):
        ix.add(x)
    return ix


@functools.lru_cache(maxsize=None)
def _case(kind, d, n, nq):
    rng = np.random.default_rng(9000 + d + n + nq)
    if kind == "int":
        x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
        q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    else:
        x = rng.standard_normal((n, d)).astype(np.float32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
    for a in (q, x):
        a.setflags(write=False)
    return q, x


def _beta(kind, d):
    return (2.0 ** -5 if d <= 64 else 2.0 ** -7) if kind == "int" else float(np.float32(1.0 / np.sqrt(d)))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _sp(ix, q, k, beta, seed=SEED, check_lp=True, **kw):
    """the call's planes as NumPy; `log_partition`'s bits on the same index and the clean status words are asserted"""
    qd = _dev(q)
    r = ix.sample_posterior(qd, k, temperature=1.0 / beta, seed=seed, **kw)
    nq = len(q)
    assert r.ids.dtype == torch.int64 and r.ids.shape == (nq, k) and r.ids.is_cuda
    for t in (r.scores, r.log_p, r.log_weight):
        assert t.dtype == torch.float32 and t.shape == (nq, k)
    assert r.keys.dtype == torch.float32 and r.keys.shape == (nq, k + 1) and r.log_tau.shape == (nq,)
    assert ix.get_stat("last_sample_overflow") == 0 and ix.get_stat("last_sample_selfcheck") == 0
    if check_lp:
        lp = ix.log_partition(qd, temperature=1.0 / beta, subset=kw.get("subset"))
        for a, b in zip(r.log_partition, lp):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    out = {name: getattr(r, name).cpu().numpy() for name in ("ids", "scores", "log_p", "log_weight", "log_tau", "keys")}
    out["max"], out["log_rel"] = r.log_partition.max_score.cpu().numpy(), r.log_partition.log_rel.cpu().numpy()
    return out


def _check(got, q, x, dtype, k, beta, seed=SEED, query_offset=0, id_base=0, eligible=None, dot=False, what=""):
    """the band equality of the module docstring for every query; returns the largest |key - float64| / bound"""
    nq, n = len(q), len(x)
    s = P.scores(q, x, dtype)
    ref = R.sample_from_scores(s, k, beta, seed, query_offset, id_base, eligible)
    keymat = ref["key_matrix"]
    tolmat = R.key_bound(q, x, dtype, beta, seed, query_offset, id_base, dot=dot)
    can = keymat > -np.inf
    n_el = (~np.isnan(s) if eligible is None else (eligible & ~np.isnan(s))).sum(axis=1)
    e_dot = P.dot_bound(q, x, dtype, eligible) if dot else np.zeros(nq)
    pb = P.device_bound(q, x, dtype, beta, np.maximum(n_el, 1), dot=dot)
    worst = 0.0
    for a in range(nq):
        ids, keys = got["ids"][a], got["keys"][a]
        count = min(k, int(can[a].sum()))
        assert (ids[:count] >= 0).all() and (ids[count:] == -1).all(), (what, a)
        for name in ("scores", "log_p", "log_weight"):
            assert np.isneginf(got[name][a][count:]).all(), (what, a, name)
        assert np.isneginf(keys[min(int(can[a].sum()), k + 1):]).all(), (what, a)
        if count == 0:
            assert np.isneginf(got["log_tau"][a]), (what, a)
            continue
        rows = ids[:count] - id_base
        assert ((rows >= 0) & (rows < n)).all() and len(set(rows.tolist())) == count, (what, a)
        assert can[a][rows].all(), (what, a, "an ineligible row was drawn")
        tol = tolmat[a][can[a]].max()
        ka, kb = ref["keys"][a][count - 1], ref["keys"][a][k]
        assert (keymat[a][rows] >= ka - tol).all(), (what, a, "a returned row below the band")
        rest = np.ones(n, dtype=bool)
        rest[rows] = False
        if (rest & can[a]).any():
            assert keymat[a][rest & can[a]].max() <= kb + tol, (what, a, "a better row was left out")
        assert (np.diff(keys[:count]) <= 0).all(), (what, a)
        err = np.abs(keys[:count].astype(np.float64) - keymat[a][rows])
        assert (err <= tolmat[a][rows]).all(), (what, a, (err / tolmat[a][rows]).max())
        worst = max(worst, float((err / tolmat[a][rows]).max()))
        # scores: the scan's float32 dot product
        assert (np.abs(got["scores"][a][:count].astype(np.float64) - s[a][rows]) <= e_dot[a]).all(), (what, a)
        # log_p = beta (s - max) - log_rel in double from the float32 words, rounded once
        lp = beta * (s[a][rows] - ref["max"][a]) - ref["log_rel"][a]
        d_lp = 2 * beta * e_dot[a] + pb[a]
        t_lp = d_lp + 1.001 * U * np.abs(lp) + 1e-37
        assert (np.abs(got["log_p"][a][:count] - lp) <= t_lp).all(), (what, a, "log_p")
        if np.isneginf(kb):
            assert np.isneginf(got["log_tau"][a]) and np.isneginf(keys[k]), (what, a)
            assert np.array_equal(got["log_weight"][a][:count], got["log_p"][a][:count]), (what, a)
            continue
        assert abs(float(keys[k]) - kb) <= tol, (what, a, "key_{k+1}")
        # log_tau = (key_{k+1} - fl(beta max)) - log_rel in float32: three roundings behind the inputs' own errors
        lt = ref["log_tau"][a]
        bm = abs(beta * ref["max"][a])
        d_lt = tol + beta * e_dot[a] + pb[a]
        t_lt = d_lt + 1.001 * U * (abs(kb) + 2 * bm + abs(lt) + 3 * d_lt)
        assert abs(got["log_tau"][a] - lt) <= t_lt, (what, a, "log_tau")
        # log_weight = log_p - f(log_p - log_tau), 0 < f' <= 1: moves by at most 2 d_lp + d_lt, then rounds once
        lw = R.weights(lp, lt)
        t_lw = 2 * d_lp + d_lt + 1.001 * U * np.abs(lw) + 1e-37
        assert (np.abs(got["log_weight"][a][:count] - lw) <= t_lw).all(), (what, a, "log_weight")
    print(f"{what}: max |key - float64| / bound = {worst:.3f}")
    return worst


# ---- band equality over sizes, widths, batches, k, dtypes -----------------------------------------------------------------------------------
BAND = [  # rows, dim, nq, k, dtype
    (1, 64, 1, 1, "float16"),
    (255, 64, 64, 4, "bfloat16"),
    (256, 765, 65, 32, "float16"),
    (257, 768, 130, 255, "float16"),
    (300, 64, 300, 255, "bfloat16"),
    (3000, 765, 300, 4, "float16"),      # 12 tiles, k + 1 = 5: the threshold path
    (3000, 768, 65, 32, "bfloat16"),     # 12 tiles < k + 1: theta = -inf
    (20000, 64, 130, 32, "float16"),     # 79 tiles, k + 1 = 33: the threshold path
    (20000, 768, 64, 255, "bfloat16"),   # 79 tiles < 256: every row is a candidate, the select loops over 12 chunks
    (20000, 765, 1, 1, "float16"),
    (20000, 64, 65, 4, "bfloat16"),
]


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("n,d,nq,k,dtype", BAND)
def test_band_equality(n, d, nq, k, dtype, kind):
    q, x = _case(kind, d, n, nq)
    beta = _beta(kind, d)
    with _index(x, dtype) as ix:
        got = _sp(ix, q, k, beta)
        tiles = (n + 255) // 256
        print(f"tiles {tiles} k+1 {k + 1}: candidates max {ix.get_stat('last_sample_max_candidates')}, emit groups "
              f"{ix.get_stat('last_sample_emit_groups')} skipped {ix.get_stat('last_sample_emit_skipped')}")
        assert ix.get_stat("last_sample_max_candidates") <= min((n + 255) // 256, k + 1) * 256
    _check(got, q, x, dtype, k, beta, dot=kind == "gauss", what=f"{kind} n {n} d {d} nq {nq} k {k} {dtype}")


# ---- edges -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_k_at_least_ntotal_and_an_empty_store(dtype):
    q, x = _case("int", 64, 300, 300)
    beta = 2.0 ** -5
    for n, k in ((5, 8), (5, 5), (255, 255), (256, 255)):
        with _index(x[:n], dtype) as ix:
            got = _sp(ix, q[:65], k, beta)
        _check(got, q[:65], x[:n], dtype, k, beta, what=f"k {k} >= n {n} {dtype}")
        if k >= n:
            assert np.isneginf(got["log_tau"]).all() and np.array_equal(_bits(got["log_weight"]), _bits(got["log_p"]))
            total = np.exp(got["log_p"][:, :n].astype(np.float64)).sum(axis=1)
            pb = P.device_bound(q[:65], x[:n], dtype, beta, n, dot=False)
            lp_max = np.abs(got["log_p"][:, :n]).max(axis=1)  # every row returned: the probabilities sum to 1 (each log_p within
            assert (np.abs(total - 1) <= np.expm1(pb + 1.001 * U * lp_max)).all()  # PB of the truth, rounded once)
    with _index(x[:0], dtype, capacity=8, dim=64) as ix:
        got = _sp(ix, q[:5], 3, beta)
    assert (got["ids"] == -1).all() and np.isneginf(got["max"]).all()
    for name in ("scores", "log_p", "log_weight", "log_tau", "keys"):
        assert np.isneginf(got[name]).all(), name


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("nq,k", [(8, 4), (132, 32)])
def test_subset_labels(nq, k, dtype):
    q, x = _case("int", 64, 3000, 300)
    beta = 2.0 ** -5
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    patterns = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)  # one label, two, unrestricted, a label no row has
    sub = patterns[np.arange(nq) % 4]
    elig = np.stack([(labels[None, :] == row[row != -1][:, None]).any(axis=0) if (row != -1).any() else np.ones(len(x), dtype=bool)
                     for row in sub])
    with _index(x, dtype) as ix:
        ix.set_row_labels(labels)
        got = _sp(ix, q[:nq], k, beta, subset=sub)
        _check(got, q[:nq], x, dtype, k, beta, eligible=elig, what=f"subset nq {nq} k {k} {dtype}")
        assert (got["ids"][3::4] == -1).all() and np.isneginf(got["keys"][3::4]).all()  # no allowed row: all pads
        assert (labels[got["ids"][0::4]] == 0).all()
        _check(_sp(ix, q[:nq], k, beta), q[:nq], x, dtype, k, beta, what="row labels without query labels")


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_stale_rows_are_never_returned(dtype):
    q, x = _case("int", 64, 3000, 300)
    beta = 2.0 ** -5
    with _index(x, dtype, capacity=3000) as ix:
        ix.reset()
        ix.add(x[2300:])  # 700 rows; rows 700 .. 2999 of the store still hold the first ingest
        got = _sp(ix, q[:65], 32, beta)
        assert got["ids"].max() < 700
        _check(got, q[:65], x[2300:], dtype, 32, beta, what=f"reset {dtype}")
        got = _sp(ix, q[:65], 1, beta)  # 3 tiles, k + 1 = 2: the threshold path over a stale tail
        _check(got, q[:65], x[2300:], dtype, 1, beta, what=f"reset k 1 {dtype}")


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_nan_and_infinite_scores(dtype):
    q, x = _case("int", 64, 3000, 300)
    q = np.array(q[:70])
    q[:, 0] = 1.0
    beta = 2.0 ** -5
    xn = np.array(x)
    xn[7, 3] = np.nan       # every score of row 7 is NaN: never drawn
    xn[300, 0] = -np.inf    # a -inf score for every query: probability 0, never drawn
    for k in (4, 255):
        with _index(xn, dtype) as ix:
            got = _sp(ix, q, k, beta)
        assert not np.isin(got["ids"], (7, 300)).any()
        _check(got, q, xn, dtype, k, beta, what=f"NaN and -inf rows k {k} {dtype}")
    xi = np.array(x)
    xi[2999, 0] = np.inf    # +inf for every query: log Z is not finite, all pads
    with _index(xi, dtype) as ix:
        got = _sp(ix, q, 4, beta)
    assert (got["ids"] == -1).all() and np.isposinf(got["max"]).all()
    for name in ("scores", "log_p", "log_weight", "log_tau", "keys"):
        assert np.isneginf(got[name]).all(), name


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_a_clustered_head_and_a_duplicated_row(dtype):
    q, x = _case("int", 64, 3000, 300)
    q = np.array(q[:65])
    q[:, 0] = 256.0
    xc = np.array(x)
    xc[:, 0] = 0
    xc[1000:1040, 0] = 8    # the 40 best rows are consecutive (24 in tile 3, 16 in tile 4): beta * 2048 = 64 above the rest (sd 6.6)
    beta = 2.0 ** -5
    with _index(xc, dtype) as ix:
        got = _sp(ix, q, 4, beta)
        print("clustered head: candidates max", ix.get_stat("last_sample_max_candidates"), "of", ix.get_stat("last_sample_candidates"))
        assert ix.get_stat("last_sample_max_candidates") <= 5 * 256
    assert ((got["ids"] >= 1000) & (got["ids"] < 1040)).all()
    _check(got, q, xc, dtype, 4, beta, what=f"clustered head {dtype}")
    xd = np.array(x[:300])
    xd[11] = xd[10]         # equal scores, different noise: different keys
    with _index(xd, dtype) as ix:
        got = _sp(ix, q, 255, 2.0 ** -5)
    _check(got, q, xd, dtype, 255, 2.0 ** -5, what=f"duplicated row {dtype}")
    both = 0
    for a in range(len(q)):
        at10, at11 = np.flatnonzero(got["ids"][a] == 10), np.flatnonzero(got["ids"][a] == 11)
        if len(at10) and len(at11):
            both += 1
            assert got["scores"][a][at10[0]] == got["scores"][a][at11[0]] and got["keys"][a][at10[0]] != got["keys"][a][at11[0]]
    assert both > 10


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("n,k", [(3000, 4), (3000, 32)])
def test_a_query_has_the_same_bits_in_any_batch_and_on_every_repeat(n, k, dtype):
    q, x = _case("gauss", 765, n, 300)
    beta = _beta("gauss", 765)
    with _index(x, dtype) as ix:
        a = _sp(ix, q, k, beta)
        b = _sp(ix, q, k, beta)
        for name in PLANES:
            assert np.array_equal(_bits(a[name]), _bits(b[name])), name
        for j in (0, 63, 64, 217, 299):
            one = _sp(ix, q[j : j + 1], k, beta, query_offset=j)
            for name in PLANES:
                assert np.array_equal(_bits(a[name][j : j + 1]), _bits(one[name])), (j, name)
        part = _sp(ix, q[200:265], k, beta, query_offset=200)  # the 128-query instantiation against the 300-query batch
        for name in PLANES:
            assert np.array_equal(_bits(a[name][200:265]), _bits(part[name])), name
        other = _sp(ix, q, k, beta, seed=SEED + 1, check_lp=False)
        assert (other["ids"] != a["ids"]).any(axis=1).mean() > 0.9
        shifted = _sp(ix, q, k, beta, query_offset=1, check_lp=False)  # another stream index: another draw
        assert (shifted["ids"] != a["ids"]).any(axis=1).mean() > 0.9
        assert np.array_equal(_bits(shifted["max"]), _bits(a["max"]))


@pytest.mark.parametrize("id_base", [1000, 1001, 1002, 1003, (1 << 34) + 6])
def test_id_base_on_a_slice_returns_the_whole_store_restricted_to_it(id_base):
    q, x = _case("int", 64, 3000, 300)
    beta, k, lo = 2.0 ** -5, 32, 1000
    if id_base < 3000:  # the whole store with only the slice's rows allowed: the same ids, keys and scores, bit for bit
        labels = ((np.arange(len(x)) >= id_base) & (np.arange(len(x)) < id_base + 300)).astype(np.int32)
        with _index(x, "float16") as ix:
            ix.set_row_labels(labels)
            whole = _sp(ix, q[:65], k, beta, subset=np.ones((65, 1), dtype=np.int32))
        lo = id_base
    with _index(x[lo : lo + 300], "float16") as ix:
        part = _sp(ix, q[:65], k, beta, id_base=id_base)
    _check(part, q[:65], x[lo : lo + 300], "float16", k, beta, id_base=id_base, what=f"id_base {id_base}")
    assert part["ids"].min() >= id_base and part["ids"].max() < id_base + 300
    if id_base < 3000:
        for name in ("ids", "keys", "scores"):
            assert np.array_equal(_bits(whole[name]), _bits(part[name])), name


# ---- consistency ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int", "gauss"])
def test_scores_equal_score_ids(kind):
    q, x = _case(kind, 765, 3000, 300)
    beta = _beta(kind, 765)
    with _index(x, "float16") as ix:
        got = _sp(ix, q[:130], 32, beta)
        listed = ix.score_ids(_dev(q[:130]), _dev(got["ids"]))
        listed = (listed[0] if isinstance(listed, tuple) else listed).cpu().numpy()
    if kind == "int":
        assert np.array_equal(_bits(listed), _bits(got["scores"]))
    else:  # the listed-row kernel adds in another order: both are within the dot bound of the float64 score
        s = P.scores(q[:130], x, "float16")
        want = np.take_along_axis(s, got["ids"], axis=1)
        e = P.dot_bound(q[:130], x, "float16")[:, None]
        assert (np.abs(listed - want) <= e).all() and (np.abs(got["scores"] - want) <= e).all()


def test_a_call_between_search_async_and_finish_on_another_stream():
    q, x = _case("int", 768, 3000, 65)
    qd = _dev(q)
    with _index(x, "float16") as ix:
        serial_s, serial_i = ix.search(qd, 100)
        serial = ix.sample_posterior(qd, 32, temperature=128.0, seed=SEED)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        s, i = ix.search_async(qd, 100)
        with torch.cuda.stream(side):
            sp = ix.sample_posterior(qd, 32, temperature=128.0, seed=SEED)
        ix.finish()
        side.synchronize()
        torch.cuda.synchronize()
        assert torch.equal(s, serial_s) and torch.equal(i, serial_i)
        assert torch.equal(sp.ids, serial.ids) and torch.equal(sp.keys.view(torch.int32), serial.keys.view(torch.int32))
        assert torch.equal(sp.log_weight.view(torch.int32), serial.log_weight.view(torch.int32))
        assert ix.get_stat("last_overflow") == 0 and ix.get_stat("last_sample_overflow") == 0


# ---- node index --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 255])
def test_node_index_merges_two_shards(k):
    from vod_amd.index import HipNodeIndex

    q, x = _case("int", 64, 3000, 300)
    nq, beta = 130, 2.0 ** -5
    labels = (np.arange(len(x)) % 4).astype(np.int32)
    sub = np.array([[0, -1], [1, 2], [-1, -1], [9, -1]], dtype=np.int32)[np.arange(nq) % 4]
    with _index(x, "float16") as ix:
        flat = _sp(ix, q[:nq], k, beta, query_offset=7)
        ix.set_row_labels(labels)
        flat_sub = _sp(ix, q[:nq], k, beta, query_offset=7, subset=sub)
    with HipNodeIndex(64, 3000, [0, 0]) as nx:
        nx.add(np.array(x))
        got = nx.sample_posterior(np.array(q[:nq]), k, temperature=1.0 / beta, seed=SEED, query_offset=7)
        nx.set_row_labels(labels)
        got_sub = nx.sample_posterior(np.array(q[:nq]), k, temperature=1.0 / beta, seed=SEED, query_offset=7, subset=sub)
    pb = P.device_bound(q[:nq], x, "float16", beta, len(x), dot=False)
    for res, ref in ((got, flat), (got_sub, flat_sub)):
        assert isinstance(res.ids, np.ndarray) and res.ids.dtype == np.int64 and res.ids.shape == (nq, k)
        assert np.array_equal(res.ids, ref["ids"])
        assert np.array_equal(_bits(res.scores), _bits(ref["scores"])) and np.array_equal(_bits(res.keys), _bits(ref["keys"]))
        assert np.array_equal(_bits(res.log_partition.max_score), _bits(ref["max"]))
        # the folded log_rel and the flat one are each within PB (+ the fold's 4 u (1 + log n)) of the truth; the words round once
        fold = 2 * (pb + 4 * U * (1 + np.log(len(x))))
        live = res.ids >= 0
        for name, mult in (("log_p", 1.0), ("log_weight", 3.0)):
            a, b = getattr(res, name), ref[name]
            assert np.array_equal(np.isneginf(a), np.isneginf(b))
            err = np.abs(np.where(live, a, 0.0).astype(np.float64) - np.where(live, b, 0.0))
            assert (err <= mult * fold[:, None] + 2.002 * U * np.abs(np.where(live, b, 0.0))).all(), (name, err.max())
        lt_a, lt_b = res.log_tau, ref["log_tau"]
        fin = np.isfinite(lt_b)
        assert np.array_equal(np.isfinite(lt_a), fin) and (np.abs(lt_a[fin] - lt_b[fin]) <= fold[fin] + 2.002 * U * np.abs(lt_b[fin])).all()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from vod_amd import _native
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    lib = _native.load_library()
    q, x = _case("int", 64, 300, 300)
    qd = _dev(q[:5])
    k = 3
    f = lambda *shape: torch.full(shape, 123.0, device="cuda")  # noqa: E731
    om, ol, sc, lp, lw, keys = f(5), f(5), f(5, k), f(5, k), f(5, k), f(5, k + 1)
    ids = torch.full((5, k), 123, dtype=torch.int64, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(h, queries=qd, nq=5, k=k, beta=1.0, qoff=0, base=0, ids=ids, keys=keys):
        return lib.vodhip_index_sample_posterior(h, ptr(queries), 2, nq, k, ctypes.c_float(beta), ctypes.c_uint64(SEED), qoff, base, None, 0,
                                                 ptr(om), ptr(ol), ptr(ids), ptr(sc), ptr(lp), ptr(lw), ptr(keys), None)

    def refused(rc, text):
        assert rc != 0 and text in lib.vodhip_last_error().decode(), lib.vodhip_last_error()

    with _index(x, "float16") as ix:
        refused(raw(None), "index is NULL")
        refused(raw(ix._h, k=0), "k=0: k must be in [1, 255]")
        refused(raw(ix._h, k=256), "k=256: k must be in [1, 255]")
        refused(raw(ix._h, k=-3), "k must be in [1, 255]")
        refused(raw(ix._h, qoff=-1), "query_offset")
        refused(raw(ix._h, qoff=(1 << 32) - 4), "query_offset")
        refused(raw(ix._h, base=-1), "id_base must be >= 0")
        refused(raw(ix._h, ids=None), "invalid query / output pointers")
        refused(raw(ix._h, keys=None), "invalid query / output pointers")
        refused(raw(ix._h, queries=None), "invalid query / output pointers")
        refused(raw(ix._h, beta=0.0), "beta must be finite and > 0")
        torch.cuda.synchronize()
        for t in (om, ol, sc, lp, lw, keys, ids):
            assert (t == 123).all()  # a refused call writes nothing
        assert raw(ix._h, queries=None, nq=0, ids=None, keys=None) == 0  # nq == 0: returns 0, needs nothing
        assert raw(ix._h, qoff=(1 << 32) - 5) == 0  # the last admissible stream indices
        torch.cuda.synchronize()
        assert (ids >= 0).all() and (ids < 300).all()
        empty = ix.sample_posterior(torch.zeros((0, 64), device="cuda"), 3, seed=1)
        assert empty.ids.shape == (0, 3) and empty.keys.shape == (0, 4) and empty.log_tau.shape == (0,)
        with pytest.raises(ValueError, match="k must be in"):
            ix.sample_posterior(qd, 256, seed=1)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipFlatIndex(64, 300, dtype=torch.float16, device=0, metric="l2") as ix:
        ix.add(x)
        with pytest.raises(_native.NativeLibraryError, match="sample_posterior is not supported on an L2 index"):
            ix.sample_posterior(qd, 3, seed=1)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipFlatIndex(64, 300, dtype=torch.float16, device=0, exact_f32=True) as ix:
        ix.add(x)
        with pytest.raises(_native.NativeLibraryError, match="sample_posterior is not supported on a VODHIP_EXACT_F32"):
            ix.sample_posterior(qd, 3, seed=1)
        assert ix.search(qd, 3)[0].shape == (5, 3)
    with HipNodeIndex(64, 600, [0, 0]) as nx:
        got = nx.sample_posterior(np.array(q[:5]), 3, seed=1)  # empty: all pads
        assert (got.ids == -1).all() and np.isneginf(got.keys).all() and np.isneginf(got.log_tau).all()
        nx.add(np.array(x))
        with pytest.raises(ValueError, match="k must be in"):
            nx.sample_posterior(np.array(q[:5]), 0, seed=1)
        with pytest.raises(_native.NativeLibraryError, match="set the row labels first"):
            nx.sample_posterior(np.array(q[:5]), 3, seed=1, subset=np.zeros((5, 2), dtype=np.int32))
        assert nx.sample_posterior(np.zeros((0, 64), dtype=np.float32), 3, seed=1).ids.shape == (0, 3)
        assert (nx.sample_posterior(np.array(q[:5]), 3, seed=1).ids >= 0).all()
    with HipNodeIndex(64, 600, [0, 0], exact_f32=True) as nx:
        with pytest.raises(_native.NativeLibraryError, match="VODHIP_EXACT_F32"):
            nx.sample_posterior(np.array(q[:5]), 3, seed=1)
