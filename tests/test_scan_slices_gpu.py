"""The whole-store scans in query slices below 1024 (`set_param("scan_temp_bytes", ...)`, vod_amd/csrc/scan_slices.h).

Nine entry points cut a batch into slices that keep their temporaries under a budget; at the sizes the library is built for the
slice is 64 .. 384 queries, at every other shape of this suite it is 1024.  Here the budget is lowered so that small stores run in
slices of 64 (through the clamp, budget 1), 128, 256 and 384 queries, and every output of every sliced call must be the bytes of the
same call under the default budget: launches at `q_first` 64, 128, 256, 384, ..., offsets into queries of every input dtype, subset
labels, listed ids, thresholds, tie ids, the staged `g`, the forward's saved words, the `lims` carried from slice to slice, the
sampler's per-query stream index, the pair staging of the divergence, and temporaries sized for one slice and reused by the next.
Every case asserts through `get_stat("last_scan_slice")` that the slice it names ran.  The outputs of every entry point are buffers
the test fills with NaN / a marker first (`out=`, or the C call itself where the wrapper allocates), so a slice that leaves its outputs
unwritten cannot pass on what the unsliced call left in recycled device memory; the wrappers and the autograd functions on top
(`log_z`, `kl_to`, `expected_values`, `outranking`, `posterior_support`, `order="score"`) are then compared through their own results.  Sliced results are also checked against the
float64 restatements of the operations' own test files, inside their bounds; no tolerance is introduced here.

Stores: 600 rows x dim 65 (three row tiles, the last partial; two K steps), `VODHIP_READOUT_GROUP_ROWS + 300` rows for the read-outs
(two groups) and 16384 + 300 rows x dim 64 for `posterior_mean` alone (its two groups); integer values in [-8, 8], fp16 and bf16.
`score_ids` / `listed_scores` of the flat index never slice (they gather the listed rows); the PICK mode of the rank scan
(`vodhip_index_scan_score_ids`) is what `HipNodeIndex.rank_ids` runs on every shard, and is covered there.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import range_ref as G
import readout_ref as RO

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_posterior_expectation_gpu import _check as _check_expectation  # noqa: E402
from test_posterior_mean_gpu import _check as _check_mean  # noqa: E402
from test_posterior_stats_gpu import _check_int as _check_stats  # noqa: E402

TDT = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}
DEFAULT_SLICE = 1024
NQ = 450
N_COLS = 65
BETAS = [1.0, 1.0 / 64.0, 4.0]
ROWS = {"small": (600, 65), "groups": (RO.GROUP_ROWS + 300, 65), "mean_groups": (16384 + 300, 64)}

# (queries, slice, store dtype, query dtype, subset labels): 450 = 384 + 66 (the tail runs at nq_pad 128) = 3 x 128 + 66 = 256 + 194 =
# 7 x 64 + 2; 130 = 64 + 64 + 2; 64 and 65 = one slice, and one slice plus one query; 256 = 2 x 128 (no tail)
CASES = [
    (450, 384, "float16", "float32", False),
    (450, 128, "bfloat16", "float16", True),
    (450, 64, "float16", "bfloat16", False),
    (130, 64, "bfloat16", "float32", True),
    (64, 64, "float16", "float16", False),
    (65, 64, "bfloat16", "bfloat16", True),
    (256, 128, "float16", "float32", False),
    (450, 256, "bfloat16", "float16", False),
]
CASE_IDS = [f"nq{c[0]}-slice{c[1]}-{c[2]}-q{c[3]}{'-subset' if c[4] else ''}" for c in CASES]
assert {c[1] for c in CASES} == {64, 128, 256, 384} and {c[3] for c in CASES} == set(TDT) and any(c[4] for c in CASES)
each_case = pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)


@functools.lru_cache(maxsize=None)
def _case(kind):
    """integer rows, two query sets, a value table and row labels; every score is exact in float32 and both store dtypes hold the data"""
    n, d = ROWS[kind]
    rng = np.random.default_rng(600 + n)
    c = SimpleNamespace(n=n, d=d)
    c.x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    c.q = rng.integers(-8, 9, size=(NQ, d)).astype(np.float32)
    c.q2 = rng.integers(-8, 9, size=(NQ, d)).astype(np.float32)
    c.v = rng.integers(-8, 9, size=(n, N_COLS)).astype(np.float32)
    c.labels = rng.integers(0, 2, size=n).astype(np.int32)  # a query allows label q % 2: about half the rows (test_store_scan_gpu.py)
    c.sub = (np.arange(NQ, dtype=np.int32) % 2)[:, None]
    c.elig = c.labels[None, :] == c.sub
    c.s = c.q.astype(np.float64) @ c.x.astype(np.float64).T
    assert np.array_equal(c.s.astype(np.float32).astype(np.float64), c.s)
    assert len(np.unique(np.concatenate([c.q, c.q2]), axis=0)) == 2 * NQ  # pairwise distinct: a wrong offset changes the answer
    for a in vars(c).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@pytest.fixture(scope="module")
def store():
    """`store(dtype, kind)`: the index over `_case(kind)` with its labels and value table, built once, budget reset to the default"""
    from vod_amd.index import HipFlatIndex

    made = {}

    def get(dtype, kind="small"):
        if (dtype, kind) not in made:
            c = _case(kind)
            ix = HipFlatIndex(c.d, c.n, dtype=TDT[dtype], device=0)
            ix.add(c.x)
            ix.set_row_labels(c.labels)
            if kind != "mean_groups":
                ix.set_row_values(c.v)
            made[dtype, kind] = ix
        ix = made[dtype, kind]
        ix.set_param("scan_temp_bytes", 0)
        return ix

    yield get
    for ix in made.values():
        ix.close()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


POISON_INT = -(2 ** 62)


def _poison(shape, dtype=torch.float32):
    """an output buffer of the test's own, filled with NaN / POISON_INT: what a slice leaves unwritten cannot hold a right answer that
    an earlier call left in recycled memory"""
    return torch.full(tuple(shape), float("nan") if dtype == torch.float32 else POISON_INT, dtype=dtype, device="cuda")


def _np(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)


def _same_bytes(got, want, what=""):
    """every output tensor, as integer words"""
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        a, b = _np(a), _np(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.dtype in (np.float32, np.int64), (what, k, a.dtype)
        ua, ub = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
        diff = np.argwhere(ua != ub)
        assert diff.size == 0, f"{what}: output {k} differs at {len(diff)} places, first at {tuple(diff[0])}"


def _budget_for(per_query, wanted):
    return 1 if wanted == 64 else per_query * wanted  # 64: through the clamp (the temporaries then exceed the budget)


def _sliced(ix, call, wanted, what=""):
    """`call()` under the default budget and in slices of `wanted`; both must be the same bytes.  Returns the sliced outputs."""
    ix.set_param("scan_temp_bytes", 0)
    want = [_np(a) for a in call()]
    assert ix.get_stat("last_scan_slice") == DEFAULT_SLICE, what
    per_query = ix.get_stat("last_scan_per_query_bytes")
    assert per_query >= 1
    ix.set_param("scan_temp_bytes", _budget_for(per_query, wanted))
    try:
        got = [_np(a) for a in call()]
        assert ix.get_stat("last_scan_slice") == wanted, (what, ix.get_stat("last_scan_slice"), per_query)
        assert ix.get_stat("last_scan_per_query_bytes") == per_query
    finally:
        ix.set_param("scan_temp_bytes", 0)
    _same_bytes(got, want, what)
    return got


def _setup(store, i, kind="small"):
    nq, wanted, dtype, qdt, subset = CASES[i]
    c = _case(kind)
    ix = store(dtype, kind)
    qd = _dev(c.q[:nq]).to(TDT[qdt])
    kw = {"subset": _dev(c.sub[:nq])} if subset else {}
    elig = c.elig[:nq] if subset else None
    return SimpleNamespace(nq=nq, wanted=wanted, dtype=dtype, qdt=qdt, subset=subset, c=c, ix=ix, qd=qd, kw=kw, elig=elig,
                           what=f"{kind} {CASE_IDS[i]}")


def _kind(i):
    """the read-outs meet both stores: two groups in half of the cases"""
    return "groups" if i % 2 == 0 else "small"


# ---- the CPU arithmetic is what the library runs ----------------------------------------------------------------------------------------
def test_budget_selects_the_slice_and_zero_restores_the_default(store):
    from vod_amd import _native

    a, b = store("float16"), store("bfloat16")
    qd = _dev(_case("small").q[:130])
    default = a.get_stat("scan_temp_bytes")
    assert default == 256 << 20 == b.get_stat("scan_temp_bytes")
    a.posterior_stats(qd)
    per_query = a.get_stat("last_scan_per_query_bytes")
    assert per_query == 3 * 16 and a.get_stat("last_scan_slice") == DEFAULT_SLICE  # three row tiles of float4 partials
    for wanted in (64, 128, 256, 384, 512, 1024):
        a.set_param("scan_temp_bytes", _budget_for(per_query, wanted))
        a.posterior_stats(qd)
        assert a.get_stat("last_scan_slice") == wanted
        b.posterior_stats(qd)  # a budget set on one index does not change another
        assert b.get_stat("last_scan_slice") == DEFAULT_SLICE and b.get_stat("scan_temp_bytes") == default
    a.set_param("scan_temp_bytes", per_query * 128 - 1)  # one byte short of 128 queries
    a.posterior_stats(qd)
    assert a.get_stat("last_scan_slice") == 64
    a.set_param("scan_temp_bytes", 0)
    assert a.get_stat("scan_temp_bytes") == default
    a.posterior_stats(qd)
    assert a.get_stat("last_scan_slice") == DEFAULT_SLICE
    with pytest.raises(_native.NativeLibraryError, match="scan_temp_bytes"):
        a.set_param("scan_temp_bytes", -1)
    assert a.get_stat("scan_temp_bytes") == default



# ---- posterior_stats -----------------------------------------------------------------------------------------------------------------------
@each_case
def test_posterior_stats(store, i):
    t = _setup(store, i)
    beta = BETAS[i % 3]

    def call():
        out = tuple(_poison((t.nq,)) for _ in range(4))  # (max_score, log_rel, mean_rel, var)
        r = t.ix.posterior_stats(t.qd, temperature=1.0 / beta, out=out, **t.kw)
        return [*out, r.entropy, r.mean_score, r.log_partition.log_z]

    got = _sliced(t.ix, call, t.wanted, t.what)
    _check_stats(tuple(got), t.c.s[: t.nq], beta, t.elig, what=t.what)


# ---- posterior_mean / log_z ----------------------------------------------------------------------------------------------------------------
def _mean_and_log_z(t, beta):
    def mean():
        out = (_poison((t.nq,)), _poison((t.nq,)), _poison((t.nq, t.c.d)))  # (max_score, log_rel, mean)
        r = t.ix.posterior_mean(t.qd, temperature=1.0 / beta, out=out, **t.kw)
        return [out[2], r.log_partition.log_z, out[0], out[1]]

    def log_z():
        q = t.qd.clone().requires_grad_(True)
        lz = t.ix.log_z(q, 1.0 / beta, t.kw.get("subset"))
        lz.backward(torch.linspace(0.5, 2.0, t.nq, device="cuda"))
        return [lz.detach(), q.grad.float()]

    got = _sliced(t.ix, mean, t.wanted, t.what)
    lz = _sliced(t.ix, log_z, t.wanted, t.what)
    _same_bytes([lz[0]], [got[1]], t.what)  # log_z is the forward's word
    _check_mean(tuple(got), t.c.q[: t.nq], t.c.x, t.dtype, beta, t.elig, what=t.what)


@each_case
def test_posterior_mean_and_log_z(store, i):
    _mean_and_log_z(_setup(store, i, _kind(i)), BETAS[(i + 1) % 3])


@pytest.mark.parametrize("i", [0, 1], ids=[CASE_IDS[0], CASE_IDS[1]])
def test_posterior_mean_over_two_of_its_own_groups(store, i):
    _mean_and_log_z(_setup(store, i, "mean_groups"), 1.0 / 64.0)


# ---- posterior_expectation and its backward -------------------------------------------------------------------------------------------------
def _expectation_call(t, T):
    def call():
        out = (_poison((t.nq,)), _poison((t.nq,)), _poison((t.nq, N_COLS)))  # (max_score, log_rel, values)
        r = t.ix.posterior_expectation(t.qd, temperature=T, out=out, **t.kw)
        return [out[2], r.log_partition.log_z, out[0], out[1]]

    return call


@each_case
def test_posterior_expectation(store, i):
    t = _setup(store, i, _kind(i))
    beta = BETAS[(i + 2) % 3]
    got = _sliced(t.ix, _expectation_call(t, 1.0 / beta), t.wanted, t.what)
    _check_expectation(tuple(got), t.c.q[: t.nq], t.c.x, t.c.v, t.dtype, beta, t.elig, dot=False, what=t.what)


@each_case
def test_posterior_expectation_backward(store, i):
    from vod_amd.index import LogPartition, PosteriorExpectation

    t = _setup(store, i, _kind(i + 1))
    T = (64.0, 16.0)[i % 2]  # a spread posterior: a one-hot one has gradient zero, whatever the query
    rng = np.random.default_rng(i)
    scale = 10.0 ** rng.uniform(-6.0, 3.0, size=(t.nq, 1))  # the per-row power-of-two normalisation differs per query
    g = torch.from_numpy((rng.standard_normal((t.nq, N_COLS)) * scale).astype(np.float32)).cuda()

    def as_expectation(words):
        values, log_z, max_score, log_rel = (torch.as_tensor(a).cuda() for a in words)
        return PosteriorExpectation(values, LogPartition(log_z, max_score, log_rel))

    def backward(pe):
        def call():
            out = _poison((t.nq, t.c.d))
            assert t.ix.posterior_expectation_backward(t.qd, g, pe, temperature=T, out=out, **t.kw) is out
            return [out]

        return call

    t.ix.set_param("scan_temp_bytes", 0)
    pe0 = as_expectation(_expectation_call(t, T)())  # the unsliced forward
    assert t.ix.get_stat("last_scan_slice") == DEFAULT_SLICE
    # the sliced backward behind the unsliced forward
    want = _sliced(t.ix, backward(pe0), t.wanted, t.what)
    assert np.isfinite(want[0]).all() and len(np.unique(want[0], axis=0)) > t.nq // 2
    # the sliced backward behind the sliced forward
    pe1 = as_expectation(_sliced(t.ix, _expectation_call(t, T), t.wanted, t.what))
    got = _sliced(t.ix, backward(pe1), t.wanted, t.what)
    _same_bytes(got, want, t.what)

    # expected_values(q).backward(g): forward and backward both in slices of 64 under one budget
    def autograd():
        q = t.qd.clone().requires_grad_(True)
        y = t.ix.expected_values(q, T, t.kw.get("subset"))
        y.backward(g)
        return [y.detach(), q.grad.float()]

    t.ix.set_param("scan_temp_bytes", 0)
    full = autograd()
    assert t.ix.get_stat("last_scan_slice") == DEFAULT_SLICE
    t.ix.set_param("scan_temp_bytes", 1)
    try:
        cut = autograd()
        assert t.ix.get_stat("last_scan_slice") == 64
    finally:
        t.ix.set_param("scan_temp_bytes", 0)
    _same_bytes(cut, full, t.what)
    _same_bytes([full[0]], [pe0.values], t.what)
    _same_bytes([torch.from_numpy(want[0]).cuda().to(TDT[t.qdt]).float()], [full[1]], t.what)  # the gradient, cast to the queries' dtype


# ---- posterior_divergence / kl_to -----------------------------------------------------------------------------------------------------------
@each_case
def test_posterior_divergence_and_kl_to(store, i):
    t = _setup(store, i)
    qb = _dev(t.c.q2[: t.nq]).to(TDT[t.qdt])
    T_a = 1.0 / BETAS[i % 3]
    T_b = 2.0 * T_a if i % 2 else None  # (None: as a)

    def call():
        words = tuple(_poison((t.nq,)) for _ in range(8))
        r = t.ix.posterior_divergence(t.qd, qb, T_a, T_b, out=words, **t.kw)
        return [*words, r.kl_ab, r.kl_ba, r.cross_entropy_ab, r.cross_entropy_ba]

    got = _sliced(t.ix, call, t.wanted, t.what)  # (the slice counts pairs: 2 x slice staged queries per launch)
    assert len(got) == 12 and not np.array_equal(got[0], got[4])  # the two sides see different queries

    def kl():
        student = qb.clone().requires_grad_(True)
        out = t.ix.kl_to(t.qd, student, T_a, temperature_teacher=T_b, subset=t.kw.get("subset"))
        out.backward(torch.linspace(0.5, 2.0, t.nq, device="cuda"))
        return [out.detach(), student.grad.float()]

    t.ix.set_param("scan_temp_bytes", 0)
    full = kl()
    assert t.ix.get_stat("last_scan_slice") == DEFAULT_SLICE
    t.ix.set_param("scan_temp_bytes", 1)  # the divergence and both posterior means in slices of 64
    try:
        cut = kl()
        assert t.ix.get_stat("last_scan_slice") == 64
    finally:
        t.ix.set_param("scan_temp_bytes", 0)
    _same_bytes(cut, full, t.what)


# ---- rank_ids / count_above -------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.data_ptr())


def _native_call(t, name, *args):
    """the C entry point itself, on the current stream, so that the outputs are the test's own (poisoned) tensors"""
    from vod_amd import _native

    sub = t.kw.get("subset")
    head = (t.ix._h, _ptr(t.qd), _native.torch_dtype_code(t.qd.dtype), t.nq)
    labels = (_ptr(sub), 0 if sub is None else int(sub.shape[1]))
    fn = getattr(_native.load_library(), name)
    return head, labels, lambda *a: _native.check(fn(*a, _native.current_stream_ptr(t.ix.device)))


@each_case
def test_rank_ids(store, i):
    t = _setup(store, i)
    rng = np.random.default_rng(100 + i)
    ids = rng.integers(0, t.c.n, size=(t.nq, 5))  # five listed rows per query, different per query
    base = 0 if i % 2 == 0 else 2 ** 33
    lst = torch.from_numpy(ids + base).cuda()
    head, labels, run = _native_call(t, "vodhip_index_rank_ids")

    def call():
        rank, score = _poison((t.nq, 5), torch.int64), _poison((t.nq, 5))
        run(*head, _ptr(lst), 5, base, *labels, _ptr(rank), _ptr(score))
        return [rank, score]

    rank, score = _sliced(t.ix, call, t.wanted, t.what)
    _same_bytes(list(t.ix.rank_ids(t.qd, lst, id_base=base, **t.kw)), [rank, score], t.what)  # (the wrapper makes the same call)
    # exact integer scores: the rank is a count over the float64 score matrix
    s = t.c.s[: t.nq]
    mine = np.take_along_axis(s, ids, axis=1)
    elig = np.ones_like(s, dtype=bool) if t.elig is None else t.elig
    ahead = (s[:, None, :] > mine[:, :, None]) | ((s[:, None, :] == mine[:, :, None]) & (np.arange(t.c.n)[None, None, :] < ids[:, :, None]))
    want_rank = (ahead & elig[:, None, :]).sum(axis=2)
    present = np.take_along_axis(elig, ids, axis=1)
    np.testing.assert_array_equal(rank, np.where(present, want_rank, -1))
    np.testing.assert_array_equal(score, np.where(present, mine, -np.inf).astype(np.float32))


@each_case
def test_count_above(store, i):
    t = _setup(store, i)
    rng = np.random.default_rng(200 + i)
    s = t.c.s[: t.nq]
    thr = np.take_along_axis(s, rng.integers(0, t.c.n, size=(t.nq, 3)), axis=1).astype(np.float32)  # per-query thresholds [nq, 3]
    tie = rng.integers(0, t.c.n + 1, size=(t.nq, 3))
    thr_d, tie_d = torch.from_numpy(thr).cuda(), torch.from_numpy(tie).cuda()
    elig = np.ones_like(s, dtype=bool) if t.elig is None else t.elig
    above = s[:, None, :] > thr[:, :, None]
    tied = (s[:, None, :] == thr[:, :, None]) & (np.arange(t.c.n)[None, None, :] < tie[:, :, None])
    head, labels, run = _native_call(t, "vodhip_index_count_above")
    for name, ties, inn in (("strict", None, above), ("tie_ids", tie_d, above | tied)):

        def call():
            out = _poison((t.nq, 3), torch.int64)
            run(*head, _ptr(thr_d), _ptr(ties), 3, 0, *labels, _ptr(out))
            return [out]

        (cnt,) = _sliced(t.ix, call, t.wanted, f"{t.what} {name}")
        _same_bytes([t.ix.count_above(t.qd, thr_d, tie_ids=ties, **t.kw)], [cnt], name)
        np.testing.assert_array_equal(cnt, (inn & elig[:, None, :]).sum(axis=2), err_msg=name)


# ---- range_search, outranking, posterior_support ----------------------------------------------------------------------------------------------
def _range_thresholds(t):
    """list lengths from 0 to a few hundred, different per query"""
    s = t.c.s[: t.nq]
    desc = -np.sort(-s, axis=1)
    thr = desc[np.arange(t.nq), (np.arange(t.nq) * 37) % 300].astype(np.float32)
    thr[::9] = (desc[::9, 0] + 1.0).astype(np.float32)  # above every score: an empty list
    return thr


@each_case
def test_range_search(store, i):
    t = _setup(store, i)
    mode = ("tie_ids", "inclusive", "strict")[i % 3]
    order = "id" if i % 2 == 0 else "score"
    base = 10 ** 12 if i == 3 else 0
    rng = np.random.default_rng(300 + i)
    thr = _range_thresholds(t)
    tie = rng.integers(0, t.c.n + 1, size=t.nq) + base if mode == "tie_ids" else None
    thr_d = torch.from_numpy(thr).cuda()
    tie_d = None if tie is None else torch.from_numpy(tie).cuda()
    lib_tie = torch.full((t.nq,), G.TIE_PAST_EVERY_ROW, dtype=torch.int64, device="cuda") if mode == "inclusive" else tie_d
    # the exact integer scores
    want = G.range_search(t.c.s[: t.nq].astype(np.float32), thr, tie, eligible=t.elig, id_base=base, inclusive=mode == "inclusive")
    total = int(want[0][-1])
    lens = np.diff(want[0])
    assert lens.min() == 0 and lens.max() >= (100 if t.elig is None else 50) and len(set(lens.tolist())) > min(t.nq, 60) // 3
    head, labels, run = _native_call(t, "vodhip_index_range_search")

    def call():  # the sizing call (lims alone), then the call that emits
        sized, lims = _poison((t.nq + 1,), torch.int64), _poison((t.nq + 1,), torch.int64)
        scores, ids = _poison((total + 7,)), _poison((total + 7,), torch.int64)
        run(*head, _ptr(thr_d), _ptr(lib_tie), base, *labels, _ptr(sized), None, None, 0)
        run(*head, _ptr(thr_d), _ptr(lib_tie), base, *labels, _ptr(lims), _ptr(scores), _ptr(ids), total)
        assert t.ix.get_stat("last_range_selfcheck") == 0 and t.ix.get_stat("last_range_overflow") == 0
        return [sized, lims, scores, ids]

    sized, lims, scores, ids = _sliced(t.ix, call, t.wanted, t.what)
    _same_bytes([sized, lims, scores[:total], ids[:total]], [want[0], *want], t.what)
    assert (ids[total:] == POISON_INT).all() and np.isnan(scores[total:]).all()  # nothing past the result is written

    def wrapped():
        r = t.ix.range_search(t.qd, thr_d, tie_ids=tie_d, inclusive=mode == "inclusive", id_base=base, order=order, **t.kw)
        assert t.ix.get_stat("last_range_selfcheck") == 0 and t.ix.get_stat("last_range_overflow") == 0
        return list(r)

    if order == "score":
        want = (want[0], *G.sort_by_score(*want))
    _same_bytes(_sliced(t.ix, wrapped, t.wanted, t.what), list(want), t.what)

    # lims[nq] is the sum of count_above (itself sliced)
    def counts():
        return [t.ix.count_above(t.qd, thr_d[:, None], tie_ids=None if lib_tie is None else lib_tie[:, None], id_base=base, **t.kw)]

    (cnt,) = _sliced(t.ix, counts, t.wanted, t.what)
    assert lims[t.nq] == cnt.sum()
    np.testing.assert_array_equal(lens, cnt[:, 0])


@pytest.mark.parametrize("i", [0, 1, 2, 7], ids=[CASE_IDS[k] for k in (0, 1, 2, 7)])
def test_outranking_and_posterior_support(store, i):
    t = _setup(store, i)
    rng = np.random.default_rng(400 + i)
    tgt = torch.from_numpy(rng.integers(0, t.c.n, size=t.nq)).cuda()
    order = "score" if i % 2 == 0 else "id"
    # (rank_ids in front runs under the same budget with its own, larger, temporaries per query: the slice asserted is range_search's)
    lims, scores, ids = _sliced(t.ix, lambda: list(t.ix.outranking(t.qd, tgt, order=order, **t.kw)), t.wanted, t.what)
    assert t.ix.get_stat("last_range_selfcheck") == 0
    rank = t.ix.rank_ids(t.qd, tgt[:, None], **t.kw).rank[:, 0].cpu().numpy()
    np.testing.assert_array_equal(np.diff(lims), np.maximum(rank, 0))  # as many rows as the target's rank
    assert np.diff(lims).max() > 100

    def support():
        r = t.ix.posterior_support(t.qd, 1e-4, temperature=64.0, **t.kw)
        return [r.lims, r.scores, r.ids, r.log_p, *r.log_partition]

    got = _sliced(t.ix, support, t.wanted, t.what)
    assert t.ix.get_stat("last_range_selfcheck") == 0
    assert len(set(np.diff(got[0]).tolist())) > 10 and got[0][-1] > t.nq


# ---- sample_posterior ---------------------------------------------------------------------------------------------------------------------------
@each_case
def test_sample_posterior(store, i):
    t = _setup(store, i)
    k = 8 if i % 2 == 0 else 100
    offset = 0 if i % 4 < 2 else 7
    seed = 1234 + i
    sub = t.kw.get("subset")

    def draw(qd, off, sub):
        n = qd.shape[0]
        f32 = lambda *shape: _poison(shape)  # noqa: E731
        out = (f32(n), f32(n), _poison((n, k), torch.int64), f32(n, k), f32(n, k), f32(n, k), f32(n, k + 1))
        r = t.ix.sample_posterior(qd, k, temperature=64.0, seed=seed, query_offset=off, out=out, **({} if sub is None else {"subset": sub}))
        assert t.ix.get_stat("last_sample_selfcheck") == 0 and t.ix.get_stat("last_sample_overflow") == 0
        return [*out, r.log_tau, r.log_partition.log_z]  # (max_score, log_rel, ids, scores, log_p, log_weight, keys), the derived words

    got = _sliced(t.ix, lambda: draw(t.qd, offset, sub), t.wanted, t.what)
    ids, keys = got[2], got[6]
    assert (ids >= 0).all() and len(np.unique(ids, axis=0)) > t.nq // 2 and np.isfinite(keys).all()
    if sub is not None:
        assert np.take_along_axis(t.c.elig[: t.nq], ids, axis=1).all()
    # a draw does not depend on the batch: the same queries drawn alone, with their index in the stream
    for j in sorted({0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 383, 384, t.nq - 1}):
        if j < t.nq:
            alone = draw(t.qd[j : j + 1], offset + j, None if sub is None else sub[j : j + 1])
            _same_bytes(alone, [a[j : j + 1] for a in got], f"{t.what} query {j} alone")
    other = draw(t.qd[:1], offset + 1, None if sub is None else sub[:1])  # (and the stream index matters)
    assert not np.array_equal(_np(other[6]), keys[:1])


# ---- the node index ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wanted", [64, 128])
def test_node_index_forwards_the_budget_to_every_shard(wanted):
    from vod_amd.index import HipNodeIndex

    c = _case("small")
    q = np.array(c.q)
    thr = _range_thresholds(SimpleNamespace(c=c, nq=NQ))
    ids = np.random.default_rng(5).integers(0, c.n, size=(NQ, 5))
    with HipNodeIndex(c.d, c.n, [0, 0, 0]) as nx:  # 200 rows per shard
        nx.add(c.x)
        nx.set_row_labels(c.labels)
        nx.set_row_values(c.v)
        shards = range(3)

        def stats():
            r = nx.posterior_stats(q, temperature=64.0, subset=c.sub)
            return [r.entropy, r.mean_score, r.var_score, r.mean_rel, *r.log_partition]

        def ranged():
            return list(nx.range_search(q, thr, order="score"))

        def sample():
            r = nx.sample_posterior(q, 8, temperature=64.0, seed=77, query_offset=7)
            return [r.ids, r.scores, r.log_p, r.log_weight, r.keys, r.log_tau, *r.log_partition]

        def expectation():
            r = nx.posterior_expectation(q, temperature=64.0)
            return [r.values, *r.log_partition]

        def ranks():  # every shard picks its listed pairs' scan scores (the PICK mode of the rank scan), then counts
            return list(nx.rank_ids(q, ids))

        for name, call in (("posterior_stats", stats), ("range_search", ranged), ("sample_posterior", sample),
                           ("posterior_expectation", expectation), ("rank_ids", ranks)):
            nx.set_param("scan_temp_bytes", 0)
            want = call()
            assert [nx.shard_stat(g, "last_scan_slice") for g in shards] == [DEFAULT_SLICE] * 3, name
            per_query = {nx.shard_stat(g, "last_scan_per_query_bytes") for g in shards}
            assert len(per_query) == 1, name
            nx.set_param("scan_temp_bytes", _budget_for(per_query.pop(), wanted))
            got = call()
            assert [nx.shard_stat(g, "last_scan_slice") for g in shards] == [wanted] * 3, name
            _same_bytes(got, want, name)
        nx.set_param("scan_temp_bytes", 0)
        stats()
        assert [nx.shard_stat(g, "last_scan_slice") for g in shards] == [DEFAULT_SLICE] * 3
