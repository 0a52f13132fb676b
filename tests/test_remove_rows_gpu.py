"""`remove_rows` on the device (include/vodhip.h H2r): after every call every plane the store keeps equals, BYTE FOR BYTE over rows
[0, ntotal), an index freshly built by `add` from the surviving rows in order - the padded 16-bit plane (with an L2 store's bias
columns), an exact store's float32 plane and its two per-row statistics, the row labels, the value table with its zero pad rows.
`add` is the ingest path that was there before; which rows survive comes from the NumPy restatement (tests/remove_rows_ref.py).
No comparison has a tolerance: every one is `torch.equal` / `==` on integer views.

Sizes: ntotal = 1029 (no multiple of 4, 256 or the slab) with remove_slab_rows = 64 - 17 slabs, direct and bounced ones."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import remove_rows_ref as R
from vod_amd import _native
from vod_amd.index import HipFlatIndex, HipNodeIndex

pytestmark = pytest.mark.gpu

KINDS = ("plain", "l2", "exact")
DIMS = (1, 7, 8, 509, 513, 768, 1031)
COLS = (1, 64, 65, 256)
N = 1029
DEV = torch.device("cuda", 0)
PLANE_LABELS, PLANE_VALUES, PLANE_ROW_N2, PLANE_ROW_D2, PLANE_OWNER = range(5)


def make_index(kind: str, dim: int, capacity: int, dtype=torch.float16, slab: int | None = 64) -> HipFlatIndex:
    ix = HipFlatIndex(dim, capacity, dtype=dtype, device=0, exact_f32=kind == "exact", metric="l2" if kind == "l2" else "inner_product")
    if slab is not None:
        ix.set_param("remove_slab_rows", slab)
    return ix


class _DeviceWords:
    """`[rows, cols]` words of a store's plane as an object torch can wrap (`__cuda_array_interface__`)."""

    def __init__(self, ptr: int, rows: int, cols: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (rows, cols), "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}


def _view(ptr, rows: int, cols: int, typestr: str) -> torch.Tensor:
    dtype = torch.int16 if typestr == "<i2" else torch.int32
    if not ptr or rows == 0 or cols == 0:
        return torch.empty((0, cols), dtype=dtype, device=DEV)
    return torch.as_tensor(_DeviceWords(ptr, rows, cols, typestr), device=DEV).clone()


def raw_planes(handle) -> dict[str, torch.Tensor]:
    """every plane of the flat index behind `handle`, rows [0, ntotal) (the value table: all its padded rows), as integer words"""
    lib = _native.load_library()
    h = ctypes.c_void_p(handle) if isinstance(handle, int) else handle
    nt, ptr, stride, dt = ctypes.c_int64(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int32()
    _native.check(lib.vodhip_index_ntotal(h, ctypes.byref(nt)))
    torch.cuda.synchronize()
    _native.check(lib.vodhip_index_data(h, ctypes.byref(ptr), ctypes.byref(stride), ctypes.byref(dt)))
    out = {"plane": _view(ptr.value, nt.value, stride.value, "<i2")}
    exact = ctypes.c_int64()
    _native.check(lib.vodhip_index_get_stat(h, b"exact", ctypes.byref(exact)))
    if exact.value:
        _native.check(lib.vodhip_index_data_f32(h, ctypes.byref(ptr), ctypes.byref(stride)))
        out["f32"] = _view(ptr.value, nt.value, stride.value, "<i4")
    rows = ctypes.c_int64()
    for name, which, typestr in (("labels", PLANE_LABELS, "<i4"), ("values", PLANE_VALUES, "<i2"), ("n2", PLANE_ROW_N2, "<i4"), ("d2", PLANE_ROW_D2, "<i4")):
        _native.check(lib.vodhip_index_plane(h, which, ctypes.byref(ptr), ctypes.byref(rows), ctypes.byref(stride)))
        if ptr.value and rows.value:  # (an index built from no rows has no labels: a plane of no rows is no plane here)
            out[name] = _view(ptr.value, rows.value, stride.value, typestr)
    _native.check(lib.vodhip_index_plane(h, PLANE_OWNER, ctypes.byref(ptr), ctypes.byref(rows), ctypes.byref(stride)))
    out["owner"] = _view(ptr.value, rows.value, 1, "<i4")
    return out


def assert_same_planes(a: dict, b: dict, what: str = "") -> None:
    assert not a["owner"].any(), f"{what}: the owner table is not all zero"
    names = (set(a) | set(b)) - {"owner"}
    for name in sorted(names):
        assert name in a and name in b, f"{what}: plane '{name}' is kept by one index only"
        assert a[name].shape == b[name].shape, f"{what}: plane '{name}' {tuple(a[name].shape)} != {tuple(b[name].shape)}"
        assert torch.equal(a[name], b[name]), f"{what}: plane '{name}' differs in {int((a[name] != b[name]).sum())} words"


class Corpus:
    """host rows, labels and a value table, and the indexes built from them"""

    def __init__(self, rng, n: int, dim: int, cols: int | None):
        self.rows = rng.standard_normal((n, dim)).astype(np.float32)
        self.labels = rng.integers(0, 5, n).astype(np.int32)
        self.values = None if cols is None else rng.standard_normal((n, cols)).astype(np.float32)

    def build(self, kind: str, dtype, capacity: int, keep=None, slab: int | None = 64, labels: bool = True) -> HipFlatIndex:
        """every kind takes the table (only a plain store can read it out: the gather and the bounce layout do not care)"""
        keep = slice(None) if keep is None else keep
        rows = self.rows[keep]
        ix = make_index(kind, self.rows.shape[1], capacity, dtype, slab)
        if rows.shape[0]:
            ix.add(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV))
            if labels:
                ix.set_row_labels(self.labels[keep])
        if self.values is not None:
            ix.set_row_values(np.ascontiguousarray(self.values[keep]))
        return ix


def check_removal(ix: HipFlatIndex, corpus: Corpus, kind: str, keep_before: np.ndarray, what: str, *, ids=None, begin=0, n=None, mask=None, device_ids=False,
                  labels: bool = True):
    """one call on `ix` (which holds corpus[keep_before]), checked against the restatement and a fresh index; returns the new keep mask"""
    old = ix.ntotal
    if mask is not None:
        keep, counts = R.resolve_removal(old, ids=np.flatnonzero(mask))
    else:
        keep, counts = R.resolve_removal(old, ids=ids, begin=begin, n=n)
    given = ids
    if ids is not None and device_ids:
        given = torch.as_tensor(np.asarray(ids, dtype=np.int64)).to(DEV)
    removed, new_ids = ix.remove_rows(ids=given, begin=begin, n=n, mask=mask, return_map=True)
    got = (ix.get_stat("last_remove_removed"), ix.get_stat("last_remove_skipped"), ix.get_stat("last_remove_duplicates"))
    assert got == tuple(counts) and removed == counts[0], f"{what}: stats {got}, returned {removed} != {tuple(counts)}"
    assert ix.ntotal == old - counts[0] and ix.capacity >= old
    assert new_ids.dtype == torch.int64 and np.array_equal(new_ids.cpu().numpy(), R.new_ids(keep)), f"{what}: new_ids"
    now = np.flatnonzero(keep_before)[keep]
    with corpus.build(kind, ix.dtype, max(1, ix.capacity), keep=now, labels=labels) as fr:
        mine, fresh = raw_planes(ix._h), raw_planes(fr._h)
        assert ("labels" in fresh) == (labels and now.size > 0) and ("values" in fresh) == (corpus.values is not None)
        assert_same_planes(mine, fresh, what)
        if corpus.values is not None:
            assert ix.row_values_shape == (ix.ntotal, corpus.values.shape[1]) == fr.row_values_shape
    out = np.zeros(keep_before.size, dtype=bool)
    out[now] = True
    return out


def assert_same_bits(a, b, what: str) -> None:
    """two results (named tuples of tensors and plain values) hold the same bits"""
    def walk(x, y) -> int:
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape, what
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), what
            return 1
        if isinstance(x, tuple):  # (a result may hold another one: the read-out carries its log partition)
            assert len(x) == len(y), what
            return sum(walk(p, q) for p, q in zip(x, y))
        assert x == y, what
        return 0

    assert walk(tuple(a), tuple(b)) > 0, what


def _dtype_for(i: int):
    return torch.float16 if i % 2 == 0 else torch.bfloat16


# ---- planes, byte for byte --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_every_plane_equals_a_fresh_index_across_dims(dim, kind):
    rng = np.random.default_rng(2000 + dim)
    cols = COLS[DIMS.index(dim) % len(COLS)]
    corpus = Corpus(rng, N, dim, cols)
    dtype = _dtype_for(DIMS.index(dim) + KINDS.index(kind))
    all_rows = np.ones(N, dtype=bool)
    cases = [
        ("a random 25 %", dict(ids=rng.permutation(N)[: N // 4])),
        ("row 0 only", dict(ids=[0])),
        ("the last row only", dict(ids=[N - 1])),
        ("a contiguous middle range by the range form", dict(begin=300, n=333)),
        ("every other row", dict(mask=np.arange(N) % 2 == 0)),
    ]
    for what, kw in cases:
        with corpus.build(kind, dtype, N + 8) as ix:
            check_removal(ix, corpus, kind, all_rows, f"{kind} dim {dim}: {what}", **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cols", COLS)
def test_all_none_and_bad_lists_with_every_table_width(cols, kind):
    rng = np.random.default_rng(31 + cols)
    dim = 72
    corpus = Corpus(rng, N, dim, cols)
    dtype = _dtype_for(COLS.index(cols) + KINDS.index(kind))
    all_rows = np.ones(N, dtype=bool)
    with corpus.build(kind, dtype, N) as ix:
        before = raw_planes(ix._h)
        # nothing leaves: an empty list, an empty range, a list that skips every slot
        check_removal(ix, corpus, kind, all_rows, "an empty list", ids=np.zeros(0, dtype=np.int64))
        check_removal(ix, corpus, kind, all_rows, "an empty range at the end", begin=N, n=0)
        check_removal(ix, corpus, kind, all_rows, "every slot skipped", ids=[-1, N, -5, 2**40, N + 7])
        assert_same_planes(raw_planes(ix._h), before, "a no-op wrote something")
        # negative, out-of-range and repeated ids, from the host and from the device
        bad = np.concatenate([rng.permutation(N)[:200], [-1, N, 5, 5, 5, 2**33, -(2**40), N - 1, N - 1, 0, 0]])
        rng.shuffle(bad)
        keep = check_removal(ix, corpus, kind, all_rows, "a list with pads and repeats, host", ids=bad)
        with corpus.build(kind, dtype, N) as ix2:
            check_removal(ix2, corpus, kind, all_rows, "the same list, device", ids=bad, device_ids=True)
            assert_same_planes(raw_planes(ix._h), raw_planes(ix2._h), "host list vs device list")
        # then every row that is left
        keep = check_removal(ix, corpus, kind, keep, "all rows", begin=0, n=ix.ntotal)
        assert ix.ntotal == 0 and not keep.any()
        lib, ptr, rows, stride = _native.load_library(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        _native.check(lib.vodhip_index_plane(ix._h, PLANE_LABELS, ctypes.byref(ptr), ctypes.byref(rows), ctypes.byref(stride)))
        assert ptr.value, "the labels are still attached"
        assert ix.row_values_shape == (0, cols)
        # and the emptied store takes rows again
        ix.add(torch.from_numpy(corpus.rows[:5]).to(DEV))
        with make_index(kind, dim, N, dtype) as fr:
            fr.add(torch.from_numpy(corpus.rows[:5]).to(DEV))
            assert torch.equal(raw_planes(ix._h)["plane"], raw_planes(fr._h)["plane"])


def test_all_rows_by_a_list_and_a_single_row_store():
    rng = np.random.default_rng(5)
    for n in (1, 5, N):
        corpus = Corpus(rng, n, 65, 65)
        with corpus.build("plain", torch.float16, n) as ix:
            check_removal(ix, corpus, "plain", np.ones(n, dtype=bool), f"all {n} rows by a shuffled list", ids=rng.permutation(n))
        with corpus.build("exact", torch.bfloat16, n + 3) as ix:
            check_removal(ix, corpus, "exact", np.ones(n, dtype=bool), f"row 0 of {n}", ids=[0])


def test_value_table_pad_rows_are_zero_after_a_removal():
    rng = np.random.default_rng(6)
    corpus = Corpus(rng, N, 40, 65)
    with corpus.build("plain", torch.float16, N) as ix:
        ix.remove_rows(ids=rng.permutation(N)[:300])  # 729 rows stay: rows [729, 768) of the table are pad rows that held values
        table = raw_planes(ix._h)["values"]
        assert ix.ntotal == 729 and table.shape == (768, 128)
        assert table[:729, :65].any() and not table[729:].any() and not table[:, 65:].any()
        ix.remove_rows(begin=100, n=629)  # 100 rows stay
        table = raw_planes(ix._h)["values"]
        assert table.shape == (256, 128) and not table[100:].any()


# ---- no result depends on the stale rows behind ntotal ----------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["tail", "head"])
def test_stale_rows_behind_ntotal_change_no_result(where):
    rng = np.random.default_rng(8)
    dim, cols = 64, 64
    corpus = Corpus(rng, N, dim, cols)
    poison = np.zeros((40, dim), dtype=np.float32)
    poison[0::4], poison[1::4], poison[2::4], poison[3::4] = np.inf, -np.inf, np.nan, 65504.0
    at = slice(N - 40, N) if where == "tail" else slice(0, 40)
    corpus.rows[at] = poison
    corpus.values[at] = 65504.0
    keep = np.ones(N, dtype=bool)
    keep[at] = False
    q = torch.from_numpy(rng.standard_normal((33, dim)).astype(np.float32)).to(DEV).half()
    with corpus.build("plain", torch.float16, N) as ix, corpus.build("plain", torch.float16, N, keep=np.flatnonzero(keep)) as fr:
        # tail: nothing moves, the poisoned rows stay behind ntotal; head: every row moves down by 40, the tail holds stale finite copies
        assert ix.remove_rows(begin=at.start, n=40) == 40
        assert_same_planes(raw_planes(ix._h), raw_planes(fr._h), where)
        for k in (1, 10, 100):
            (s, i), (fs, fi) = ix.search(q, k), fr.search(q, k)
            assert torch.equal(s.view(torch.int32), fs.view(torch.int32)) and torch.equal(i, fi)
        assert_same_bits(ix.log_partition(q, temperature=0.5), fr.log_partition(q, temperature=0.5), "log_partition")
        assert_same_bits(ix.posterior_expectation(q, temperature=0.5), fr.posterior_expectation(q, temperature=0.5), "posterior_expectation")


# ---- every combination of planes: a store without labels, with and without a table ------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cols", [None, 65])
def test_stores_without_labels_with_and_without_a_table(cols, kind):
    rng = np.random.default_rng(21)
    corpus = Corpus(rng, N, 136, cols)
    all_rows = np.ones(N, dtype=bool)
    with corpus.build(kind, torch.bfloat16, N, labels=False) as ix:
        assert "labels" not in raw_planes(ix._h) and ("values" in raw_planes(ix._h)) == (cols is not None)
        keep = check_removal(ix, corpus, kind, all_rows, "no labels: a random 25 %", ids=rng.permutation(N)[: N // 4], labels=False)
        keep = check_removal(ix, corpus, kind, keep, "no labels: row 0", ids=[0], labels=False)
        check_removal(ix, corpus, kind, keep, "no labels: a middle range", begin=100, n=300, labels=False)


# ---- a table that rows were added behind is refused, not moved -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_value_table_left_short_by_add_is_refused_and_stays_stale(kind):
    rng = np.random.default_rng(22)
    corpus = Corpus(rng, N, 72, 65)
    with make_index(kind, 72, N) as ix:
        ix.add(torch.from_numpy(corpus.rows[:100]).to(DEV))
        ix.set_row_values(corpus.values[:100])  # allocated for 256 rows
        ix.add(torch.from_numpy(corpus.rows[100:]).to(DEV))  # legal: the table stays, short, and every read-out refuses it
        assert ix.row_values_shape == (100, 65) and ix.ntotal == N
        before = raw_planes(ix._h)
        for kw in (dict(ids=[0, 500, N - 1]), dict(begin=50, n=700), dict(mask=np.arange(N) % 2 == 0), dict(ids=[])):
            with pytest.raises(_native.NativeLibraryError, match="value table holds 100 rows"):
                ix.remove_rows(**kw)
        assert ix.ntotal == N and ix.row_values_shape == (100, 65)  # still short: not passed off as valid
        assert_same_planes(raw_planes(ix._h), before, "a refused call wrote something")
        if kind == "plain":
            q = torch.from_numpy(rng.standard_normal((4, 72)).astype(np.float32)).to(DEV).half()
            with pytest.raises(_native.NativeLibraryError, match="set the table again"):
                ix.posterior_expectation(q)
        # set again: the removal goes through; cleared: too
        ix.set_row_values(corpus.values)
        keep = check_removal(ix, corpus, kind, np.ones(N, dtype=bool), "after the table was set again", ids=[0, 500, N - 1], labels=False)
        ix.set_row_values(None)
        corpus.values = None
        check_removal(ix, corpus, kind, keep, "after the table was cleared", begin=10, n=20, labels=False)


def test_node_index_refuses_a_value_table_left_short_by_add():
    rng = np.random.default_rng(23)
    corpus = Corpus(rng, 700, 64, 65)
    with _node(corpus, "plain", 2, keep=np.arange(300)) as nx:
        nx.add(corpus.rows[300:])
        before = [raw_planes(nx.shard(g)[0]) for g in range(2)]
        for kw in (dict(ids=[5]), dict(begin=350, n=100)):  # (the second range lies in a shard whose own table is not short)
            with pytest.raises(_native.NativeLibraryError, match="value table holds 300 rows"):
                nx.remove_rows(**kw)
        assert nx.ntotal == 700 and nx.row_values_shape == (300, 65)
        for g in range(2):
            assert_same_planes(raw_planes(nx.shard(g)[0]), before[g], f"a refused call wrote to shard {g}")


# ---- the slab size changes nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_slab_sizes_give_identical_bytes(kind):
    rng = np.random.default_rng(9)
    corpus = Corpus(rng, N, 200, 65)
    ids = rng.permutation(N)[:400]
    got = []
    for slab in (4, 64, None):
        with corpus.build(kind, torch.float16, N, slab=slab) as ix:
            assert ix.get_stat("remove_slab_rows") == (slab or 65536)
            assert ix.remove_rows(ids=ids) == 400
            got.append(raw_planes(ix._h))
    assert_same_planes(got[0], got[1], "slab 4 vs 64")
    assert_same_planes(got[0], got[2], "slab 4 vs the default")
    with make_index(kind, 8, 16) as ix:
        for bad in (1, 3, 6, 96, -4, 2**31):
            with pytest.raises(_native.NativeLibraryError):
                ix.set_param("remove_slab_rows", bad)


# ---- the exact store's bound is re-derived ------------------------------------------------------------------------------------------
def test_exact_store_rederives_its_maxima_after_the_extreme_rows_left():
    rng = np.random.default_rng(10)
    dim = 96
    corpus = Corpus(rng, N, dim, None)
    # the largest norm, with no rounding error at all (8192 is an fp16 value); the largest rounding error, with a smaller norm
    # (2000 * (1 + 2^-12) = 2000.488..: fp16 values are 1 apart there, every column is off by 0.488)
    corpus.rows[517] = 8192.0 * np.sign(corpus.rows[517])
    corpus.rows[33] = np.float32(2000.0 * (1.0 + 2.0 ** -12)) * np.sign(corpus.rows[33])
    q = torch.from_numpy(rng.standard_normal((17, dim)).astype(np.float32)).to(DEV)
    keep = np.ones(N, dtype=bool)
    keep[[33, 517]] = False
    with corpus.build("exact", torch.float16, N) as ix, corpus.build("exact", torch.float16, N, keep=np.flatnonzero(keep)) as fr:
        n2, d2 = raw_planes(ix._h)["n2"].view(torch.float32), raw_planes(ix._h)["d2"].view(torch.float32)
        assert int(n2.argmax()) == 517 and int(d2.argmax()) == 33
        assert ix.remove_rows(ids=[517, 33]) == 2
        assert_same_planes(raw_planes(ix._h), raw_planes(fr._h), "exact")
        (s, i), (fs, fi) = ix.search(q, 10), fr.search(q, 10)
        assert torch.equal(s.view(torch.int32), fs.view(torch.int32)) and torch.equal(i, fi)
        for key in ("last_exact_kx", "last_exact_band_passes", "last_exact_band_queries", "exact_outliers"):
            assert ix.get_stat(key) == fr.get_stat(key), key


# ---- life after a removal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_add_update_and_a_second_removal_work_afterwards(kind):
    rng = np.random.default_rng(11)
    dim = 130
    corpus = Corpus(rng, N + 100, dim, None)
    first = np.zeros(N + 100, dtype=bool)
    first[:N] = True
    with make_index(kind, dim, N + 100) as ix:
        ix.add(torch.from_numpy(corpus.rows[:N]).to(DEV))
        ix.set_row_labels(corpus.labels[:N])
        keep = check_removal(ix, corpus, kind, first, "first removal", ids=rng.permutation(N)[:257])
        # add of 100 more rows (labels are set again for all rows, as after any add)
        ix.add(torch.from_numpy(corpus.rows[N:]).to(DEV))
        keep[N:] = True
        now = np.flatnonzero(keep)
        ix.set_row_labels(corpus.labels[now])
        with corpus.build(kind, torch.float16, N + 100, keep=now) as fr:
            assert_same_planes(raw_planes(ix._h), raw_planes(fr._h), "add after a removal")
        # a listed update_rows
        upd = rng.permutation(now.size)[:50]
        new_rows = rng.standard_normal((50, dim)).astype(np.float32)
        ix.update_rows(torch.from_numpy(new_rows).to(DEV), ids=upd)
        assert ix.get_stat("last_update_written") == 50
        corpus.rows[now[upd]] = new_rows
        with corpus.build(kind, torch.float16, N + 100, keep=now) as fr:
            assert_same_planes(raw_planes(ix._h), raw_planes(fr._h), "update_rows after a removal")
        # a second removal
        check_removal(ix, corpus, kind, keep, "second removal", mask=rng.random(now.size) < 0.5)


def test_removal_is_refused_while_a_search_is_pending():
    rng = np.random.default_rng(12)
    corpus = Corpus(rng, N, 64, 64)
    q = torch.from_numpy(rng.standard_normal((8, 64)).astype(np.float32)).to(DEV).half()
    with corpus.build("plain", torch.float16, N) as ix:
        before = raw_planes(ix._h)
        ix.search_async(q, 5)
        with pytest.raises(_native.NativeLibraryError, match="in flight"):
            ix.remove_rows(ids=[1, 2, 3])
        ix.finish()
        assert ix.ntotal == N
        assert_same_planes(raw_planes(ix._h), before, "a refused call wrote something")
        for kw in (dict(begin=N - 1, n=2), dict(begin=N + 1, n=0)):
            with pytest.raises(ValueError):
                ix.remove_rows(**kw)
        lib = _native.load_library()
        for args in ((None, N - 1, 2, 0), (None, -1, 1, 0), (None, 0, -1, 0), (None, 0, 1, 7)):  # the C call's own refusals
            assert lib.vodhip_index_remove_rows(ix._h, args[0], args[1], args[2], args[3], 0, None, None, None) == -1
        assert_same_planes(raw_planes(ix._h), before, "a refused call wrote something")
        assert ix.remove_rows(ids=[1, 2, 3]) == 3


# ---- the node index -------------------------------------------------------------------------------------------------------------------
def _node(corpus: Corpus, kind: str, n_shards: int, keep=None, slab: int = 64) -> HipNodeIndex:
    keep = slice(None) if keep is None else keep
    nx = HipNodeIndex(corpus.rows.shape[1], 400 * n_shards, devices=[0] * n_shards, dtype=torch.float16, exact_f32=kind == "exact")
    nx.set_param("remove_slab_rows", slab)
    rows = np.ascontiguousarray(corpus.rows[keep])
    if rows.shape[0]:
        nx.add(rows)
        nx.set_row_labels(np.ascontiguousarray(corpus.labels[keep]))
        nx.set_row_values(np.ascontiguousarray(corpus.values[keep]))
    return nx


@pytest.mark.parametrize("kind", ["plain", "exact"])
@pytest.mark.parametrize("n_shards", [2, 3])
def test_node_index_ends_byte_equal_to_one_built_from_the_survivors(n_shards, kind):
    rng = np.random.default_rng(13 + n_shards)
    dim = 72
    n = 400 * n_shards - 37  # the last shard is not full
    corpus = Corpus(rng, n, dim, 65)
    q = rng.standard_normal((9, dim)).astype(np.float32)
    cases = [
        ("a range across the first shard boundary", dict(begin=390, n=20)),
        ("the middle (or last) shard empties", dict(begin=400, n=min(400, n - 400))),
        ("a list with pads and repeats over all shards", dict(ids=np.concatenate([rng.permutation(n)[:300], [-1, n, 399, 399, 400, 400, 2**40]]))),
        ("row 0 only: every shard shifts by one", dict(ids=[0])),
        ("nothing", dict(ids=[-1, n])),
        ("all rows", dict(mask=np.ones(n, dtype=bool))),
    ]
    for what, kw in cases:
        if "mask" in kw:
            keep, counts = R.resolve_removal(n, ids=np.flatnonzero(kw["mask"]))
        else:
            keep, counts = R.resolve_removal(n, ids=kw.get("ids"), begin=kw.get("begin", 0), n=kw.get("n"))
        now = np.flatnonzero(keep)
        with _node(corpus, kind, n_shards) as nx, _node(corpus, kind, n_shards, keep=now) as fr:
            removed, new_ids = nx.remove_rows(return_map=True, **kw)
            got = (nx.get_stat("last_remove_removed"), nx.get_stat("last_remove_skipped"), nx.get_stat("last_remove_duplicates"))
            assert got == tuple(counts) and removed == counts[0], f"{what}: {got} != {counts}"
            assert nx.ntotal == now.size == fr.ntotal
            assert np.array_equal(new_ids, R.new_ids(keep)), what
            for g in range(n_shards):
                a, b = raw_planes(nx.shard(g)[0]), raw_planes(fr.shard(g)[0])
                if now.size == 0:  # (a node index built from no rows has no labels and no table to compare with)
                    assert a["plane"].shape[0] == 0
                    continue
                assert_same_planes(a, b, f"{what}: shard {g}")
            if now.size == 0:
                continue
            (s, i), (fs, fi) = nx.search(q, 10), fr.search(q, 10)
            assert np.array_equal(s.view(np.int32), fs.view(np.int32)) and np.array_equal(i, fi), what
            assert nx.row_values_shape == (now.size, 65) == fr.row_values_shape
            if kind == "plain":
                ids = rng.integers(0, now.size, (4, 6))
                w = rng.standard_normal((4, 6)).astype(np.float32)
                assert np.array_equal(np.asarray(nx.sum_ids(ids, w)).view(np.int32), np.asarray(fr.sum_ids(ids, w)).view(np.int32)), what


def test_node_index_refuses_a_bad_range_and_a_pending_search():
    rng = np.random.default_rng(14)
    corpus = Corpus(rng, 700, 64, 65)
    with _node(corpus, "plain", 2) as nx:
        with pytest.raises(ValueError):
            nx.remove_rows(begin=699, n=2)
        lib = _native.load_library()
        assert lib.vodhip_node_index_remove_rows(nx._h, None, 699, 2, None, None) == -1
        assert lib.vodhip_node_index_remove_rows(nx._h, None, 0, -1, None, None) == -1
        nx.search_async(rng.standard_normal((3, 64)).astype(np.float32), 5)
        with pytest.raises(_native.NativeLibraryError, match="in flight"):
            nx.remove_rows(ids=[1])
        nx.finish()
        assert nx.ntotal == 700 and nx.remove_rows(ids=[1]) == 1 and nx.ntotal == 699
