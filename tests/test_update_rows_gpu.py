"""`update_rows` / `add_to_rows` on the device (include/vodhip.h H2u): after every call the store equals, BYTE FOR BYTE, an index freshly
built by `add` from the final rows.  `add` is the ingest path that was there before; the final rows come from the NumPy restatement
(tests/update_rows_ref.py).  No comparison has a tolerance: every one is `torch.equal` on integer views of the planes."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import update_rows_ref as R
from vod_amd import _native
from vod_amd.index import HipFlatIndex, HipNodeIndex

pytestmark = pytest.mark.gpu

KINDS = ("plain", "l2", "exact")
DIMS = (1, 7, 8, 64, 65, 509, 510, 512, 513, 768, 1031)
DEV = torch.device("cuda", 0)


def make_index(kind: str, dim: int, capacity: int, dtype=torch.float16) -> HipFlatIndex:
    return HipFlatIndex(dim, capacity, dtype=dtype, device=0, exact_f32=kind == "exact", metric="l2" if kind == "l2" else "inner_product")


class _DevicePlane:
    """The padded 16-bit plane of a store, `[ntotal, dim_pad]`, as an object torch can wrap (`__cuda_array_interface__`)."""

    def __init__(self, ptr: int, rows: int, cols: int):
        self.__cuda_array_interface__ = {"shape": (rows, cols), "typestr": "<i2", "data": (ptr, False), "version": 2, "strides": None}


def padded_plane(handle, ntotal: int) -> torch.Tensor:
    lib = _native.load_library()
    ptr, stride, dt = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int32()
    _native.check(lib.vodhip_index_data(handle, ctypes.byref(ptr), ctypes.byref(stride), ctypes.byref(dt)))
    if ntotal == 0:
        return torch.empty((0, stride.value), dtype=torch.int16, device=DEV)
    torch.cuda.synchronize()
    return torch.as_tensor(_DevicePlane(ptr.value, ntotal, stride.value), device=DEV).clone()


def planes(ix: HipFlatIndex) -> dict[str, torch.Tensor]:
    out = {"rows": ix.stored_rows().view(torch.int16), "plane": padded_plane(ix._h, ix.ntotal)}
    if ix.exact_f32:
        out["f32"] = ix.stored_rows_f32().view(torch.int32)
    return out


def master(ix: HipFlatIndex) -> np.ndarray:
    """the float32 matrix an ADD adds to: the float32 plane of an exact store, the 16-bit rows widened anywhere else"""
    return (ix.stored_rows_f32() if ix.exact_f32 else ix.stored_rows().float()).cpu().numpy()


def fresh_like(ix: HipFlatIndex, kind: str, matrix: np.ndarray) -> HipFlatIndex:
    fr = make_index(kind, ix.dim, max(1, ix.capacity), ix.dtype)
    if matrix.shape[0]:
        fr.add(torch.from_numpy(np.ascontiguousarray(matrix, dtype=np.float32)).to(DEV))
    return fr


def assert_same_store(ix: HipFlatIndex, fr: HipFlatIndex, what: str = "") -> None:
    a, b = planes(ix), planes(fr)
    assert ix.ntotal == fr.ntotal
    for name in a:
        assert torch.equal(a[name], b[name]), f"{what}: plane '{name}' differs in {int((a[name] != b[name]).sum())} words"
    if ix.metric == "l2":
        assert ix.get_stat("l2_saturated_rows") >= fr.get_stat("l2_saturated_rows")


def source(rng, n: int, dim: int, dtype: torch.dtype, where: str, misaligned: bool = False):
    """`[n, dim]` N(0, 1) rows of `dtype`, on the host (NumPy; bf16 as a CPU tensor) or the device; `misaligned`: a device view that
    starts one element into its buffer.  Returns (what the index is handed, the same values as float32 NumPy)."""
    v = torch.from_numpy(rng.standard_normal((n, dim)).astype(np.float32)).to(dtype)
    f32 = v.float().numpy()
    if where == "host":
        return (v if dtype == torch.bfloat16 else v.numpy()), f32
    if misaligned:
        buf = torch.empty(n * dim + 1, dtype=dtype, device=DEV)
        buf[1:] = v.reshape(-1).to(DEV)
        view = buf[1:].view(n, dim)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        return view, f32
    return v.to(DEV), f32


def do_update(ix: HipFlatIndex, kind: str, src, src_f32, *, ids=None, begin=0, mode="set", alpha=1.0, check=True, what=""):
    """one call on `ix`, checked against a fresh index built from the restatement's matrix; returns the counts"""
    want, counts = R.apply_update(master(ix), src_f32, ids=ids, begin=begin, mode=mode, alpha=alpha)
    if mode == "set":
        ix.update_rows(src, ids=ids, begin=begin)
    else:
        ix.add_to_rows(src, alpha=alpha, ids=ids, begin=begin, check=check)
    got = (ix.get_stat("last_update_written"), ix.get_stat("last_update_skipped"), ix.get_stat("last_update_duplicates"))
    assert got == tuple(counts), f"{what}: stats {got} != {tuple(counts)}"
    with fresh_like(ix, kind, want) as fr:
        assert_same_store(ix, fr, what)
    return counts


# ---- planes, byte for byte --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", DIMS)
def test_every_plane_equals_a_fresh_index_across_dims(dim, kind):
    rng = np.random.default_rng(1000 + dim)
    n = 1029
    dtype = torch.float16 if (DIMS.index(dim) + KINDS.index(kind)) % 2 == 0 else torch.bfloat16
    with make_index(kind, dim, n + 8, dtype) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        ids = rng.permutation(n)[:257]
        do_update(ix, kind, *source(rng, 257, dim, torch.float32, "device"), ids=ids, what="listed SET 257 f32 device")
        do_update(ix, kind, *source(rng, 5, dim, torch.float16, "host"), ids=rng.permutation(n)[:5], mode="add", alpha=-0.125, what="listed ADD 5 f16 host")
        do_update(ix, kind, *source(rng, 4, dim, torch.bfloat16, "device"), begin=3, what="dense SET 4 bf16 device")
        do_update(ix, kind, *source(rng, n - 2, dim, torch.float32, "host"), begin=2, mode="add", alpha=3e-4, what="dense ADD f32 host")
        do_update(ix, kind, *source(rng, 3, dim, torch.float32, "device", misaligned=True), ids=[n - 1, 0, 512], mode="add", alpha=1.0,
                  what="listed ADD 3 misaligned f32")
        do_update(ix, kind, *source(rng, 1, dim, torch.float16, "device", misaligned=True), ids=[n - 1], what="listed SET 1 misaligned f16")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_every_source_dtype_mode_and_location(dtype, kind):
    rng = np.random.default_rng(7)
    n, dim = 1029, 72
    with make_index(kind, dim, n, dtype) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        for src_dtype in (torch.float16, torch.bfloat16, torch.float32):
            for where in ("host", "device"):
                for mode, alpha in (("set", 1.0), ("add", 1.0), ("add", -0.125), ("add", 3e-4)):
                    what = f"{src_dtype} {where} {mode} {alpha}"
                    do_update(ix, kind, *source(rng, 4, dim, src_dtype, where), ids=rng.permutation(n)[:4], mode=mode, alpha=alpha, what="listed " + what)
                    do_update(ix, kind, *source(rng, 5, dim, src_dtype, where), begin=n - 5, mode=mode, alpha=alpha, what="dense " + what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 5])
def test_small_stores_and_lists_at_the_workgroup_edge(n, kind):
    rng = np.random.default_rng(n)
    dim = 65
    with make_index(kind, dim, n) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        for slots in (1, 3, 4, 5):
            ids = rng.integers(0, n, size=slots)  # (repeats: the last slot of a row wins)
            do_update(ix, kind, *source(rng, slots, dim, torch.float32, "device"), ids=ids, what=f"listed SET {slots}")
            do_update(ix, kind, *source(rng, slots, dim, torch.float32, "host"), ids=ids, mode="add", alpha=-0.125, check=False, what=f"listed ADD {slots}")
        do_update(ix, kind, *source(rng, n, dim, torch.float16, "device"), what="dense SET all")
        do_update(ix, kind, *source(rng, 1, dim, torch.float16, "host"), begin=n - 1, mode="add", what="dense ADD last")
        do_update(ix, kind, *source(rng, 0, dim, torch.float32, "device"), ids=[], what="empty list")
        do_update(ix, kind, *source(rng, 0, dim, torch.float32, "host"), begin=n, what="empty range at the end")


# ---- duplicates and skips ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["host", "device"])
def test_duplicates_pads_and_out_of_range_ids(where, kind):
    rng = np.random.default_rng(3)
    n, dim = 600, 65
    with make_index(kind, dim, n + 50) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        ids = rng.permutation(n)[:257].astype(np.int64)
        ids[100] = ids[256] = ids[0]  # one id in slots 0, 100 and 256: the last wins
        src, f32 = source(rng, 257, dim, torch.float32, where)
        c = do_update(ix, kind, src, f32, ids=ids, what="three slots, one id")
        assert c == (255, 0, 2)
        assert torch.equal(ix.stored_rows(int(ids[0]), 1).view(torch.int16), torch.from_numpy(f32[256:257]).to(DEV).to(ix.dtype).view(torch.int16))
        before = planes(ix)
        c = do_update(ix, kind, src, f32, ids=ids, what="the same call again")  # (and the owner table was clean)
        assert c == (255, 0, 2) and all(torch.equal(before[k], v) for k, v in planes(ix).items())
        c = do_update(ix, kind, *source(rng, 257, dim, torch.float16, where), ids=np.full(257, 77), what="257 slots, one id")
        assert c == (1, 0, 256)
        ids = rng.permutation(n)[:257].astype(np.int64)
        ids[[0, 5, 64, 255]] = [-1, n, n + 49, -(2**40)]  # a pad, the first id past ntotal (inside the capacity), a far one
        ids[256] = 2**40
        c = do_update(ix, kind, *source(rng, 257, dim, torch.float32, where), ids=ids, mode="add", alpha=-0.125, what="pads and strangers")
        assert c == (252, 5, 0)
        before = planes(ix)
        c = do_update(ix, kind, *source(rng, 5, dim, torch.float32, where), ids=[-1, n, -7, n + 1, 2**62], what="nothing but pads")
        assert c == (0, 5, 0) and all(torch.equal(before[k], v) for k, v in planes(ix).items())
        # a second, different update right behind: the owner words of the calls above are all back to zero
        do_update(ix, kind, *source(rng, 257, dim, torch.float32, where), ids=rng.permutation(n)[:257], what="a different list right after")


def test_add_to_rows_check_raises_on_a_duplicate_and_check_false_applies_the_last_slot():
    rng = np.random.default_rng(4)
    n, dim = 40, 64
    with make_index("exact", dim, n) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        src, f32 = source(rng, 3, dim, torch.float32, "device")
        want, counts = R.apply_update(master(ix), f32, ids=[9, 4, 9], mode="add", alpha=0.5)
        assert counts == (2, 0, 1)
        with pytest.raises(ValueError, match="repeat"):
            ix.add_to_rows(src, alpha=0.5, ids=[9, 4, 9])
        with fresh_like(ix, "exact", want) as fr:  # (the rows were written before the count was read)
            assert_same_store(ix, fr, "check=True")
        do_update(ix, "exact", src, f32, ids=[9, 4, 9], mode="add", alpha=0.5, check=False, what="check=False")
        ix.add_to_rows(src, alpha=0.5, begin=0)  # (a dense call has no list to check)


# ---- values that saturate or are not finite ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_saturating_and_non_finite_values_match_the_ingest(kind):
    rng = np.random.default_rng(5)
    n, dim = 64, 65
    with make_index(kind, dim, n) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        f32 = rng.standard_normal((6, dim)).astype(np.float32)
        f32[0, 3] = 1.0e6          # beyond fp16: saturates to 65504 in the 16-bit plane
        f32[1, :] = -7.0e4         # a whole row beyond fp16: |x~|^2 = 65 * 65504^2 is beyond an fp16 L2 split too
        f32[2, 0] = np.inf
        f32[3, 64] = -np.inf
        f32[4, 7] = np.nan
        f32[5, 1] = 65519.0        # rounds to 65504 without saturating
        want, _ = R.apply_update(master(ix), f32, ids=[1, 2, 3, 5, 8, 13])
        sat0 = ix.get_stat("l2_saturated_rows") if kind == "l2" else 0
        ix.update_rows(torch.from_numpy(f32).to(DEV), ids=[1, 2, 3, 5, 8, 13])
        with fresh_like(ix, kind, want) as fr:
            assert_same_store(ix, fr, "non-finite SET")
            if kind == "l2":  # the count grows by the saturated splits of this call: the fresh index saw exactly those
                grew = fr.get_stat("l2_saturated_rows")
                assert grew >= 3 and ix.get_stat("l2_saturated_rows") == sat0 + grew
        # ADD that saturates (finite + finite beyond the range); the non-finite rows are SET back first (inf - inf has no one NaN)
        do_update(ix, kind, *source(rng, 6, dim, torch.float32, "device"), ids=[1, 2, 3, 5, 8, 13], what="back to ordinary rows")
        big = np.full((2, dim), 6.0e4, dtype=np.float32)
        do_update(ix, kind, torch.from_numpy(big).to(DEV), big, ids=[20, 21], what="SET 6e4")
        do_update(ix, kind, torch.from_numpy(big).to(DEV), big, ids=[20, 30], mode="add", alpha=1.0, what="ADD 6e4 onto 6e4 and onto N(0, 1)")


# ---- behaviour through the scans --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_searches_and_scans_agree_with_the_fresh_index(kind):
    rng = np.random.default_rng(6)
    n, dim, nq, k = 3000, 96, 16, 10
    with make_index(kind, dim, n) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float32)).to(DEV)
        ix.search(q, k)  # (an exact store derives its statistics here: the update has to make them dirty again)
        ids = rng.permutation(n)[:700]
        src, f32 = source(rng, 700, dim, torch.float32, "device")
        want, _ = R.apply_update(master(ix), f32 * 3.0, ids=ids)
        ix.update_rows(src * 3.0, ids=ids)
        want, _ = R.apply_update(want if kind == "exact" else master(ix), f32, begin=100, mode="add", alpha=-0.125)
        ix.add_to_rows(src, alpha=-0.125, begin=100)
        with fresh_like(ix, kind, want) as fr:
            assert_same_store(ix, fr, "before the scans")
            s0, i0 = ix.search(q, k)
            s1, i1 = fr.search(q, k)
            assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))  # (L2: the distances)
            if kind != "l2":
                listed = torch.from_numpy(rng.integers(-1, n + 2, size=(nq, 33))).to(DEV)
                assert torch.equal(ix.score_ids(q, listed).view(torch.int32), fr.score_ids(q, listed).view(torch.int32))
            if kind == "plain":
                a, b = ix.log_partition(q), fr.log_partition(q)
                assert torch.equal(a.max_score.view(torch.int32), b.max_score.view(torch.int32))
                assert torch.equal(a.log_rel.view(torch.int32), b.log_rel.view(torch.int32))


def test_value_table_and_labels_survive_an_update():
    rng = np.random.default_rng(8)
    n, dim, nq, cols = 1500, 64, 8, 5
    x = rng.standard_normal((n, dim)).astype(np.float32)
    values = rng.standard_normal((n, cols)).astype(np.float32)
    labels = rng.integers(0, 4, size=n).astype(np.int32)
    q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float32)).to(DEV)
    subset = rng.integers(0, 4, size=(nq, 2)).astype(np.int32)
    with make_index("plain", dim, n) as ix:
        ix.add(x)
        ix.set_row_values(values)
        ix.set_row_labels(labels)
        ids = rng.permutation(n)[:300]
        src, f32 = source(rng, 300, dim, torch.float32, "device")
        want, _ = R.apply_update(master(ix), f32, ids=ids)
        ix.update_rows(src, ids=ids)
        assert ix.row_values_shape == (n, cols)
        with fresh_like(ix, "plain", want) as fr:
            fr.set_row_values(values)
            fr.set_row_labels(labels)
            for sub in (None, subset):
                a, b = ix.posterior_expectation(q, subset=sub), fr.posterior_expectation(q, subset=sub)
                assert torch.equal(a.values.view(torch.int32), b.values.view(torch.int32))
                assert torch.equal(a.log_partition.log_z.view(torch.int32), b.log_partition.log_z.view(torch.int32))
            s0, i0 = ix.search(q, 10, subset=subset)
            s1, i1 = fr.search(q, 10, subset=subset)
            assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))


# ---- exact statistics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0e6, 1.0e8])
def test_exact_statistics_follow_the_rows_now_stored(scale):
    # |x|^2 of the scaled row is scale^2 times an ordinary row's and scale^2 / 4096 times a 64-fold row's.  The outlier cuts are the
    # maximum / 4^j, j <= 15: left in place, the maximum of the row that was replaced keeps the cuts near it - at 1e8 (1e16 / 4096 >
    # 4^15) above every row now stored, so no outlier would be found
    rng = np.random.default_rng(9)
    n, dim = 2004, 64
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[[10, 900, 1999]] *= 64.0
    x[1234] *= scale
    q = torch.from_numpy(rng.standard_normal((8, dim)).astype(np.float32)).to(DEV)
    with make_index("exact", dim, n) as ix:
        ix.add(x)
        ix.search(q, 5)
        ordinary = rng.standard_normal((1, dim)).astype(np.float32)
        ix.update_rows(torch.from_numpy(ordinary).to(DEV), ids=[1234])
        x[1234] = ordinary[0]
        with fresh_like(ix, "exact", x) as fr:
            s0, i0 = ix.search(q, 5)
            s1, i1 = fr.search(q, 5)
            assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
            assert fr.get_stat("exact_outliers") == 3  # (the level rule: the three rows scaled by 64)
            assert ix.get_stat("exact_outliers") == 3
            assert ix.get_stat("last_exact_band_queries") == fr.get_stat("last_exact_band_queries")
            assert_same_store(ix, fr, "exact statistics")


# ---- order of operations, refusals ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_update_then_add_and_add_then_update(kind):
    rng = np.random.default_rng(10)
    n, dim = 300, 65
    with make_index(kind, dim, 2 * n) as ix:
        x = rng.standard_normal((n, dim)).astype(np.float32)
        ix.add(x)
        do_update(ix, kind, *source(rng, 50, dim, torch.float32, "device"), ids=rng.permutation(n)[:50], what="update")
        first = master(ix)
        more = rng.standard_normal((n, dim)).astype(np.float32)
        ix.add(more)
        with fresh_like(ix, kind, np.concatenate([first, more])) as fr:
            assert_same_store(ix, fr, "update then add")
        do_update(ix, kind, *source(rng, 40, dim, torch.float32, "host"), ids=n + rng.permutation(n)[:40], what="add then update of the new rows")
        do_update(ix, kind, *source(rng, n, dim, torch.float32, "device"), begin=n, mode="add", alpha=-0.125, what="dense ADD of the new rows")


def test_refusals_leave_the_store_unchanged():
    rng = np.random.default_rng(11)
    n, dim = 100, 64
    lib = _native.load_library()
    with make_index("plain", dim, n + 10) as ix:
        ix.add(rng.standard_normal((n, dim)).astype(np.float32))
        before = planes(ix)
        src = torch.from_numpy(rng.standard_normal((4, dim)).astype(np.float32)).to(DEV)
        ids = torch.tensor([1, 2, 3, 4], dtype=torch.int64, device=DEV)
        stream = _native.current_stream_ptr(DEV)

        def call(ids_ptr, begin, rows_ptr, cnt, dt=_native.F32, loc=_native.DEVICE, mode=_native.UPDATE_SET, alpha=1.0):
            return lib.vodhip_index_update_rows(ix._h, ids_ptr, begin, rows_ptr, cnt, dt, loc, mode, alpha, 0, stream)

        q = torch.from_numpy(rng.standard_normal((4, dim)).astype(np.float32)).to(DEV)
        ix.search_async(q, 5)
        with pytest.raises(_native.NativeLibraryError, match="in flight"):
            ix.update_rows(src, ids=ids)
        with pytest.raises(_native.NativeLibraryError, match="in flight"):
            ix.add_to_rows(src, begin=0)
        ix.finish()
        for bad, text in (
            (lambda: call(None, -1, src.data_ptr(), 4), "out of bounds"),
            (lambda: call(None, n - 3, src.data_ptr(), 4), "out of bounds"),
            (lambda: call(None, n + 1, src.data_ptr(), 0), "out of bounds"),
            (lambda: call(ids.data_ptr(), 0, src.data_ptr(), -1), "negative"),
            (lambda: call(ids.data_ptr(), 0, None, 4), "rows is NULL"),
            (lambda: call(ids.data_ptr(), 0, src.data_ptr(), 4, dt=3), "src_dtype"),
            (lambda: call(ids.data_ptr(), 0, src.data_ptr(), 4, dt=-1), "src_dtype"),
            (lambda: call(ids.data_ptr(), 0, src.data_ptr(), 4, loc=2), "location"),
            (lambda: call(ids.data_ptr(), 0, src.data_ptr(), 4, mode=2), "mode"),
            (lambda: call(ids.data_ptr(), 0, src.data_ptr(), 4, mode=_native.UPDATE_ADD, alpha=float("inf")), "alpha"),
            (lambda: call(ids.data_ptr(), 0, src.data_ptr(), 4, mode=_native.UPDATE_ADD, alpha=float("nan")), "alpha"),
        ):
            assert bad() == -1
            assert text in lib.vodhip_last_error().decode()
        torch.cuda.synchronize()
        assert all(torch.equal(before[k], v) for k, v in planes(ix).items())
        # what succeeds: n == 0 (also at the very end of the store, also with NULL rows), and a SET whose alpha is not finite
        assert call(None, n, None, 0) == 0 and call(ids.data_ptr(), 0, None, 0) == 0
        assert (ix.get_stat("last_update_written"), ix.get_stat("last_update_skipped"), ix.get_stat("last_update_duplicates")) == (0, 0, 0)
        assert all(torch.equal(before[k], v) for k, v in planes(ix).items())
        assert call(ids.data_ptr(), 0, src.data_ptr(), 4, alpha=float("nan")) == 0
        torch.cuda.synchronize()
        assert torch.equal(ix.stored_rows(1, 4).view(torch.int16), src.to(torch.float16).view(torch.int16))
        with pytest.raises(ValueError):
            ix.update_rows(src, ids=[1, 2, 3])
        with pytest.raises(ValueError):
            ix.update_rows(src[:, :-1].contiguous(), begin=0)


# ---- node index -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [False, True], ids=["plain", "exact"])
@pytest.mark.parametrize("n_shards", [2, 3])
def test_node_index_routes_slots_to_their_shards(n_shards, exact):
    rng = np.random.default_rng(12 + n_shards)
    n, dim = 600, 65
    rps = n // n_shards
    kind = "exact" if exact else "plain"
    x = rng.standard_normal((n, dim)).astype(np.float32)
    lib = _native.load_library()
    with HipNodeIndex(dim, n, [0] * n_shards, exact_f32=exact) as nx, make_index(kind, dim, n) as flat:
        nx.add(x)
        flat.add(x)

        def same_as_flat(what):
            for g in range(n_shards):
                h, base, _ = nx.shard(g)
                rows = torch.empty((rps, dim), dtype=torch.float16, device=DEV)
                _native.check(lib.vodhip_index_get_rows(ctypes.c_void_p(h), 0, rps, rows.data_ptr(), _native.DEVICE, _native.current_stream_ptr(DEV)))
                assert base == g * rps
                assert torch.equal(rows.view(torch.int16), flat.stored_rows(base, rps).view(torch.int16)), f"{what}: shard {g} rows"
                assert torch.equal(padded_plane(ctypes.c_void_p(h), rps), padded_plane(flat._h, n)[base:base + rps]), f"{what}: shard {g} plane"
                if exact:
                    f32 = torch.empty((rps, dim), dtype=torch.float32, device=DEV)
                    _native.check(lib.vodhip_index_get_rows_f32(ctypes.c_void_p(h), 0, rps, f32.data_ptr(), _native.DEVICE, _native.current_stream_ptr(DEV)))
                    assert torch.equal(f32.view(torch.int32), flat.stored_rows_f32(base, rps).view(torch.int32)), f"{what}: shard {g} float32"
            for key in ("last_update_written", "last_update_skipped", "last_update_duplicates"):
                assert nx.get_stat(key) == flat.get_stat(key), (what, key)

        # ids on both sides of every shard edge, a duplicate pair inside shard 0, a pad and an id past the store
        ids = np.concatenate([rng.permutation(n)[:40], [rps - 1, rps, n - 1, 0, 7, -1, n, 7]]).astype(np.int64)
        rows = rng.standard_normal((len(ids), dim)).astype(np.float32)
        nx.update_rows(rows, ids=ids)
        flat.update_rows(rows, ids=ids)
        same_as_flat("listed SET")
        assert nx.get_stat("last_update_skipped") == 2 and nx.get_stat("last_update_duplicates") >= 1
        uniq = rng.permutation(n)[:64].astype(np.int64)
        delta = rng.standard_normal((64, dim)).astype(np.float16)
        nx.add_to_rows(delta, alpha=-0.125, ids=uniq)
        flat.add_to_rows(delta, alpha=-0.125, ids=uniq)
        same_as_flat("listed ADD")
        with pytest.raises(ValueError, match="repeat"):
            nx.add_to_rows(delta[:2], ids=[5, 5])
        flat.add_to_rows(delta[:2], ids=[5, 5], check=False)
        same_as_flat("a duplicate ADD")
        span = rng.standard_normal((min(rps + 20, n - (rps - 10)), dim)).astype(np.float32)  # crosses every boundary behind shard 0
        nx.update_rows(span, begin=rps - 10)
        flat.update_rows(span, begin=rps - 10)
        same_as_flat("dense SET across a boundary")
        nx.add_to_rows(span[:30], alpha=3e-4, begin=n - 30)
        flat.add_to_rows(span[:30], alpha=3e-4, begin=n - 30)
        same_as_flat("dense ADD at the end")
        with pytest.raises(_native.NativeLibraryError, match="out of bounds"):
            nx.update_rows(span, begin=n - 10)


# ---- the training loop the call closes --------------------------------------------------------------------------------------------
def test_training_step_through_read_out_and_add_to_rows():
    # (key_gradient refuses exact_f32 stores, as posterior_adjoint does: the loop runs on the plain fp16 store, whose master copy is
    # the 16-bit row)
    rng = np.random.default_rng(13)
    n, dim, nq, cols = 700, 64, 12, 6
    with make_index("plain", dim, n) as ix:
        ix.add((0.3 * rng.standard_normal((n, dim))).astype(np.float32))
        q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float32)).to(DEV)
        V = torch.from_numpy(rng.standard_normal((n, cols)).astype(np.float32)).to(DEV)
        keys = ix.stored_rows().float().requires_grad_()
        ix.read_out(q, V, keys=keys).sum().backward()
        assert keys.grad is not None and bool(torch.isfinite(keys.grad).all()) and float(keys.grad.abs().max()) > 0
        table = ix.row_values_shape
        want, _ = R.apply_update(keys.detach().cpu().numpy(), keys.grad.cpu().numpy(), begin=0, mode="add", alpha=-0.5)
        ix.add_to_rows(keys.grad, alpha=-0.5)
        with fresh_like(ix, "plain", want) as fr:
            assert_same_store(ix, fr, "the step")
        assert ix.row_values_shape == table and table is not None
        y = ix.posterior_expectation(q)  # the table is still attached: no set_row_values in between
        assert bool(torch.isfinite(y.values).all())
        # the other route: the caller's float32 parameter, stepped and written back
        with torch.no_grad():
            keys -= 0.5 * keys.grad
        ix.update_rows(keys.detach())
        with fresh_like(ix, "plain", keys.detach().cpu().numpy()) as fr:
            assert_same_store(ix, fr, "update_rows(keys)")
