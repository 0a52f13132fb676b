"""HBM-resident corpus vector store + exact inner-product top-k (host wrapper over the C-ABI).

Mirrors what the reference gets from a faiss `IndexFlat` with METRIC_INNER_PRODUCT:
`index.add(float32 batch)` (/root/reference/src/vod_search/faiss_search/build.py:65-73) and
`index.search(query_vec, k)` (/root/reference/src/vod_search/faiss_search/server.py:72,84).
PyTorch is used only to own the query / result buffers and the stream; the store itself is owned by
libvodhip.so.
"""
from __future__ import annotations

import collections
import ctypes
import math
from typing import Any, NamedTuple

import numpy as np
import torch

from vod_amd import _native


def pad_listed_ids(ids, nq: int | None = None) -> np.ndarray:
    """`ids` of `score_ids` as a C-contiguous int64 [nq, m] NumPy array: an array is taken as it is, a ragged list of lists is padded
    with -1 (an empty slot) to its longest row - at least one column, so that a batch of empty lists is still a list."""
    if isinstance(ids, np.ndarray):
        arr = ids
    else:
        rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in ids]
        arr = np.full((len(rows), max(1, max((len(r) for r in rows), default=0))), -1, dtype=np.int64)
        for i, r in enumerate(rows):
            arr[i, : len(r)] = r
    arr = np.ascontiguousarray(arr, dtype=np.int64)
    if arr.ndim != 2 or (nq is not None and arr.shape[0] != nq):
        raise ValueError(f"expected ids of shape [{'nq' if nq is None else nq}, m], got {tuple(arr.shape)}")
    return arr


def pad_listed_weights(weights, shape: tuple[int, int]) -> np.ndarray:
    """`weights` of `sum_ids` as a C-contiguous float32 NumPy array of `shape` = the shape of the padded ids: an array is taken as it is,
    a ragged list of lists is padded with 0 (a zero weight skips its slot)."""
    if isinstance(weights, np.ndarray):
        arr = weights
    else:
        rows = [np.asarray(r, dtype=np.float32).reshape(-1) for r in weights]
        if len(rows) != shape[0] or any(len(r) > shape[1] for r in rows):
            raise ValueError(f"expected weights of shape {tuple(shape)}, got {len(rows)} rows of up to {max((len(r) for r in rows), default=0)}")
        arr = np.zeros(shape, dtype=np.float32)
        for i, r in enumerate(rows):
            arr[i, : len(r)] = r
    arr = np.ascontiguousarray(arr, dtype=np.float32)
    if arr.shape != tuple(shape):
        raise ValueError(f"expected weights of shape {tuple(shape)}, got {tuple(arr.shape)}")
    return arr


def _host_update_args(vectors, ids, dim: int):
    """Host `vectors` / `ids` of `update_rows` / `add_to_rows` as C-contiguous NumPy: float16 / float32 `[n, dim]` and int64 `[n]` (or None)."""
    if isinstance(vectors, torch.Tensor):
        vectors = vectors.detach()
        vectors = vectors.numpy() if vectors.dtype != torch.bfloat16 else vectors.float().numpy()
    v = np.ascontiguousarray(vectors)
    if v.dtype not in (np.float16, np.float32):
        v = v.astype(np.float32)
    if v.ndim != 2 or v.shape[1] != dim:
        raise ValueError(f"expected [n, {dim}] vectors, got {v.shape}")
    ida = None
    if ids is not None:
        if isinstance(ids, torch.Tensor):
            ids = ids.detach().cpu().numpy()
        ida = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
        if ida.size != v.shape[0]:
            raise ValueError(f"expected {v.shape[0]} ids, got {ida.size}")
    return v, ida


def remove_rows_args(ids, begin: int, n, mask, ntotal: int):
    """The three spellings of `remove_rows` as the native call takes them: `(ids, begin, n)` with `ids` None (the range
    `begin .. begin + n`) or an int64 id list (`begin` is 0 and `n` its length then).  A list stays what it was - a device tensor is
    not copied to the host; a boolean `mask` of length `ntotal` becomes the ids of its True entries.  Exactly one spelling per call."""
    given = [ids is not None, mask is not None, n is not None]
    if sum(given) != 1 or (begin != 0 and n is None):
        raise ValueError("remove_rows takes exactly one of: ids=, mask=, or the range begin= / n=")
    if n is not None:
        begin, n = int(begin), int(n)
        if n < 0 or begin < 0 or begin + n > ntotal:
            raise ValueError(f"rows [{begin}, {begin} + {n}) are outside the {ntotal} stored rows")
        return None, begin, n
    if mask is not None:
        if isinstance(mask, torch.Tensor):
            if mask.dtype != torch.bool or mask.ndim != 1 or mask.numel() != ntotal:
                raise ValueError(f"expected a boolean mask of length {ntotal}, got {mask.dtype} {tuple(mask.shape)}")
            ids = torch.nonzero(mask.detach()).reshape(-1)
        else:
            m = np.asarray(mask)
            if m.dtype != np.bool_ or m.ndim != 1 or m.size != ntotal:
                raise ValueError(f"expected a boolean mask of length {ntotal}, got {m.dtype} {m.shape}")
            ids = np.flatnonzero(m).astype(np.int64)
    if isinstance(ids, torch.Tensor):
        ids = ids.detach().to(torch.int64).contiguous().reshape(-1)
        if not ids.is_cuda:
            ids = ids.numpy()
    if not isinstance(ids, torch.Tensor):
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.int64)
    return ids, 0, int(ids.numel() if isinstance(ids, torch.Tensor) else ids.size)


class HipFlatIndex:
    """Exact MIPS index: row-major fp16/bf16 rows in HBM, searched by the fused MFMA + top-k kernels.

    `exact_f32=True` (VODHIP_EXACT_F32): the store also keeps the float32 rows and every search returns what a float32 brute force
    over the UNROUNDED rows and queries returns - the reference's own arithmetic (faiss IndexFlat holds float32,
    /root/reference/src/vod_search/faiss_search/build.py:65-73) - with the fp16 / bf16 scan as the filter.  Without it scores are
    dot products of the values as rounded to `dtype`.

    `metric="l2"` (VODHIP_L2; faiss `index_factory(D, "Flat", METRIC_L2)`): searches return SQUARED L2 distances of the stored
    (rounded) rows and the rounded queries, ascending.  The store keeps three bias columns per row behind the user's `dim` (they
    show in `dim_pad` only: `add`, `stored_rows` and `save` speak `dim`).  Not combined with `exact_f32`; `score_ids` raises."""

    def __init__(self, dim: int, capacity: int, dtype: torch.dtype = torch.float16, device: int | torch.device = 0,
                 exact_f32: bool = False, metric: str = "inner_product"):
        self._lib = _native.load_library()
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("HipFlatIndex needs a ROCm device (torch.cuda.is_available() is False)")
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError("store dtype must be torch.float16 or torch.bfloat16")
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.dim = int(dim)
        self.capacity = int(capacity)
        self.dtype = dtype
        self.exact_f32 = bool(exact_f32)
        self.metric = metric
        flags = _native.metric_flag(metric) | (_native.EXACT_F32 if self.exact_f32 else 0)
        handle = ctypes.c_void_p()
        _native.check(
            self._lib.vodhip_index_create(
                self.device.index or 0, self.dim, _native.torch_dtype_code(dtype) | flags,
                self.capacity, ctypes.byref(handle)
            )
        )
        self._h = handle
        self._keep: collections.deque = collections.deque()
        self._keep_subset = None

    # -- lifecycle ---------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vodhip_index_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "HipFlatIndex":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    # -- store -------------------------------------------------------------------------------------
    @property
    def ntotal(self) -> int:
        out = ctypes.c_int64()
        _native.check(self._lib.vodhip_index_ntotal(self._h, ctypes.byref(out)))
        return out.value

    def reset(self) -> None:
        _native.check(self._lib.vodhip_index_reset(self._h))

    def add(self, vectors: np.ndarray | torch.Tensor) -> None:
        """Append rows (float32/float16 NumPy on the host, or float32/float16/bfloat16 tensors on this device)."""
        if isinstance(vectors, torch.Tensor) and vectors.is_cuda:
            if vectors.device != self.device:
                raise ValueError(f"vectors live on {vectors.device}, the index on {self.device}")
            v = vectors.contiguous()
            if v.ndim != 2 or v.shape[1] != self.dim:
                raise ValueError(f"expected [n, {self.dim}] vectors, got {tuple(v.shape)}")
            _native.check(
                self._lib.vodhip_index_add(
                    self._h, v.data_ptr(), v.shape[0], _native.torch_dtype_code(v.dtype), _native.DEVICE,
                    _native.current_stream_ptr(self.device),
                )
            )
            torch.cuda.current_stream(self.device).synchronize()  # `v` may be freed by the caller right after
            return
        if isinstance(vectors, torch.Tensor):
            vectors = vectors.numpy() if vectors.dtype != torch.bfloat16 else vectors.float().numpy()
        v = np.ascontiguousarray(vectors)
        if v.dtype not in (np.float16, np.float32):
            v = v.astype(np.float32)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"expected [n, {self.dim}] vectors, got {v.shape}")
        with torch.cuda.device(self.device):
            _native.check(
                self._lib.vodhip_index_add(
                    self._h, v.ctypes.data, v.shape[0], _native.numpy_dtype_code(v.dtype), _native.HOST,
                    _native.current_stream_ptr(self.device),
                )
            )

    def stored_rows(self, begin: int = 0, n: int | None = None) -> torch.Tensor:
        """Copy of the stored (rounded) rows [begin, begin+n) as a device tensor [n, dim] (an L2 store's bias columns are not part of
        it) -- tests / persistence."""
        n = self.ntotal - begin if n is None else int(n)
        out = torch.empty((n, self.dim), dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(
                self._lib.vodhip_index_get_rows(self._h, int(begin), n, out.data_ptr(), _native.DEVICE,
                                                _native.current_stream_ptr(self.device))
            )
        return out

    def stored_rows_f32(self, begin: int = 0, n: int | None = None) -> torch.Tensor:
        """Copy of the float32 rows [begin, begin+n) of an `exact_f32` store (what was added, bit for bit)."""
        n = self.ntotal - begin if n is None else int(n)
        out = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(
                self._lib.vodhip_index_get_rows_f32(self._h, int(begin), n, out.data_ptr(), _native.DEVICE,
                                                    _native.current_stream_ptr(self.device))
            )
        return out

    # -- rows changed in place (H2u) ------------------------------------------------------------------
    def _update(self, mode: int, vectors, alpha: float, ids, begin: int) -> None:
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device)
            if isinstance(vectors, torch.Tensor) and vectors.is_cuda:
                if vectors.device != self.device:
                    raise ValueError(f"vectors live on {vectors.device}, the index on {self.device}")
                v = vectors.detach()
                if v.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                    v = v.float()
                if not v.is_contiguous():  # (a contiguous view keeps its own - possibly misaligned - address: the kernel handles it)
                    v = v.contiguous()
                if v.ndim != 2 or v.shape[1] != self.dim:
                    raise ValueError(f"expected [n, {self.dim}] vectors, got {tuple(v.shape)}")
                idt = None
                if ids is not None:
                    idt = torch.as_tensor(ids, dtype=torch.int64).to(self.device).contiguous().reshape(-1)
                    if idt.numel() != v.shape[0]:
                        raise ValueError(f"expected {v.shape[0]} ids, got {idt.numel()}")
                _native.check(self._lib.vodhip_index_update_rows(
                    self._h, idt.data_ptr() if idt is not None and idt.numel() else None, int(begin), v.data_ptr() if v.numel() else None, v.shape[0],
                    _native.torch_dtype_code(v.dtype), _native.DEVICE, mode, float(alpha), 0, stream))
                torch.cuda.current_stream(self.device).synchronize()  # `v` and the ids may be freed by the caller right after
                return
            v, ida = _host_update_args(vectors, ids, self.dim)
            _native.check(self._lib.vodhip_index_update_rows(
                self._h, ida.ctypes.data if ida is not None and ida.size else None, int(begin), v.ctypes.data if v.size else None, v.shape[0],
                _native.numpy_dtype_code(v.dtype), _native.HOST, mode, float(alpha), 0, stream))

    def update_rows(self, vectors: np.ndarray | torch.Tensor, ids=None, begin: int = 0) -> None:
        """Overwrite stored rows in place: `x[ids] = vectors`, or with `ids=None` the rows `begin .. begin + n`.  `vectors` is `[n, dim]`,
        a device tensor (f16 / bf16 / f32) or host NumPy / CPU tensor, as for `add`; `ids` is `[n]` int64 (global row ids of THIS
        index).  Every plane of the store is rewritten as `add` would have written it: afterwards the index equals, byte for byte, one
        built by `add` from the final rows.  `ntotal`, the row labels and the value table stay (`set_row_values` survives, unlike
        `reset(); add(...)`).  An id that is negative or not below `ntotal` is skipped; when an id repeats the LAST slot wins, as
        NumPy's `x[ids] = rows`.  `get_stat("last_update_written" | "last_update_skipped" | "last_update_duplicates")` tells.
        Refused while searches are in flight, like `add`."""
        self._update(_native.UPDATE_SET, vectors, 1.0, ids, begin)

    def add_to_rows(self, delta: np.ndarray | torch.Tensor, alpha: float = 1.0, ids=None, begin: int = 0, check: bool = True) -> None:
        """`x[ids] += alpha * delta` in place (`ids=None`: the rows `begin .. begin + n`), in float32 with two roundings
        (`alpha * delta`, then the sum), then stored as `add` stores the result - the SGD step `add_to_rows(keys.grad, alpha=-lr)`.

        On a plain 16-bit store the master copy IS the 16-bit row: a step below half an ulp of the row is lost, every time.  An
        `exact_f32` store keeps the float32 master and adds to that.  For optimisers with state (momentum, Adam) or steps that small
        keep the float32 `keys` parameter yourself, step it with the optimiser, and write it back with `update_rows(keys)`.

        Ids must be unique: with a repeated id only its last slot is applied.  `check=True` reads `last_update_duplicates` after a
        listed call (one synchronisation) and raises ValueError when it is not zero - the rows are already written then."""
        self._update(_native.UPDATE_ADD, delta, alpha, ids, begin)
        if check and ids is not None and (dup := self.get_stat("last_update_duplicates")):
            raise ValueError(f"add_to_rows: {dup} slots repeat an id that a later slot lists too; only the last slot of an id was applied")

    # -- rows removed, the gaps closed in place (H2r) ------------------------------------------------------
    def remove_rows(self, ids=None, begin: int = 0, n: int | None = None, mask=None, return_map: bool = False):
        """Remove stored rows and close the gaps in place, as faiss `IndexFlat.remove_ids`: `ids` (int64 row ids, host or device),
        or the range `begin .. begin + n`, or a boolean `mask` of length `ntotal` (True = remove).  The compaction is stable: a
        survivor's new id is its old id minus the number of removed rows below it.  Every plane of the store - the rows, an
        `exact_f32` store's float32 rows and statistics, the row labels, the value table - is compacted the same way and equals,
        byte for byte, an index freshly built by `add` from the survivors; labels and table stay attached (unlike `reset(); add(...)`).
        An id that is negative or not below `ntotal` is skipped, a repeated id removes its row once:
        `get_stat("last_remove_removed" | "last_remove_skipped" | "last_remove_duplicates")` tells.  Returns the number of rows
        removed; with `return_map=True` the pair `(removed, new_ids)`, `new_ids` a device int64 tensor `[old ntotal]` with the new id
        of every old row and -1 for a removed one - what remaps gold ids and side tables.  Waits for the device once.  Refused while
        searches are in flight, like `add`, and when rows were added after `set_row_values` (the table is short then and describes
        other rows: set it again or clear it first).  A device error during the call leaves the store undefined: `reset()` it."""
        old = self.ntotal
        ida, begin, n = remove_rows_args(ids, begin, n, mask, old)
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device)
            on_device = isinstance(ida, torch.Tensor)
            if on_device and ida.device != self.device:
                raise ValueError(f"ids live on {ida.device}, the index on {self.device}")
            new_ids = torch.arange(old, dtype=torch.int64, device=self.device) if return_map else None  # (an empty call writes no map: the identity)
            ptr = None
            if ida is not None and n:
                ptr = ida.data_ptr() if on_device else ida.ctypes.data
            removed = ctypes.c_int64()
            _native.check(self._lib.vodhip_index_remove_rows(
                self._h, ptr, begin, n, _native.DEVICE if on_device else _native.HOST, 0, new_ids.data_ptr() if return_map and old else None,
                ctypes.byref(removed), stream))
            if on_device:
                torch.cuda.current_stream(self.device).synchronize()  # the ids may be freed by the caller right after
        return (removed.value, new_ids) if return_map else removed.value

    # -- subset filter ---------------------------------------------------------------
    def set_row_labels(self, labels: np.ndarray | torch.Tensor | None) -> None:
        """Attach an int32 subset label to every stored row (None clears).  Needed before `search(..., subset=...)`."""
        with torch.cuda.device(self.device):
            if labels is None:
                _native.check(self._lib.vodhip_index_set_row_labels(self._h, None, 0, _native.HOST, None))
                return
            if isinstance(labels, torch.Tensor) and labels.is_cuda:
                lab = labels.to(torch.int32).contiguous()
                _native.check(self._lib.vodhip_index_set_row_labels(self._h, lab.data_ptr(), lab.numel(), _native.DEVICE,
                                                                    _native.current_stream_ptr(self.device)))
                return
            lab = np.ascontiguousarray(np.asarray(labels), dtype=np.int32)
            _native.check(self._lib.vodhip_index_set_row_labels(self._h, lab.ctypes.data, lab.size, _native.HOST,
                                                                _native.current_stream_ptr(self.device)))

    # -- value table of the posterior read-out ---------------------------------------------------------
    def set_row_values(self, values: np.ndarray | torch.Tensor | None) -> None:
        """Attach a value row `[n_cols]` (1 <= n_cols <= 256) to every stored row: `values` is `[ntotal, n_cols]` (a vector is one
        column), NumPy or torch, host or device, fp16 / bf16 / fp32 (anything else is cast to fp32); None clears.  The index keeps a copy
        in the store dtype, rounded as the rows are.  `reset` drops the table, `save` / `load` do not carry it, and rows added afterwards
        leave it short (`posterior_expectation` then refuses).  Needed before `posterior_expectation`."""
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device)
            if values is None:
                _native.check(self._lib.vodhip_index_set_row_values(self._h, None, 0, 0, 0, _native.HOST, stream))
                return
            if isinstance(values, torch.Tensor):
                v = values.detach()
                v = v.reshape(-1, 1) if v.ndim == 1 else v
                if v.ndim != 2:
                    raise ValueError(f"expected [ntotal, n_cols] values, got {tuple(values.shape)}")
                if v.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                    v = v.float()
                v = v.to(self.device).contiguous() if v.is_cuda else v.contiguous()
                src = v if v.numel() else v.new_zeros(1)  # (a table of no rows is still a table: NULL would clear it)
                _native.check(self._lib.vodhip_index_set_row_values(self._h, src.data_ptr(), v.shape[0], v.shape[1], _native.torch_dtype_code(v.dtype),
                                                                    _native.DEVICE if v.is_cuda else _native.HOST, stream))
                return
            v = np.asarray(values)
            v = v.reshape(-1, 1) if v.ndim == 1 else v
            if v.ndim != 2:
                raise ValueError(f"expected [ntotal, n_cols] values, got {tuple(v.shape)}")
            if v.dtype not in (np.float32, np.float16):
                v = v.astype(np.float32)
            v = np.ascontiguousarray(v)
            src = v if v.size else np.zeros(1, dtype=v.dtype)  # (a table of no rows is still a table: NULL would clear it)
            _native.check(self._lib.vodhip_index_set_row_values(self._h, src.ctypes.data, v.shape[0], v.shape[1],
                                                                2 if v.dtype == np.float32 else 0, _native.HOST, stream))

    @property
    def row_values_shape(self) -> tuple[int, int] | None:
        """`(n_rows, n_cols)` of the value table, or None when there is none."""
        return _row_values_shape(self._lib.vodhip_index_row_values_info, self._h)

    # -- persistence (the store itself is the on-disk format, no faiss file round trip) -----------
    def save(self, path, chunk: int = 1 << 20) -> None:
        """Write the stored rows (as stored: fp16, or bf16 widened to fp32; the float32 rows of an `exact_f32` store - what
        `faiss.write_index` persists for the reference, factory.py:167) to a `.npy`, slice by slice.  An L2 store writes the user's
        columns only: `load(..., metric="l2")` derives the bias columns again."""
        n = self.ntotal
        np_dtype = np.float16 if (self.dtype == torch.float16 and not self.exact_f32) else np.float32
        out = np.lib.format.open_memmap(path, mode="w+", dtype=np_dtype, shape=(n, self.dim))
        for lo in range(0, n, chunk):
            if self.exact_f32:
                rows = self.stored_rows_f32(lo, min(chunk, n - lo))
                out[lo : lo + rows.shape[0]] = rows.cpu().numpy()
                continue
            rows = self.stored_rows(lo, min(chunk, n - lo))
            out[lo : lo + rows.shape[0]] = (rows if self.dtype == torch.float16 else rows.float()).cpu().numpy()
        out.flush()
        del out

    @classmethod
    def load(cls, path, dtype: torch.dtype = torch.float16, device: int | torch.device = 0, capacity: int | None = None,
             chunk: int = 1 << 18, exact_f32: bool = False, metric: str = "inner_product") -> "HipFlatIndex":
        """Build an index of `metric` from a 2-D float16/float32 `.npy` (memory-mapped, streamed to HBM in slices)."""
        arr = np.load(path, mmap_mode="r", allow_pickle=False)
        if arr.ndim != 2:
            raise ValueError(f"expected a 2-D vector file, got shape {arr.shape}")
        ix = cls(arr.shape[1], max(capacity or arr.shape[0], 1), dtype=dtype, device=device, exact_f32=exact_f32, metric=metric)
        if arr.flags.c_contiguous:
            ix.add(arr)  # ONE call: the library pipelines page-cache reads, pinned staging and DMA itself (64 MB slices)
        else:
            for lo in range(0, arr.shape[0], chunk):
                ix.add(np.ascontiguousarray(arr[lo : lo + chunk]))
        return ix

    # -- search ------------------------------------------------------------------------------------
    def set_param(self, key: str, value: int) -> None:
        _native.check(self._lib.vodhip_index_set_param(self._h, key.encode(), int(value)))

    def get_stat(self, key: str) -> int:
        out = ctypes.c_int64()
        _native.check(self._lib.vodhip_index_get_stat(self._h, key.encode(), ctypes.byref(out)))
        return out.value

    def _prep_queries(self, queries) -> torch.Tensor:
        if isinstance(queries, np.ndarray):
            q = np.ascontiguousarray(queries)
            if q.dtype not in (np.float16, np.float32):
                q = q.astype(np.float32)
            queries = torch.from_numpy(q).to(self.device, non_blocking=False)
        q = queries
        if q.device != self.device:
            q = q.to(self.device)
        if q.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            q = q.float()
        q = q.contiguous()
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        return q

    def search_async(self, queries, k: int, id_base: int = 0, out: tuple[torch.Tensor, torch.Tensor] | None = None,
                     subset: np.ndarray | torch.Tensor | None = None):
        """Enqueue a search on the current stream; call `finish()` before trusting the outputs.

        `subset`: optional int32 [nq, S] allowed row labels per query (-1 = empty slot, all -1 = unrestricted).

        On a `metric="l2"` index the scores are squared L2 distances, ascending, ties -> smaller id, clamped at 0, pads (+inf, -1);
        `id_base`, `subset`, the lanes and up to 4 searches in flight work as for inner product."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            self._keep_subset = sub
            _native.check(self._lib.vodhip_index_set_query_labels(self._h, sub.data_ptr(), int(sub.shape[1])))
        else:
            self._keep_subset = None
            _native.check(self._lib.vodhip_index_set_query_labels(self._h, None, 0))
        if out is None:
            scores = torch.empty((nq, k), dtype=torch.float32, device=self.device)
            ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        else:
            scores, ids = out
        _native.check(
            self._lib.vodhip_index_search_async(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, int(k), int(id_base),
                scores.data_ptr(), ids.data_ptr(), _native.current_stream_ptr(self.device),
            )
        )
        # only a search the library accepted is tracked (a refused one synchronised the stream before returning);
        # its buffers stay alive until its finish()
        self._keep.append((q, self._keep_subset, scores, ids))
        return scores, ids

    def finish(self) -> None:
        """Complete the OLDEST enqueued search (up to 4 may be in flight): waits for it alone and, if a candidate list
        overflowed, runs recovery passes seeded from its incomplete result.  Pipelined searches need their own `out` buffers if their
        results are read after younger searches were enqueued."""
        _native.check(self._lib.vodhip_index_search_finish(self._h, _native.current_stream_ptr(self.device)))
        if self._keep:
            self._keep.popleft()

    def search(self, queries, k: int, id_base: int = 0, out=None, subset=None) -> tuple[torch.Tensor, torch.Tensor]:
        """Exact top-k by inner product: (scores f32 [nq,k] desc, ids i64 [nq,k]); ties -> smaller id; pad -inf/-1.

        `metric="l2"`: exact top-k by squared L2 distance of the rounded rows and queries: (distances f32 [nq,k] ASCENDING, ids);
        ties -> smaller id; distances are clamped at 0; pad +inf/-1 (faiss pads with +FLT_MAX)."""
        with torch.cuda.device(self.device):
            res = self.search_async(queries, k, id_base, out, subset)
            self.finish()
        return res

    def score_ids(self, queries, ids, k: int | None = None, *, subset=None, id_base: int = 0, out=None):
        """Scores of LISTED rows - the dense counterpart of `ids` in the reference's `SearchClient.search`, which its Elasticsearch client
        honours with a `terms` filter and its faiss client drops (/root/reference/src/vod_search/es_search/client.py:145,177-183,
        faiss_search/client.py:70).

        `ids`: int64 [nq, m] tensor / array, or a ragged list of lists (padded with -1).  A slot that is empty (id < 0), out of range
        (id - id_base outside [0, ntotal)) or whose row carries none of the query's `subset` labels scores -inf.
        `k=None`: float32 [nq, m] aligned to `ids` (`out`: that tensor).  `k=int`: (scores [nq, k], ids [nq, k]) - the k best distinct
        listed rows by (score desc, id asc), pads (-inf, -1); m <= 8192 (`out`: the pair).
        Enqueued on the current stream; nothing to finish, and safe beside searches of this index that are in flight.
        An L2 index refuses (the library's message: listed ids need an inner-product store)."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        if isinstance(ids, torch.Tensor):
            lst = ids.to(self.device, torch.int64).contiguous()
            if lst.ndim != 2 or lst.shape[0] != nq:
                raise ValueError(f"expected ids of shape [{nq}, m], got {tuple(lst.shape)}")
        else:
            lst = torch.from_numpy(pad_listed_ids(ids, nq)).to(self.device)
        m = int(lst.shape[1])
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        sub_ptr = None if sub is None else sub.data_ptr()
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device)
            if k is None:
                scores = torch.empty((nq, m), dtype=torch.float32, device=self.device) if out is None else out
                _native.check(self._lib.vodhip_index_score_ids(self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, lst.data_ptr(), m,
                                                               int(id_base), sub_ptr, n_sub, scores.data_ptr(), stream))
                res = scores
            else:
                if out is None:
                    scores = torch.empty((nq, int(k)), dtype=torch.float32, device=self.device)
                    top = torch.empty((nq, int(k)), dtype=torch.int64, device=self.device)
                else:
                    scores, top = out
                _native.check(self._lib.vodhip_index_search_ids(self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, lst.data_ptr(), m,
                                                                int(k), int(id_base), sub_ptr, n_sub, scores.data_ptr(), top.data_ptr(), stream))
                res = (scores, top)
        # inputs this call built itself (converted / uploaded copies) must outlive the launch: the caching allocator hands their blocks
        # out again in the order of the stream they were allocated on, which need not be the current one
        for t, given in ((q, queries), (lst, ids), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return res

    def sum_ids(self, ids, weights, *, subset=None, id_base: int = 0, out=None) -> torch.Tensor:
        """The weighted sum of LISTED rows, `out[q] = sum_j weights[q, j] * x~[ids[q, j] - id_base]`: float32 `[nq, dim]` on the device
        (`out`: that tensor).  It is the backward of `score_ids` with respect to the queries (`listed_scores` wires it); with `ids` and
        `exp(log_weight)` of `sample_posterior` it is the priority-sampling estimate of `posterior_mean`, with top-k ids and softmax
        weights the truncated posterior mean, with one-hot weights a row fetch in float32.

        `ids` as in `score_ids`; `weights`: float32 `[nq, m]` tensor / array, or a ragged list of lists (padded with 0).  A slot that
        `score_ids` scores -inf (empty, out of range, outside the query's `subset`) contributes nothing whatever its weight - NaN and inf
        included; a present slot with weight 0.0 is skipped as well (its row is not read).  All slots skipped: the zero row.  Duplicates
        add.  fp16 / bf16 stores sum the stored rows widened to float32, an `exact_f32` store its float32 rows.  One summation order per
        query, fixed by its own list and the width of the store: the bits of a row do not depend on the batch around it.
        Enqueued on the current stream; nothing to finish, and safe beside searches of this index that are in flight.
        An L2 index refuses (the library's message)."""
        if isinstance(ids, torch.Tensor):
            lst = ids.to(self.device, torch.int64).contiguous()
            if lst.ndim != 2:
                raise ValueError(f"expected ids of shape [nq, m], got {tuple(lst.shape)}")
        else:
            lst = torch.from_numpy(pad_listed_ids(ids)).to(self.device)
        nq, m = int(lst.shape[0]), int(lst.shape[1])
        if isinstance(weights, torch.Tensor):
            w = weights.to(self.device, torch.float32).contiguous()
            if tuple(w.shape) != (nq, m):
                raise ValueError(f"expected weights of shape {(nq, m)}, got {tuple(w.shape)}")
        else:
            w = torch.from_numpy(pad_listed_weights(weights, (nq, m))).to(self.device)
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        res = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device) if out is None else out
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_sum_ids(self._h, lst.data_ptr(), w.data_ptr(), nq, m, int(id_base),
                                                         None if sub is None else sub.data_ptr(), n_sub, res.data_ptr(),
                                                         _native.current_stream_ptr(self.device)))
        for t, given in ((lst, ids), (w, weights), (sub, subset)):  # (the rule of score_ids: copies this call made outlive the launch)
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return res

    def listed_scores(self, queries: torch.Tensor, ids, *, subset=None, id_base: int = 0) -> torch.Tensor:
        """`score_ids(queries, ids)` - the same bits, -inf at absent slots - as a float32 `[nq, m]` tensor that is differentiable (once)
        with respect to `queries`: backward is `sum_ids(ids, grad_out)`, cast to the dtype and device of `queries` (straight through the
        rounding of the queries to the store dtype, as `log_z`).  The gradient at absent slots vanishes by the presence rule of `sum_ids`,
        whatever arrives there (NaN included); no gradient flows to the store.  With `sample_posterior`:
        `s = index.sample_posterior(q, k, seed=...)`, `index.listed_scores(q, s.ids)` are the sampled scores as a function of `q`."""
        if not isinstance(ids, torch.Tensor):
            ids = torch.from_numpy(pad_listed_ids(ids, int(queries.shape[0]))).to(self.device)
        return _ListedScores.apply(queries, self, ids, {"subset": subset, "id_base": id_base})

    def _subset_labels(self, subset, nq: int):
        """`subset` -> (int32 device tensor `[nq, S]` or None, S)."""
        if subset is None:
            return None, 0
        sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
        sub = sub.to(self.device, torch.int32).contiguous()
        if sub.ndim != 2 or sub.shape[0] != nq:
            raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
        return sub, int(sub.shape[1])

    def rank_ids(self, queries, ids, *, subset=None, id_base: int = 0) -> "ListedRanks":
        """The exact rank of LISTED rows over the WHOLE store, however deep: `ListedRanks(rank, score)`, int64 / float32 device tensors
        `[nq, m]`.  `score[q, j]` is the scan's score of row `ids[q, j] - id_base` - the bits `search` returns for that pair - and
        `rank[q, j]` the 0-based position at which a search over the query's eligible rows returns it: the number of eligible rows
        with a larger score, or an equal score (`-0.0 == +0.0`) and a smaller id.  For every finite hit of `search(q, k)` at position
        `p`, `rank_ids(q, ids_of_search)[q, p]` is `(p, the same score bits)`.

        `ids` as in `score_ids` with `m <= 64`; a slot that `score_ids` calls absent (empty, out of range, outside the query's `subset`)
        gives `(-1, -inf)`, a NaN score rank -1 with the score as computed; duplicates are independent slots.  One scan of the store on
        the MFMA path with integer compares in place of the top-k (cost linear in `m`), no `[nq, N]` matrix.  Enqueued on the current
        stream; nothing to finish, and safe beside searches of this index that are in flight.  L2 and `exact_f32` indexes refuse."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        if isinstance(ids, torch.Tensor):
            lst = ids.to(self.device, torch.int64).contiguous()
            if lst.ndim != 2 or lst.shape[0] != nq:
                raise ValueError(f"expected ids of shape [{nq}, m], got {tuple(lst.shape)}")
        else:
            lst = torch.from_numpy(pad_listed_ids(ids, nq)).to(self.device)
        m = int(lst.shape[1])
        sub, n_sub = self._subset_labels(subset, nq)
        rank = torch.empty((nq, m), dtype=torch.int64, device=self.device)
        score = torch.empty((nq, m), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_rank_ids(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, lst.data_ptr(), m, int(id_base),
                None if sub is None else sub.data_ptr(), n_sub, rank.data_ptr(), score.data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (lst, ids), (sub, subset)):  # (the rule of score_ids: copies this call made outlive the launch)
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return ListedRanks(rank, score)

    def count_above(self, queries, thresholds, *, tie_ids=None, subset=None, id_base: int = 0) -> torch.Tensor:
        """How many eligible rows of the WHOLE store score above a threshold: int64 device tensor `[nq, m]`, entry `[q, j]` the number
        of rows `z` with `score(q, z) > thresholds[q, j]`, or - with `tie_ids` - with an equal score and `id_base + z < tie_ids[q, j]`
        (the order of `search`; `-0.0 == +0.0`).  It is the score CDF: choose `k`, size a candidate list, find a quantile.  A NaN
        threshold gives -1.  `count_above(q, score, tie_ids=ids)` is `rank_ids(q, ids).rank`.  `thresholds`: float32 `[nq, m]`,
        `m <= 64`; `tie_ids`: int64 of the same shape.  Eligibility, queries, `subset`, stream rules and refusals as `rank_ids`."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        thr = thresholds if isinstance(thresholds, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float32))
        thr = thr.to(self.device, torch.float32).contiguous()
        if thr.ndim != 2 or thr.shape[0] != nq:
            raise ValueError(f"expected thresholds of shape [{nq}, m], got {tuple(thr.shape)}")
        m = int(thr.shape[1])
        tie = None
        if tie_ids is not None:
            tie = tie_ids if isinstance(tie_ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tie_ids, dtype=np.int64))
            tie = tie.to(self.device, torch.int64).contiguous()
            if tuple(tie.shape) != (nq, m):
                raise ValueError(f"expected tie_ids of shape {(nq, m)}, got {tuple(tie.shape)}")
        sub, n_sub = self._subset_labels(subset, nq)
        out = torch.empty((nq, m), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_count_above(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, thr.data_ptr(), None if tie is None else tie.data_ptr(), m,
                int(id_base), None if sub is None else sub.data_ptr(), n_sub, out.data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (thr, thresholds), (tie, tie_ids), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return out

    def range_search(self, queries, thresholds, *, tie_ids=None, inclusive: bool = False, subset=None, id_base: int = 0,
                     max_results: int | None = None, order: str = "id") -> "RangeResult":
        """WHICH eligible rows of the WHOLE store score above a per-query threshold - the rows `count_above` counts - as CSR:
        `RangeResult(lims, scores, ids)`, device tensors int64 `[nq + 1]`, float32 `[total]` (the scan's bits, which are the bits
        `search` returns) and int64 `[total]`; query `q` owns positions `lims[q] .. lims[q + 1]`.  Row `z` is in the list of `q` when
        `score(q, z) > thresholds[q]`, or - with `tie_ids` - the score is equal (`-0.0 == +0.0`) and `id_base + z < tie_ids[q]`: with a
        hit `(s, i)` of `search` as threshold and tie id, exactly the hits a search returns ahead of it.  `inclusive=True` (without
        `tie_ids`) also takes the rows that equal the threshold.  A NaN threshold gives an empty list, `-inf` every eligible row above
        `-inf`.  Within a query ids ascend (`order="id"`), or `order="score"` re-sorts every list by (score descending, id ascending)
        on the device.  The result depends on the store and the query alone: the same bytes in any batch and on every repeat.

        `thresholds`: float32 `[nq]`; `tie_ids`: int64 `[nq]`.  With `max_results` the outputs are allocated up front and ONE native
        call runs (count scan + emit scan); more hits than that raise, with the needed size in the message.  Without it a sizing call
        (one scan) runs first, `lims[-1]` is read back, and the full call follows.  Eligibility, queries, `subset`, and refusals as
        `rank_ids`; the call that emits waits for the current stream (it reports overflow), the sizing call does not."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        thr = thresholds if isinstance(thresholds, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(thresholds, dtype=np.float32))
        thr = thr.to(self.device, torch.float32).contiguous()
        tie = None
        if tie_ids is not None:
            tie = tie_ids if isinstance(tie_ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tie_ids, dtype=np.int64))
            tie = tie.to(self.device, torch.int64).contiguous()
        check_range_args(nq, tuple(thr.shape), None if tie is None else tuple(tie.shape), inclusive, max_results, order)
        if inclusive:  # a tie row past every row
            tie = torch.full((nq,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=self.device)
        sub, n_sub = self._subset_labels(subset, nq)
        lims = torch.empty((nq + 1,), dtype=torch.int64, device=self.device)

        def call(scores, ids, capacity):
            with torch.cuda.device(self.device):
                _native.check(self._lib.vodhip_index_range_search(
                    self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, thr.data_ptr(), None if tie is None else tie.data_ptr(),
                    int(id_base), None if sub is None else sub.data_ptr(), n_sub, lims.data_ptr(), None if scores is None else scores.data_ptr(),
                    None if ids is None else ids.data_ptr(), int(capacity), _native.current_stream_ptr(self.device)))

        if max_results is None:
            call(None, None, 0)
            capacity = int(lims[-1])
        else:
            capacity = int(max_results)
        scores = torch.empty((max(capacity, 1),), dtype=torch.float32, device=self.device)  # (never a NULL pointer: that is the sizing call)
        ids = torch.empty((max(capacity, 1),), dtype=torch.int64, device=self.device)
        try:
            call(scores, ids, capacity)
        except _native.NativeLibraryError as exc:
            if self.get_stat("last_range_overflow") > 0:
                raise _native.NativeLibraryError(f"{exc}: call range_search with max_results >= {int(lims[-1])}") from None
            raise
        finally:
            for t, given in ((q, queries), (thr, thresholds), (tie, tie_ids), (sub, subset)):
                if t is not None and t is not given:
                    t.record_stream(torch.cuda.current_stream(self.device))
        total = capacity if max_results is None else int(lims[-1])
        res = RangeResult(lims, scores[:total], ids[:total])
        return sort_range_by_score(res) if order == "score" else res

    def outranking(self, queries, ids, *, subset=None, id_base: int = 0, order: str = "score") -> "RangeResult":
        """Per query, the rows a search returns AHEAD of row `ids[q]` (int64 `[nq]`, one id per query), however deep it sits: `rank_ids`
        gives the target's scan score, `range_search` with `(score, id)` as threshold and tie id the rows - as many as the target's
        rank, in search order (`order="score"`) or by ascending id.  A target that is absent (out of range, outside `subset`) or scores
        NaN gives an empty list."""
        tgt = ids if isinstance(ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64))
        tgt = tgt.to(self.device, torch.int64).reshape(-1).contiguous()
        ranks = self.rank_ids(queries, tgt[:, None], subset=subset, id_base=id_base)
        thr = torch.where(ranks.rank[:, 0] >= 0, ranks.score[:, 0], torch.full_like(ranks.score[:, 0], float("nan")))
        return self.range_search(queries, thr, tie_ids=tgt, subset=subset, id_base=id_base, order=order)

    def posterior_support(self, queries, min_prob: float, temperature: float = 1.0, subset=None) -> "PosteriorSupport":
        """The exact support of the posterior above a probability floor: every eligible row with `p(z | q) > min_prob`, an adaptive K in
        place of a fixed top-K.  One `log_partition`, then `range_search(q, thr)` with
        `thr = float32(temperature * (log_z + log(min_prob)))`, computed in double from the returned `max_score` and `log_rel`.
        MEMBERSHIP IS DEFINED BY THAT ROUNDED THRESHOLD: a row is returned when its scan score is above `thr` as a float32, which can
        differ from the real-valued test `p > min_prob` for a row within a rounding of the boundary.  Returns `PosteriorSupport(lims,
        scores, ids, log_p, log_partition)`, `log_p = score / temperature - log_z` per hit (float32, computed in double)."""
        if not 0.0 < float(min_prob) <= 1.0:
            raise ValueError(f"min_prob must be in (0, 1], got {min_prob}")
        t = float(temperature)
        lp = self.log_partition(queries, temperature=t, subset=subset)
        log_z = lp.max_score.double() / t + lp.log_rel.double()
        thr = (t * (log_z + math.log(float(min_prob)))).float()
        res = self.range_search(queries, thr, subset=subset)
        seg = torch.repeat_interleave(torch.arange(thr.shape[0], device=self.device), res.lims[1:] - res.lims[:-1])
        log_p = (res.scores.double() / t - log_z[seg]).float()
        return PosteriorSupport(res.lims, res.scores, res.ids, log_p, lp)

    def log_partition(self, queries, temperature: float = 1.0, subset=None, out=None) -> LogPartition:
        """The exact softmax normaliser over the WHOLE store, `log Z(q) = log sum_z exp(<q~, x~_z> / temperature)`, from one scan on
        the MFMA path (no `[nq, N]` score matrix): `LogPartition(log_z, max_score, log_rel)`, float32 device tensors `[nq]` with
        `log_z = max_score / temperature + log_rel`.  `max_score` is the bits `search(q, 1)` returns; `log_rel >= 0` carries what the
        float32 spacing at `max_score / temperature` would swallow.  No eligible row: all three -inf.

        `queries` as in `search`, `subset` as in `score_ids` (an argument, not index state).  `out`: a (max_score, log_rel) pair to
        write into.  Enqueued on the current stream; nothing to finish, and safe beside searches of this index that are in flight.
        L2 and `exact_f32` indexes refuse (the library's message)."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        if out is None:
            max_score = torch.empty((nq,), dtype=torch.float32, device=self.device)
            log_rel = torch.empty((nq,), dtype=torch.float32, device=self.device)
        else:
            max_score, log_rel = out
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_log_partition(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, beta, None if sub is None else sub.data_ptr(), n_sub,
                max_score.data_ptr(), log_rel.data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return LogPartition(max_score * beta + log_rel, max_score, log_rel)  # (-inf + -inf and +inf + +inf: never NaN)

    def posterior_stats(self, queries, temperature: float = 1.0, subset=None, out=None) -> "PosteriorStats":
        """The entropy and the score moments of the posterior over the WHOLE store, `p(z | q) = exp(<q~, x~_z> / temperature - log Z(q))`,
        from ONE scan (the `log_partition` scan with two more accumulators; no `[nq, N]` matrix):
        `PosteriorStats(entropy, mean_score, var_score, mean_rel, log_partition)`, float32 device tensors `[nq]`.
        `mean_score = E_p[s] = d log Z / d beta` (`beta = 1 / temperature`), `var_score = Var_p[s] = d^2 log Z / d beta^2`,
        `mean_rel = mean_score - max_score <= 0` (what the library returns: it keeps the digits that adding `max_score` rounds away),
        `entropy = log_rel - beta * mean_rel` in nats, two non-negative terms; `log_partition` is the `LogPartition` that
        `log_partition` returns for the same call, bit for bit.  A query's words are the same bits whatever the batch around it.
        No eligible row, or a +inf score: `log_partition` as `log_partition` gives it, the statistics NaN.

        Arguments, stream behaviour and refusals as `log_partition`; `out`: a (max_score, log_rel, mean_rel, var_score) 4-tuple to
        write into."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = self._subset_labels(subset, nq)
        if out is None:
            max_score, log_rel, mean_rel, var = (torch.empty((nq,), dtype=torch.float32, device=self.device) for _ in range(4))
        else:
            max_score, log_rel, mean_rel, var = out
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_posterior_stats(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, beta, None if sub is None else sub.data_ptr(), n_sub,
                max_score.data_ptr(), log_rel.data_ptr(), mean_rel.data_ptr(), var.data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return PosteriorStats(log_rel - beta * mean_rel, max_score + mean_rel, var, mean_rel,
                              LogPartition(max_score * beta + log_rel, max_score, log_rel))

    def posterior_divergence(self, queries_a, queries_b, temperature_a: float = 1.0, temperature_b: float | None = None, subset=None,
                             out=None) -> "PosteriorDivergence":
        """The exact divergences between TWO posteriors over the WHOLE store from ONE scan: pair `i` is `(queries_a[i], queries_b[i])`,
        `p = softmax(<a~, x~_z> / temperature_a)` and `r = softmax(<b~, x~_z> / temperature_b)` over the rows eligible for the pair
        (`temperature_b=None`: as a) - a teacher against a student, the last period's retriever against the current one, one query at two
        temperatures.  `PosteriorDivergence(kl_ab, kl_ba, cross_entropy_ab, cross_entropy_ba, entropy_a, entropy_b, cross_rel_ab,
        cross_rel_ba, stats_a, stats_b)`, float32 device tensors `[nq]`: `kl_ab = KL(p || r)`, `cross_entropy_ab = H(p, r)`,
        `cross_rel_ab = E_p[s_b] - max_b <= 0` (what the library returns), `stats_a` / `stats_b` the `DivergenceSide(max_score, log_rel,
        mean_rel, log_partition)` of each side - the bits `posterior_stats` returns for that side alone unless a row scores NaN
        against exactly one side.  The derived words are formed in float64 from the eight float32 words and rounded once; an identical
        pair returns `kl == 0.0` exactly.  A pair's words are the same bits whatever the batch around it.
        A row with `p > 0` that side b scores -inf: `cross_entropy_ab = kl_ab = +inf`.  A side with no eligible row or a +inf score:
        its `mean_rel` and both cross words (hence every divergence) are NaN.

        Arguments, stream behaviour and refusals as `posterior_stats`; one `subset` row per pair; `out`: the eight library words
        (max_a, log_rel_a, mean_rel_a, cross_rel_ab, max_b, log_rel_b, mean_rel_b, cross_rel_ba) to write into."""
        qa = self._prep_queries(queries_a)
        qb = self._prep_queries(queries_b)
        if qb.dtype != qa.dtype:  # (one q_dtype per call: float32 holds every input dtype)
            qa, qb = qa.float(), qb.float()
        nq = qa.shape[0]
        if qb.shape[0] != nq:
            raise ValueError(f"expected {nq} queries on each side, got {qb.shape[0]} for b")
        beta_a = 1.0 / float(temperature_a) if temperature_a else float("nan")
        beta_b = beta_a if temperature_b is None else (1.0 / float(temperature_b) if temperature_b else float("nan"))
        sub, n_sub = self._subset_labels(subset, nq)
        words = tuple(torch.empty((nq,), dtype=torch.float32, device=self.device) for _ in range(8)) if out is None else tuple(out)
        if len(words) != 8:
            raise ValueError(f"expected an 8-tuple of outputs, got {len(words)}")
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_posterior_divergence(
                self._h, qa.data_ptr(), qb.data_ptr(), _native.torch_dtype_code(qa.dtype), nq, beta_a, beta_b,
                None if sub is None else sub.data_ptr(), n_sub, *[w.data_ptr() for w in words], _native.current_stream_ptr(self.device)))
        for t, given in ((qa, queries_a), (qb, queries_b), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return posterior_divergence_words(words, beta_a, beta_b)

    def kl_to(self, teacher_queries, student_queries: torch.Tensor, temperature: float = 1.0, temperature_teacher: float | None = None,
              subset=None) -> torch.Tensor:
        """`KL(p_teacher || p_student)` over the whole store as a float32 `[nq]` tensor that is differentiable with respect to
        `student_queries` only (the teacher is a constant): forward is `posterior_divergence(teacher, student).kl_ab`, backward
        `grad_student = grad_out[:, None] * (posterior_mean(student) - posterior_mean(teacher)) / temperature`, cast to the student's
        dtype; rows whose KL is not finite get zero.  `temperature` is the student's, `temperature_teacher=None` means the same.  The
        two `posterior_mean` calls run in forward, and only when the student requires grad."""
        t_teacher = float(temperature) if temperature_teacher is None else float(temperature_teacher)
        teacher = teacher_queries.detach() if isinstance(teacher_queries, torch.Tensor) else teacher_queries
        return _KlTo.apply(student_queries, self, teacher, float(temperature), t_teacher, subset)

    def posterior_mean(self, queries, temperature: float = 1.0, subset=None, out=None) -> "PosteriorMean":
        """The posterior mean of the stored rows under the softmax over the WHOLE store, `mean[q] = sum_z p(z | q) x~_z` with
        `p(z | q) = exp(<q~, x~_z> / temperature - log Z(q))`: `PosteriorMean(mean, log_partition)`, `mean` a float32 device tensor
        `[nq, dim]`, `log_partition` the `LogPartition` that `log_partition` returns for the same call, bit for bit.  `mean / temperature`
        is the gradient of `log Z` with respect to the query (`log_z` wraps it for autograd).  Two scans on the MFMA path, no `[nq, N]`
        matrix; a `mean` row is the same bits whatever the batch around it.  A query with no eligible row (or a +inf score) gets the zero
        row.  A stored NaN / infinity in column d makes column d of every mean NaN (the library's contract, `vodhip.h` H2m).

        Arguments as `log_partition`; `out`: a (max_score, log_rel, mean) triple to write into."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        if out is None:
            max_score = torch.empty((nq,), dtype=torch.float32, device=self.device)
            log_rel = torch.empty((nq,), dtype=torch.float32, device=self.device)
            mean = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device)
        else:
            max_score, log_rel, mean = out
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_posterior_mean(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, beta, None if sub is None else sub.data_ptr(), n_sub,
                max_score.data_ptr(), log_rel.data_ptr(), mean.data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return PosteriorMean(mean, LogPartition(max_score * beta + log_rel, max_score, log_rel))

    def posterior_expectation(self, queries, temperature: float = 1.0, subset=None, out=None) -> "PosteriorExpectation":
        """The posterior expectation of the value table (`set_row_values`) under the softmax over the WHOLE store, `values[q] =
        sum_z p(z | q) v~_z` with `p(z | q) = exp(<q~, x~_z> / temperature - log Z(q))`: `PosteriorExpectation(values, log_partition)`,
        `values` a float32 device tensor `[nq, n_cols]`, `log_partition` the `LogPartition` that `log_partition` returns for the same
        call, bit for bit.  Exact attention with the store as keys and the table as values: a one-hot table gives the posterior mass per
        class, a score table the expected score, a projected copy of the rows a posterior mean in that space.  ONE scan on the MFMA path
        (running maximum with rescaling), no `[nq, N]` matrix; a `values` row is the same bits whatever the batch around it.  A query with
        no eligible row (or a +inf score) gets the zero row.  A NaN / infinity in column c of the table makes column c of every query NaN
        (the library's contract, `vodhip.h` H2e).  Forward only: `expected_values` is the same read-out with its gradient in the query.

        Arguments as `log_partition`; `out`: a (max_score, log_rel, values) triple to write into."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        shape = self.row_values_shape
        n_cols = shape[1] if shape else 0
        if out is None:
            max_score = torch.empty((nq,), dtype=torch.float32, device=self.device)
            log_rel = torch.empty((nq,), dtype=torch.float32, device=self.device)
            values = torch.empty((nq, n_cols), dtype=torch.float32, device=self.device)
        else:
            max_score, log_rel, values = out
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_posterior_expectation(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, beta, None if sub is None else sub.data_ptr(), n_sub,
                max_score.data_ptr(), log_rel.data_ptr(), (values if values.numel() else max_score.new_empty(1)).data_ptr(),
                _native.current_stream_ptr(self.device)))  # (no table: a non-NULL pointer, so that the library's own refusal names it)
        for t, given in ((q, queries), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return PosteriorExpectation(values, LogPartition(max_score * beta + log_rel, max_score, log_rel))

    def posterior_expectation_backward(self, queries, grad_values, expectation: "PosteriorExpectation", temperature: float = 1.0,
                                       subset=None, out=None) -> torch.Tensor:
        """The gradient of `posterior_expectation` in the queries: with `y = expectation.values` and `g = grad_values = dL / dy`,
        `grad[q] = sum_z p(z | q) (u_z - ubar_q) x~_z / temperature`, `u_z = <g[q], v~_z>`, `ubar_q = <g[q], y[q]>` - a float32 device
        tensor `[nq, dim]`.  `expectation` is what `posterior_expectation` returned for the same queries, temperature and subset: its
        `values`, `max_score` and `log_rel` are inputs, so ONE scan of the store runs and no partition scan in front.  Exact over every
        stored row, no `[nq, N]` matrix; a row is the same bits whatever the batch around it; scaling a row of `g` by a power of two
        scales the result by exactly that power (each row is normalised before it is rounded to the store dtype, so small loss gradients
        do not flush in fp16).  A query with no eligible row (or a +inf score) and an all-zero `g` row give the zero row; a NaN or an
        infinity in `g[q]` makes row `q` NaN (the library's contract, `vodhip.h` H2b).  The first call after `set_row_values` computes
        the table's column maxima and waits for the stream once.

        Other arguments as `posterior_expectation`; `out`: a float32 `[nq, dim]` device tensor to write into."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        y = torch.as_tensor(expectation.values).to(self.device, torch.float32).contiguous()
        g = torch.as_tensor(grad_values).to(self.device, torch.float32).contiguous()
        if y.ndim != 2 or y.shape[0] != nq or g.shape != y.shape:
            raise ValueError(f"expected values and grad_values of one shape [{nq}, n_cols], got {tuple(y.shape)} and {tuple(g.shape)}")
        shape = self.row_values_shape
        if shape is not None and y.shape[1] != shape[1]:
            raise ValueError(f"expected grad_values of shape [{nq}, {shape[1]}] (the table's columns), got {tuple(g.shape)}")
        max_score = torch.as_tensor(expectation.log_partition.max_score).to(self.device, torch.float32).contiguous()
        log_rel = torch.as_tensor(expectation.log_partition.log_rel).to(self.device, torch.float32).contiguous()
        if max_score.shape != (nq,) or log_rel.shape != (nq,):
            raise ValueError(f"expected max_score and log_rel of shape ({nq},)")
        grad = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device) if out is None else out
        spare = max_score.new_empty(1)  # (no table: non-NULL pointers, so that the library's own refusal names it)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_posterior_expectation_backward(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, beta, None if sub is None else sub.data_ptr(), n_sub,
                max_score.data_ptr(), log_rel.data_ptr(), (y if y.numel() else spare).data_ptr(), (g if g.numel() else spare).data_ptr(),
                grad.data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (sub, subset), (y, expectation.values), (g, grad_values), (max_score, expectation.log_partition.max_score),
                         (log_rel, expectation.log_partition.log_rel)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return grad

    def expected_values(self, queries: torch.Tensor, temperature: float = 1.0, subset=None) -> torch.Tensor:
        """`posterior_expectation(queries).values` as a float32 `[nq, n_cols]` tensor that is differentiable with respect to `queries`:
        forward is the unchanged `posterior_expectation`, backward `posterior_expectation_backward` - one more scan of the store - cast
        to the dtype of `queries` (straight through the rounding of the queries to the store dtype).  No gradient flows to the table,
        the store or the temperature; not twice differentiable.  A cross-entropy on class masses: with a one-hot class table,
        `-torch.log(index.expected_values(q, T)[torch.arange(nq), labels]).mean()`."""
        return _ExpectedValues.apply(queries, self, float(temperature), subset)

    def posterior_adjoint(self, queries, weights, log_partition: "LogPartition | None" = None, temperature: float = 1.0, subset=None,
                          out=None, accumulate: bool = False) -> torch.Tensor:
        """The adjoint of the read-out, its gradient in the value table: `out[z, c] = sum_q p(z | q) weights[q, c]` with
        `p(z | q) = exp(<q~, x~_z> / temperature - log Z(q))` - `P^T W`, a float32 device tensor `[ntotal, n_cols]`; it reduces over the
        QUERIES per stored row.  `weights` is `[nq, n_cols]` (a vector is one column), 1 <= n_cols <= 256: with `weights = dL / dy` the
        result is `dL / dV` of `y = posterior_expectation(...)`.  The call reads no value table.  `log_partition` is the `LogPartition` of
        any forward call with the same queries, temperature and subset (its `max_score` and `log_rel` are inputs: ONE scan of the store);
        with None the method runs `log_partition` first, two scans in all.  Exact over every stored row, no `[nq, N]` matrix; every row
        has one owning workgroup that adds the queries in batch order: no atomics, the same bits on every repeat.  Each column of
        `weights` is normalised by its power of two before it is rounded to the store dtype (1e-6 loss gradients do not flush in fp16);
        scaling a column by a power of two scales the output column by exactly that power.  A query with no eligible row (or a +inf
        score) contributes nothing; a NaN or an infinity in column c of `weights` makes column c of every row NaN (`vodhip.h` H2a).

        `out`: a float32 `[ntotal, n_cols]` device tensor to write into; `accumulate=True` adds to what it holds.  Other arguments as
        `log_partition`.  L2 and `exact_f32` indexes refuse (the library's message)."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        w_given = torch.as_tensor(weights)
        w = w_given.detach().to(self.device, torch.float32)
        w = (w.reshape(-1, 1) if w.ndim == 1 else w).contiguous()
        if w.ndim != 2 or w.shape[0] != nq:
            raise ValueError(f"expected weights of shape [{nq}, n_cols], got {tuple(w_given.shape)}")
        n_cols = int(w.shape[1])
        if log_partition is None:
            log_partition = self.log_partition(q, temperature, sub)
        max_score = torch.as_tensor(log_partition.max_score).to(self.device, torch.float32).contiguous()
        log_rel = torch.as_tensor(log_partition.log_rel).to(self.device, torch.float32).contiguous()
        if max_score.shape != (nq,) or log_rel.shape != (nq,):
            raise ValueError(f"expected max_score and log_rel of shape ({nq},)")
        ntotal = self.ntotal
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs `out`")
            out = torch.empty((ntotal, n_cols), dtype=torch.float32, device=self.device)
        elif out.shape != (ntotal, n_cols) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"expected `out` a contiguous float32 [{ntotal}, {n_cols}] tensor on {self.device}")
        spare = max_score.new_empty(1)  # (nothing to read or write: non-NULL pointers, so that the library's own refusals are the ones reported)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_posterior_adjoint(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, beta, None if sub is None else sub.data_ptr(), n_sub,
                max_score.data_ptr(), log_rel.data_ptr(), (w if w.numel() else spare).data_ptr(), n_cols, 1 if accumulate else 0,
                (out if out.numel() else spare).data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (sub, subset), (w, weights), (max_score, log_partition.max_score), (log_rel, log_partition.log_rel)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return out

    def row_mass(self, queries, temperature: float = 1.0, query_weights=None, subset=None, log_partition: "LogPartition | None" = None) -> torch.Tensor:
        """The exact posterior mass every stored row receives from a query set, `mass[z] = sum_q query_weights[q] p(z | q)`
        (`query_weights` ones by default): a float32 device tensor `[ntotal]`, `posterior_adjoint` of one column.  It sums to the number
        (the weight) of the queries that have an eligible row; a truncated top-k cannot give it: which rows a training set ever looks at,
        which are hubs, which are dead."""
        q = self._prep_queries(queries)
        w = torch.ones((q.shape[0],), dtype=torch.float32, device=self.device) if query_weights is None else torch.as_tensor(query_weights).reshape(-1)
        return self.posterior_adjoint(q, w, log_partition, temperature, subset).reshape(-1)

    def read_out(self, queries: torch.Tensor, values: torch.Tensor, temperature: float = 1.0, subset=None, keys=None) -> torch.Tensor:
        """`set_row_values(values)` followed by the read-out `y = P V~`, a float32 `[nq, n_cols]` tensor differentiable (once) in
        `queries` AND in `values`: exact attention over the store with a trainable value table.  The gradient in the queries is
        `posterior_expectation_backward` (cast to their dtype), the gradient in the values `posterior_adjoint(queries, grad_out, the
        forward's words)` cast to the dtype and device of `values` - straight through the table's rounding to the store dtype.  Each
        costs one more scan of the store and runs only when that input requires a gradient.  The index keeps the table afterwards.

        `keys`: a float tensor `[ntotal, dim]`, e.g. `index.stored_rows().float().requires_grad_()`, of which the caller states that it is
        the store.  It is not read: its only role is to receive `key_gradient(queries, grad_values=grad_out, the forward's words)`,
        cast to its dtype and device, when it requires a gradient - straight through the rounding of the rows at ingest.  Without
        `keys` the call is exactly what it was."""
        if keys is None:
            return _ReadOut.apply(queries, values, self, float(temperature), subset)
        return _ReadOutKeys.apply(queries, values, _checked_keys(self, keys), self, float(temperature), subset)

    def key_gradient(self, queries, *, grad_log_z=None, grad_values=None, expectation: "PosteriorExpectation | None" = None,
                     log_partition: "LogPartition | None" = None, temperature: float = 1.0, subset=None, out=None,
                     accumulate: bool = False) -> torch.Tensor:
        """The posterior's exact gradient in the STORED ROWS: `out[z, d] = sum_q p(z | q) c_qz q~[q, d] / temperature` with
        `c_qz = a_q + (u_qz - ubar_q)`, `a = grad_log_z` (`[nq]`), `u_qz = <G[q], v~_z>`, `ubar_q = <G[q], y[q]>`, `G = grad_values`
        (`[nq, n_cols]`, acting on the attached value table) - a float32 device tensor `[ntotal, dim]`, up to rounding the gradient of
        `sum_q a_q log Z_q + sum_qc G_qc y_qc` in the rows as stored.  At least one of the two gradients; an absent one counts as zero
        (and without `grad_values` no table is needed).  `expectation` (what `posterior_expectation` returned for the same queries,
        temperature and subset; needed values with `grad_values`) or `log_partition` hand in the forward's words: ONE scan of the
        store; with neither the forward runs first.  Every row has one owning workgroup that adds the queries in batch order: no
        atomics, the same bits on every repeat.  The gradients are normalised by ONE power of two per batch (not per query: the
        contraction runs over the queries), so on an fp16 store a query whose gradient is far below the batch's largest loses
        relative, not absolute, precision.  A query with no eligible row contributes nothing; a NaN or an infinity in `a[q]` or
        `G[q]` makes the whole result NaN (`vodhip.h` H2k).

        `out`: a float32 `[ntotal, dim]` device tensor to write into; `accumulate=True` adds to what it holds.  Other arguments as
        `log_partition`.  L2 and `exact_f32` indexes refuse (the library's message)."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        a = g = y = None
        if grad_log_z is not None:
            a = torch.as_tensor(grad_log_z).detach().to(self.device, torch.float32).reshape(-1).contiguous()
            if a.shape != (nq,):
                raise ValueError(f"expected grad_log_z of shape ({nq},), got {tuple(torch.as_tensor(grad_log_z).shape)}")
        if grad_values is not None:
            g = torch.as_tensor(grad_values).detach().to(self.device, torch.float32).contiguous()
            if expectation is None and self.row_values_shape is not None:
                expectation = self.posterior_expectation(q, temperature, sub)
            if expectation is not None:
                y = torch.as_tensor(expectation.values).to(self.device, torch.float32).contiguous()
                if y.ndim != 2 or y.shape[0] != nq or g.shape != y.shape:
                    raise ValueError(f"expected values and grad_values of one shape [{nq}, n_cols], got {tuple(y.shape)} and {tuple(g.shape)}")
            shape = self.row_values_shape
            if shape is not None and (g.ndim != 2 or g.shape[1] != shape[1]):
                raise ValueError(f"expected grad_values of shape [{nq}, {shape[1]}] (the table's columns), got {tuple(g.shape)}")
        if expectation is not None and log_partition is None:
            log_partition = expectation.log_partition
        if log_partition is None:
            log_partition = self.log_partition(q, temperature, sub)
        max_score = torch.as_tensor(log_partition.max_score).to(self.device, torch.float32).contiguous()
        log_rel = torch.as_tensor(log_partition.log_rel).to(self.device, torch.float32).contiguous()
        if max_score.shape != (nq,) or log_rel.shape != (nq,):
            raise ValueError(f"expected max_score and log_rel of shape ({nq},)")
        ntotal = self.ntotal
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs `out`")
            out = torch.empty((ntotal, self.dim), dtype=torch.float32, device=self.device)
        elif out.shape != (ntotal, self.dim) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"expected `out` a contiguous float32 [{ntotal}, {self.dim}] tensor on {self.device}")
        spare = max_score.new_empty(1)  # (nothing to read or write: non-NULL pointers, so that the library's own refusals are the ones reported)

        def ptr(t):
            return None if t is None else (t if t.numel() else spare).data_ptr()

        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_posterior_key_gradient(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, beta, None if sub is None else sub.data_ptr(), n_sub,
                max_score.data_ptr(), log_rel.data_ptr(), ptr(a), ptr(g if y is None else y), ptr(g), 1 if accumulate else 0,
                (out if out.numel() else spare).data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (sub, subset), (a, grad_log_z), (g, grad_values), (y, None), (max_score, log_partition.max_score),
                         (log_rel, log_partition.log_rel)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        return out

    def sample_posterior(self, queries, k: int, temperature: float = 1.0, *, seed: int, query_offset: int = 0, subset=None,
                         id_base: int = 0, out=None) -> "PosteriorSample":
        """`k` rows drawn WITHOUT replacement from the softmax over the WHOLE store, `p(z | q) = exp(<q~, x~_z> / temperature - log Z(q))`,
        with their priority-sampling weights: `PosteriorSample(ids, scores, log_p, log_weight, log_tau, keys, log_partition)`.  `ids`
        int64 `[nq, k]` (pads -1), `scores` / `log_p` / `log_weight` float32 `[nq, k]` (pads -inf), `keys` float32 `[nq, k + 1]` the
        unnormalised Gumbel keys `score / temperature - log E` in descending order (pads -inf), `log_tau` `[nq]` the (k+1)-th key minus
        `log Z` (-inf when every eligible row was returned), `log_partition` the `LogPartition` that `log_partition` returns for the same
        call, bit for bit.  `sum_j exp(log_weight[q, j]) f(ids[q, j])` is an unbiased estimate of `E_{p(. | q)}[f]`; with
        `log_tau = -inf` the weights are the probabilities themselves.  Exact over every stored row (no top-K proposal, no `[nq, N]`
        matrix): three scans on the MFMA path, `1 <= k <= 255`.

        The noise is counter-based (Philox4x32-10): the draw of row `id_base + z` for query `query_offset + i` depends on `seed`, that
        row id and that query index alone, so a query's result is the same bits alone, inside any batch (give it its `query_offset`),
        on every repeat, and over shards that pass their own `id_base`.  A query with no eligible row (or a +inf score) is all pads.
        The call waits for the current stream before it returns (it reads its overflow word).

        Arguments as `log_partition`; `out`: a (max_score, log_rel, ids, scores, log_p, log_weight, keys) tuple to write into."""
        q = self._prep_queries(queries)
        nq = q.shape[0]
        k = int(k)
        if not 1 <= k <= 255:
            raise ValueError(f"k must be in [1, 255], got {k}")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be in [0, 2^64), got {seed}")
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))
            sub = sub.to(self.device, torch.int32).contiguous()
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"expected subset labels of shape [{nq}, S], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        if out is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            max_score, log_rel = torch.empty((nq,), **f32), torch.empty((nq,), **f32)
            ids = torch.empty((nq, k), dtype=torch.int64, device=self.device)
            scores, log_p, log_weight = torch.empty((nq, k), **f32), torch.empty((nq, k), **f32), torch.empty((nq, k), **f32)
            keys = torch.empty((nq, k + 1), **f32)
        else:
            max_score, log_rel, ids, scores, log_p, log_weight, keys = out
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_index_sample_posterior(
                self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), nq, k, beta, int(seed), int(query_offset), int(id_base),
                None if sub is None else sub.data_ptr(), n_sub, max_score.data_ptr(), log_rel.data_ptr(), ids.data_ptr(), scores.data_ptr(),
                log_p.data_ptr(), log_weight.data_ptr(), keys.data_ptr(), _native.current_stream_ptr(self.device)))
        for t, given in ((q, queries), (sub, subset)):
            if t is not None and t is not given:
                t.record_stream(torch.cuda.current_stream(self.device))
        log_tau = (keys[:, k] - max_score * beta) - log_rel  # (a pad key -inf stays -inf; a query without a finite log Z: NaN -> -inf)
        log_tau = torch.where(torch.isnan(log_tau), torch.full_like(log_tau, float("-inf")), log_tau)
        return PosteriorSample(ids, scores, log_p, log_weight, log_tau, keys, LogPartition(max_score * beta + log_rel, max_score, log_rel))

    def log_z(self, queries: torch.Tensor, temperature=1.0, subset=None, keys=None) -> torch.Tensor:
        """`log Z(q)` over the whole store as a float32 `[nq]` tensor that is differentiable with respect to `queries`: forward is
        `posterior_mean`, backward `grad_q = grad_out[:, None] * mean / temperature`, cast to the dtype of `queries` (straight through
        the rounding of the queries to the store dtype).  No gradient flows to the store; rows of `grad_q` whose `log_z` is not finite
        are zero.  The exact retrieval NLL of a positive row: `-(<q, x_pos> / T - index.log_z(q, T))`.

        `temperature` may be a one-element tensor (a learnable scale): reading its value is ONE host synchronisation.  If it requires
        grad, `grad_T = -sum_q grad_out[q] * mean_score[q] / T^2` with `mean_score` of `posterior_stats` (queries whose `log_z` is not
        finite contribute 0).  With a tensor temperature `posterior_mean` runs only when `queries` requires grad: temperature-only
        calibration costs about one `log_partition`.  With a float temperature nothing changes.

        `keys`: a float tensor `[ntotal, dim]`, e.g. `index.stored_rows().float().requires_grad_()`, of which the caller states that it is
        the store.  It is not read: its only role is to receive `key_gradient(queries, grad_log_z=grad_out, the forward's words)`,
        cast to its dtype and device, when it requires a gradient.  Not together with a tensor temperature (ValueError).  Without
        `keys` the call is exactly what it was."""
        if keys is not None:
            if isinstance(temperature, torch.Tensor):
                raise ValueError("log_z: `keys` together with a tensor temperature is not supported; pass a float temperature")
            return _LogZKeys.apply(queries, _checked_keys(self, keys), self, float(temperature), subset)
        if isinstance(temperature, torch.Tensor):
            return _LogZ.apply(queries, self, temperature, subset)
        return _LogZ.apply(queries, self, float(temperature), subset)


class LogPartition(NamedTuple):
    """`log_z = max_score / temperature + log_rel` of `HipFlatIndex.log_partition` / `HipNodeIndex.log_partition`, each `[nq]`."""

    log_z: Any
    max_score: Any
    log_rel: Any


class ListedRanks(NamedTuple):
    """`rank` (int64, -1 = absent or NaN) and `score` (float32, the scan's bits; -inf = absent) of `rank_ids`, each `[nq, m]`."""

    rank: Any
    score: Any


class RangeResult(NamedTuple):
    """The CSR result of `range_search`: `lims` int64 `[nq + 1]`, and at positions `lims[q] .. lims[q + 1]` of `scores` (float32, the
    scan's bits) and `ids` (int64) the hits of query `q`."""

    lims: Any
    scores: Any
    ids: Any


class PosteriorSupport(NamedTuple):
    """`posterior_support`: the `RangeResult` fields, `log_p = score / temperature - log_z` per hit and the `LogPartition` of the call."""

    lims: Any
    scores: Any
    ids: Any
    log_p: Any
    log_partition: LogPartition


def check_range_args(nq: int, thr_shape: tuple, tie_shape: tuple | None, inclusive: bool, max_results: int | None, order: str) -> None:
    """The refusals of `range_search` that need no index: one threshold (and tie id) per query, `order`, `max_results`."""
    if thr_shape != (nq,):
        raise ValueError(f"expected thresholds of shape ({nq},), got {thr_shape}")
    if tie_shape is not None and tie_shape != (nq,):
        raise ValueError(f"expected tie_ids of shape ({nq},), got {tie_shape}")
    if inclusive and tie_shape is not None:
        raise ValueError("inclusive=True is a tie id past every row: it cannot be combined with tie_ids")
    if order not in ("id", "score"):
        raise ValueError(f"order must be 'id' or 'score', got {order!r}")
    if max_results is not None and int(max_results) < 0:
        raise ValueError(f"max_results must be >= 0, got {max_results}")


def sort_range_by_score(result: RangeResult) -> RangeResult:
    """Every list of a `RangeResult` re-sorted by (score descending, id ascending) - the order of `search` - with plain torch ops on
    the device of the result (NumPy arrays: on the host, NumPy arrays back).  Scores compare as the search's keys do: `-0.0` equals
    `+0.0`, so two zeros of either sign are ordered by id.  The score bits are kept."""
    as_numpy = isinstance(result.scores, np.ndarray)
    lims, scores, ids = (torch.as_tensor(t) for t in result)
    seg = torch.repeat_interleave(torch.arange(lims.numel() - 1, device=lims.device), lims[1:] - lims[:-1])
    by_id = torch.argsort(ids, stable=True)
    by_score = by_id[torch.argsort(-(scores[by_id] + 0.0), stable=True)]  # (x + 0.0: -0.0 -> +0.0; stable: ties keep ascending ids)
    perm = by_score[torch.argsort(seg[by_score], stable=True)]
    scores, ids = scores[perm], ids[perm]
    if as_numpy:
        return RangeResult(result.lims, scores.numpy(), ids.numpy())
    return RangeResult(result.lims, scores, ids)


class PosteriorMean(NamedTuple):
    """`mean[q] = sum_z p(z | q) x_z` (`[nq, dim]`) of `posterior_mean`, with the `LogPartition` of the same call."""

    mean: Any
    log_partition: LogPartition


class PosteriorExpectation(NamedTuple):
    """`values[q] = sum_z p(z | q) v_z` (`[nq, n_cols]`) of `posterior_expectation`, with the `LogPartition` of the same call."""

    values: Any
    log_partition: LogPartition


def _row_values_shape(info, handle) -> "tuple[int, int] | None":
    n_rows, n_cols = ctypes.c_int64(0), ctypes.c_int64(0)
    _native.check(info(handle, ctypes.byref(n_rows), ctypes.byref(n_cols)))
    return (int(n_rows.value), int(n_cols.value)) if n_cols.value else None


class PosteriorStats(NamedTuple):
    """`posterior_stats`: `entropy = log_rel - mean_rel / temperature`, `mean_score = max_score + mean_rel = E_p[s]`,
    `var_score = Var_p[s]`, `mean_rel = E_p[s] - max_score <= 0`, each `[nq]`, with the `LogPartition` of the same call."""

    entropy: Any
    mean_score: Any
    var_score: Any
    mean_rel: Any
    log_partition: LogPartition


class DivergenceSide(NamedTuple):
    """One side of `posterior_divergence`: `max_score`, `log_rel`, `mean_rel = E[s] - max_score <= 0` under the side's own posterior,
    each `[nq]`, with the side's `LogPartition`."""

    max_score: Any
    log_rel: Any
    mean_rel: Any
    log_partition: LogPartition


class PosteriorDivergence(NamedTuple):
    """`posterior_divergence` of `p = softmax(s_a / T_a)` and `r = softmax(s_b / T_b)`: `kl_ab = KL(p || r)`, `cross_entropy_ab =
    H(p, r)`, `entropy_a = H(p)`, `cross_rel_ab = E_p[s_b] - max_b <= 0` and the mirrors, each `[nq]`, with each side's words."""

    kl_ab: Any
    kl_ba: Any
    cross_entropy_ab: Any
    cross_entropy_ba: Any
    entropy_a: Any
    entropy_b: Any
    cross_rel_ab: Any
    cross_rel_ba: Any
    stats_a: DivergenceSide
    stats_b: DivergenceSide


def posterior_divergence_words(words, beta_a: float, beta_b: float) -> PosteriorDivergence:
    """The eight library words (max_a, log_rel_a, mean_rel_a, cross_rel_ab, max_b, log_rel_b, mean_rel_b, cross_rel_ba; torch tensors
    or NumPy arrays) -> `PosteriorDivergence`.  Every derived word is formed in float64 from the float32 words and rounded to float32
    once, in a grouping that pairs each word with its own side's counterpart,
        entropy_a = log_rel_a - beta_a mean_rel_a,   cross_entropy_ab = log_rel_b - beta_b cross_rel_ab,
        kl_ab = max(0, (log_rel_b - log_rel_a) + (beta_a mean_rel_a - beta_b cross_rel_ab)),
    so that identical pairs give exactly 0; the betas are the float32 values the library received."""
    ma, ra, aa, cab, mb, rb, ab, cba = words
    is_torch = isinstance(ma, torch.Tensor)
    ba, bb = float(np.float32(beta_a)), float(np.float32(beta_b))

    def f64(t):
        return t.double() if is_torch else np.asarray(t, dtype=np.float64)

    def f32(t):
        return t.float() if is_torch else t.astype(np.float32)

    def clamp0(t):  # (NaN stays NaN)
        return torch.clamp(t, min=0.0) if is_torch else np.where(t < 0.0, 0.0, t)

    Ra, Aa, Cab, Rb, Ab, Cba = (f64(t) for t in (ra, aa, cab, rb, ab, cba))
    with np.errstate(invalid="ignore"):
        ent_a, ent_b = f32(Ra - ba * Aa), f32(Rb - bb * Ab)
        ce_ab, ce_ba = f32(Rb - bb * Cab), f32(Ra - ba * Cba)
        kl_ab = f32(clamp0((Rb - Ra) + (ba * Aa - bb * Cab)))
        kl_ba = f32(clamp0((Ra - Rb) + (bb * Ab - ba * Cba)))
        if is_torch:
            lz_a, lz_b = ma * ba + ra, mb * bb + rb  # (-inf + -inf and +inf + +inf: never NaN)
        else:
            lz_a, lz_b = (ma * np.float32(ba) + ra).astype(np.float32), (mb * np.float32(bb) + rb).astype(np.float32)
    return PosteriorDivergence(kl_ab, kl_ba, ce_ab, ce_ba, ent_a, ent_b, cab, cba,
                               DivergenceSide(ma, ra, aa, LogPartition(lz_a, ma, ra)), DivergenceSide(mb, rb, ab, LogPartition(lz_b, mb, rb)))


def kl_to_backward(grad_out: torch.Tensor, mean_student: torch.Tensor, mean_teacher: torch.Tensor, kl: torch.Tensor, beta: float,
                   dtype: torch.dtype) -> torch.Tensor:
    """The backward of `kl_to` in the student's queries: `d KL(p_teacher || p_student) / d b = beta (E_student[x] - E_teacher[x])`
    (`beta = 1 / temperature` of the student), so `grad = grad_out[:, None] * beta * (mean_student - mean_teacher)`, zero where `kl` is
    not finite, cast to `dtype`."""
    g = grad_out.to(torch.float32)[:, None] * (beta * (mean_student.to(torch.float32) - mean_teacher.to(torch.float32)))
    g = torch.where(torch.isfinite(kl)[:, None], g, torch.zeros_like(g))
    return g.to(dtype)


class _KlTo(torch.autograd.Function):
    """`index.kl_to`: `index` is anything with `posterior_divergence(a, b, T_a, T_b, subset)` and `posterior_mean(q, T, subset)`."""

    @staticmethod
    def forward(ctx, student, index, teacher, temperature, temperature_teacher, subset):
        teacher = teacher.detach() if isinstance(teacher, torch.Tensor) else teacher
        div = index.posterior_divergence(teacher, student.detach(), temperature_teacher, temperature, subset)
        kl = torch.as_tensor(div.kl_ab)
        ctx.q_dtype, ctx.q_device = student.dtype, student.device
        ctx.beta = 1.0 / temperature
        if ctx.needs_input_grad[0]:
            mean_s = torch.as_tensor(index.posterior_mean(student.detach(), temperature, subset).mean)
            mean_t = torch.as_tensor(index.posterior_mean(teacher, temperature_teacher, subset).mean)
            ctx.save_for_backward(mean_s, mean_t, kl)
        return kl.clone()

    @staticmethod
    def backward(ctx, grad_out):
        mean_s, mean_t, kl = ctx.saved_tensors
        g = kl_to_backward(grad_out.to(mean_s.device), mean_s, mean_t, kl, ctx.beta, ctx.q_dtype)
        return g.to(ctx.q_device), None, None, None, None, None


class PosteriorSample(NamedTuple):
    """`k` rows without replacement from `p(z | q)` over the whole store (`sample_posterior`): `ids`, `scores`, `log_p`, `log_weight`
    `[nq, k]`, `log_tau` `[nq]`, `keys` `[nq, k + 1]`, with the `LogPartition` of the same call."""

    ids: Any
    scores: Any
    log_p: Any
    log_weight: Any
    log_tau: Any
    keys: Any
    log_partition: LogPartition


def log_z_backward(grad_out: torch.Tensor, mean: torch.Tensor, log_z: torch.Tensor, beta: float, dtype: torch.dtype) -> torch.Tensor:
    """The backward of `log_z`: `grad_out[:, None] * beta * mean` in float32, zero where `log_z` is not finite, cast to `dtype`."""
    g = grad_out.to(torch.float32)[:, None] * (float(beta) * mean.to(torch.float32))
    g = torch.where(torch.isfinite(log_z)[:, None], g, torch.zeros_like(g))
    return g.to(dtype)


def log_z_temperature_backward(grad_out: torch.Tensor, mean_score: torch.Tensor, log_z: torch.Tensor, temperature: float) -> torch.Tensor:
    """The backward of `log_z` with respect to the temperature: `-sum_q grad_out[q] * mean_score[q] / T^2` (`d log Z / d beta =
    E_p[s]`, `beta = 1 / T`), summed in float64 over the queries whose `log_z` is finite; a 0-d float64 tensor."""
    g = grad_out.to(torch.float64) * mean_score.to(torch.float64)
    g = torch.where(torch.isfinite(log_z), g, torch.zeros_like(g))
    return -g.sum() / (float(temperature) ** 2)


class _LogZ(torch.autograd.Function):
    """`index.log_z`: `index` is anything with `posterior_mean(queries, temperature, subset)` and - for a tensor temperature -
    `posterior_stats(queries, temperature, subset)`."""

    @staticmethod
    def forward(ctx, queries, index, temperature, subset):
        ctx.t_tensor = isinstance(temperature, torch.Tensor)
        ctx.q_dtype, ctx.q_device = queries.dtype, queries.device
        if not ctx.t_tensor:
            pm = index.posterior_mean(queries.detach(), temperature, subset)
            log_z = torch.as_tensor(pm.log_partition.log_z)
            ctx.save_for_backward(torch.as_tensor(pm.mean), log_z)
            ctx.beta = 1.0 / temperature
            return log_z.clone()
        if temperature.numel() != 1:
            raise ValueError(f"expected a one-element temperature tensor, got shape {tuple(temperature.shape)}")
        ctx.t_shape, ctx.t_dtype, ctx.t_device = temperature.shape, temperature.dtype, temperature.device
        t = float(temperature.detach().reshape(()).item())  # (the one host synchronisation)
        ctx.temperature = t
        ctx.beta = 1.0 / t if t else float("nan")
        st = index.posterior_stats(queries.detach(), t, subset)
        log_z = torch.as_tensor(st.log_partition.log_z)
        mean = None
        if ctx.needs_input_grad[0]:
            pm = index.posterior_mean(queries.detach(), t, subset)
            mean, log_z = torch.as_tensor(pm.mean), torch.as_tensor(pm.log_partition.log_z)  # (the bits of the float path)
        ctx.save_for_backward(mean, log_z, torch.as_tensor(st.mean_score))
        return log_z.clone()

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.t_tensor:
            mean, log_z = ctx.saved_tensors
            g = log_z_backward(grad_out.to(mean.device), mean, log_z, ctx.beta, ctx.q_dtype)
            return g.to(ctx.q_device), None, None, None
        mean, log_z, mean_score = ctx.saved_tensors
        g_q = g_t = None
        if ctx.needs_input_grad[0]:
            g_q = log_z_backward(grad_out.to(mean.device), mean, log_z, ctx.beta, ctx.q_dtype).to(ctx.q_device)
        if ctx.needs_input_grad[2]:
            g_t = log_z_temperature_backward(grad_out.to(log_z.device), mean_score, log_z, ctx.temperature)
            g_t = g_t.to(device=ctx.t_device, dtype=ctx.t_dtype).reshape(ctx.t_shape)
        return g_q, None, g_t, None


def listed_scores_backward(index, ids, grad_out: torch.Tensor, dtype: torch.dtype, device: torch.device, **kw) -> torch.Tensor:
    """The backward of `listed_scores`: `index.sum_ids(ids, grad_out, **kw)` cast to `dtype` on `device`.  Absent slots drop out inside
    `sum_ids` whatever their gradient (NaN at a -inf score included): nothing is masked here."""
    g = index.sum_ids(ids, grad_out, **kw)
    if not isinstance(g, torch.Tensor):
        g = torch.as_tensor(g)
    return g if g.dtype == dtype and g.device == device else g.to(device=device, dtype=dtype)


class _ListedScores(torch.autograd.Function):
    """`index.listed_scores`: `index` is anything with `score_ids(queries, ids, **kw)` and `sum_ids(ids, weights, **kw)`."""

    @staticmethod
    def forward(ctx, queries, index, ids, kw):
        scores = torch.as_tensor(index.score_ids(queries.detach(), ids, **kw))
        ctx.index, ctx.ids, ctx.kw = index, ids, kw
        ctx.q_dtype, ctx.q_device = queries.dtype, queries.device
        return scores

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        return listed_scores_backward(ctx.index, ctx.ids, grad_out, ctx.q_dtype, ctx.q_device, **ctx.kw), None, None, None


class _ExpectedValues(torch.autograd.Function):
    """`index.expected_values`: `index` is anything with `posterior_expectation(queries, temperature, subset)` and
    `posterior_expectation_backward(queries, grad_values, expectation, temperature, subset)`."""

    @staticmethod
    def forward(ctx, queries, index, temperature, subset):
        pe = index.posterior_expectation(queries.detach(), temperature, subset)
        values = torch.as_tensor(pe.values)
        ctx.index, ctx.temperature, ctx.subset = index, temperature, subset
        ctx.q_dtype, ctx.q_device = queries.dtype, queries.device
        ctx.save_for_backward(queries.detach(), values, torch.as_tensor(pe.log_partition.max_score), torch.as_tensor(pe.log_partition.log_rel))
        return values.to(queries.device).clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        queries, values, max_score, log_rel = ctx.saved_tensors
        beta = 1.0 / ctx.temperature if ctx.temperature else float("nan")
        pe = PosteriorExpectation(values, LogPartition(max_score * beta + log_rel, max_score, log_rel))
        g = torch.as_tensor(ctx.index.posterior_expectation_backward(queries, grad_out, pe, ctx.temperature, ctx.subset))
        return g.to(device=ctx.q_device, dtype=ctx.q_dtype), None, None, None


class _ReadOut(torch.autograd.Function):
    """`index.read_out`: `index` is anything with `set_row_values`, `posterior_expectation`, `posterior_expectation_backward` and
    `posterior_adjoint(queries, weights, log_partition, temperature, subset)`."""

    @staticmethod
    def forward(ctx, queries, values, index, temperature, subset):
        index.set_row_values(values.detach())
        pe = index.posterior_expectation(queries.detach(), temperature, subset)
        y = torch.as_tensor(pe.values)
        ctx.index, ctx.temperature, ctx.subset = index, temperature, subset
        ctx.q_dtype, ctx.q_device = queries.dtype, queries.device
        ctx.v_dtype, ctx.v_device, ctx.v_shape = values.dtype, values.device, values.shape
        ctx.save_for_backward(queries.detach(), y, torch.as_tensor(pe.log_partition.max_score), torch.as_tensor(pe.log_partition.log_rel))
        return y.to(queries.device).clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        queries, y, max_score, log_rel = ctx.saved_tensors
        beta = 1.0 / ctx.temperature if ctx.temperature else float("nan")
        lp = LogPartition(max_score * beta + log_rel, max_score, log_rel)
        grad_q = grad_v = None
        if ctx.needs_input_grad[0]:
            g = torch.as_tensor(ctx.index.posterior_expectation_backward(queries, grad_out, PosteriorExpectation(y, lp), ctx.temperature, ctx.subset))
            grad_q = g.to(device=ctx.q_device, dtype=ctx.q_dtype)
        if ctx.needs_input_grad[1]:
            g = torch.as_tensor(ctx.index.posterior_adjoint(queries, grad_out, lp, ctx.temperature, ctx.subset))
            grad_v = g.to(device=ctx.v_device, dtype=ctx.v_dtype).reshape(ctx.v_shape)
        return grad_q, grad_v, None, None, None


def _checked_keys(index, keys) -> torch.Tensor:
    """`keys` of `log_z` / `read_out`: a floating tensor of the store's shape."""
    if not isinstance(keys, torch.Tensor) or not keys.is_floating_point() or tuple(keys.shape) != (index.ntotal, index.dim):
        got = tuple(keys.shape) if isinstance(keys, torch.Tensor) else type(keys).__name__
        raise ValueError(f"expected `keys` a float tensor [{index.ntotal}, {index.dim}] (the store), got {got}")
    return keys


def _key_grad_to(g, keys_meta):
    dtype, device = keys_meta
    return torch.as_tensor(g).to(device=device, dtype=dtype)


class _LogZKeys(torch.autograd.Function):
    """`index.log_z(..., keys=K)` with a float temperature: `_LogZ`'s forward and query gradient, bit for bit, and
    `index.key_gradient(queries, grad_log_z=grad_out, log_partition=the forward's)` for `K`."""

    @staticmethod
    def forward(ctx, queries, keys, index, temperature, subset):
        ctx.q_dtype, ctx.q_device = queries.dtype, queries.device
        ctx.k_meta = (keys.dtype, keys.device)
        pm = index.posterior_mean(queries.detach(), temperature, subset)
        lp = pm.log_partition
        log_z = torch.as_tensor(lp.log_z)
        ctx.index, ctx.temperature, ctx.subset = index, temperature, subset
        ctx.beta = 1.0 / temperature
        ctx.save_for_backward(queries.detach(), torch.as_tensor(pm.mean), log_z, torch.as_tensor(lp.max_score), torch.as_tensor(lp.log_rel))
        return log_z.clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        queries, mean, log_z, max_score, log_rel = ctx.saved_tensors
        g_q = g_k = None
        if ctx.needs_input_grad[0]:
            g_q = log_z_backward(grad_out.to(mean.device), mean, log_z, ctx.beta, ctx.q_dtype).to(ctx.q_device)
        if ctx.needs_input_grad[1]:
            lp = LogPartition(log_z, max_score, log_rel)
            g_k = _key_grad_to(ctx.index.key_gradient(queries, grad_log_z=grad_out, log_partition=lp, temperature=ctx.temperature, subset=ctx.subset), ctx.k_meta)
        return g_q, g_k, None, None, None


class _ReadOutKeys(torch.autograd.Function):
    """`index.read_out(..., keys=K)`: `_ReadOut`'s forward and its two gradients, bit for bit, and
    `index.key_gradient(queries, grad_values=grad_out, expectation=the forward's)` for `K`."""

    @staticmethod
    def forward(ctx, queries, values, keys, index, temperature, subset):
        ctx.k_meta = (keys.dtype, keys.device)
        index.set_row_values(values.detach())
        pe = index.posterior_expectation(queries.detach(), temperature, subset)
        y = torch.as_tensor(pe.values)
        ctx.index, ctx.temperature, ctx.subset = index, temperature, subset
        ctx.q_dtype, ctx.q_device = queries.dtype, queries.device
        ctx.v_dtype, ctx.v_device, ctx.v_shape = values.dtype, values.device, values.shape
        ctx.save_for_backward(queries.detach(), y, torch.as_tensor(pe.log_partition.max_score), torch.as_tensor(pe.log_partition.log_rel))
        return y.to(queries.device).clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        queries, y, max_score, log_rel = ctx.saved_tensors
        beta = 1.0 / ctx.temperature if ctx.temperature else float("nan")
        lp = LogPartition(max_score * beta + log_rel, max_score, log_rel)
        pe = PosteriorExpectation(y, lp)
        grad_q = grad_v = grad_k = None
        if ctx.needs_input_grad[0]:
            g = torch.as_tensor(ctx.index.posterior_expectation_backward(queries, grad_out, pe, ctx.temperature, ctx.subset))
            grad_q = g.to(device=ctx.q_device, dtype=ctx.q_dtype)
        if ctx.needs_input_grad[1]:
            g = torch.as_tensor(ctx.index.posterior_adjoint(queries, grad_out, lp, ctx.temperature, ctx.subset))
            grad_v = g.to(device=ctx.v_device, dtype=ctx.v_dtype).reshape(ctx.v_shape)
        if ctx.needs_input_grad[2]:
            grad_k = _key_grad_to(ctx.index.key_gradient(queries, grad_values=grad_out, expectation=pe, temperature=ctx.temperature, subset=ctx.subset), ctx.k_meta)
        return grad_q, grad_v, grad_k, None, None, None


def topk_log_coverage(scores: torch.Tensor, log_partition: LogPartition, temperature: float = 1.0) -> torch.Tensor:
    """Log of the posterior mass a returned top-k list covers: `logsumexp(scores / T - max_score / T) - log_rel`, `[nq]`, <= 0 up to
    rounding.  `scores`: `[nq, k]` as `search` returns them (pads -inf drop out); `log_partition`: what `log_partition` returned for the
    same queries and temperature.  Plain torch on the device of `scores`; a query with no eligible row gives NaN (0 / 0)."""
    s = torch.as_tensor(scores).float()
    m = torch.as_tensor(log_partition.max_score).to(s.device).float()
    r = torch.as_tensor(log_partition.log_rel).to(s.device).float()
    return torch.logsumexp((s - m[:, None]) / float(temperature), dim=1) - r


def rank_metrics(rank, ks=(1, 5, 20, 100)) -> dict[str, float]:
    """Retrieval metrics from exact ranks (`rank_ids(...).rank`, `[nq, m]` or `[nq]`, 0-based, -1 = not ranked): `mrr`, `hit@k` for
    every `k` of `ks`, `mean_rank` and `median_rank`.  Slots with rank -1 are left out everywhere.  For `mrr` and `hit@k` a query's BEST
    present slot counts (one reciprocal rank per query, averaged over the queries that have a present slot); `mean_rank` / `median_rank`
    are over all present slots, 0-based.  No present slot at all: every value NaN.  Plain torch on the device of `rank`."""
    r = torch.as_tensor(rank)
    if r.ndim == 1:
        r = r[:, None]
    present = r >= 0
    out: dict[str, float] = {}
    if not bool(present.any()):
        nan = float("nan")
        return {"mrr": nan, **{f"hit@{int(k)}": nan for k in ks}, "mean_rank": nan, "median_rank": nan}
    big = torch.iinfo(torch.int64).max
    best = torch.where(present, r, torch.full_like(r, big)).min(dim=1).values
    best = best[present.any(dim=1)].to(torch.float64)
    out["mrr"] = float((1.0 / (best + 1.0)).mean())
    for k in ks:
        out[f"hit@{int(k)}"] = float((best < int(k)).to(torch.float64).mean())
    flat = r[present].to(torch.float64)
    out["mean_rank"] = float(flat.mean())
    out["median_rank"] = float(flat.median())  # (the lower of the two middle values of an even count)
    return out


def merge_topk(scores: torch.Tensor, ids: torch.Tensor, k_out: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Merge per-shard top-k lists [n_shards, nq, k] (global ids, pads -1) into [nq, k_out] on the GPU."""
    lib = _native.load_library()
    if scores.ndim != 3 or ids.shape != scores.shape:
        raise ValueError("expected scores/ids of shape [n_shards, nq, k]")
    n_shards, nq, k = scores.shape
    k_out = k if k_out is None else int(k_out)
    scores = scores.contiguous().float()
    ids = ids.contiguous().long()
    out_s = torch.empty((nq, k_out), dtype=torch.float32, device=scores.device)
    out_i = torch.empty((nq, k_out), dtype=torch.int64, device=scores.device)
    with torch.cuda.device(scores.device):
        _native.check(
            lib.vodhip_merge_topk(scores.data_ptr(), ids.data_ptr(), n_shards, nq, k, k_out, out_s.data_ptr(),
                                  out_i.data_ptr(), _native.current_stream_ptr(scores.device))
        )
    return out_s, out_i


class PackedTopk:
    """One contiguous per-rank record `[scores f32 nq*k | ids i64 nq*k]` so that the multi-GPU exchange is ONE all-gather.

    `scores` / `ids` are views into `buffer` (uint8); `merge_gathered` merges `world` such records laid end to end.
    """

    def __init__(self, nq: int, k: int, device: torch.device):
        self.nq, self.k = int(nq), int(k)
        n = self.nq * self.k
        self._s_bytes = (n * 4 + 7) // 8 * 8  # keep the id block 8-byte aligned
        self.nbytes = self._s_bytes + n * 8
        self.buffer = torch.empty((self.nbytes,), dtype=torch.uint8, device=device)
        self.scores = self.buffer[: n * 4].view(torch.float32).view(self.nq, self.k)
        self.ids = self.buffer[self._s_bytes :].view(torch.int64).view(self.nq, self.k)

    def merge_gathered(self, gathered: torch.Tensor, world: int, k_out: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """`gathered`: uint8 [world * nbytes] (rank-major).  Returns merged (scores [nq,k_out], ids [nq,k_out])."""
        lib = _native.load_library()
        k_out = self.k if k_out is None else int(k_out)
        dev = gathered.device
        out_s = torch.empty((self.nq, k_out), dtype=torch.float32, device=dev)
        out_i = torch.empty((self.nq, k_out), dtype=torch.int64, device=dev)
        base = gathered.data_ptr()
        with torch.cuda.device(dev):
            _native.check(
                lib.vodhip_merge_topk_strided(base, self.nbytes // 4, base + self._s_bytes, self.nbytes // 8, int(world), self.nq,
                                              self.k, k_out, out_s.data_ptr(), out_i.data_ptr(), _native.current_stream_ptr(dev))
            )
        return out_s, out_i


class HipNodeIndex:
    """The row-sharded index of one node in ONE process (`vodhip_node_index_*`): shard g on `devices[g]` holds a contiguous row
    range, a search runs on every device at once and the per-shard top-k lists are merged on `devices[0]`.

    Counterpart of faiss `index_cpu_to_all_gpus(..., shard=True)` (/root/reference/src/vod_search/faiss_search/server.py:51-54).
    The collective variant (one process per GPU, one RCCL all-gather) is `vod_amd.distributed.ShardedFlatIndex`; this one is what a
    C / C++ consumer of the library gets, and what a single-process Python host can use without `torch.distributed`.
    """

    def __init__(self, dim: int, capacity: int, devices: list[int], dtype: torch.dtype = torch.float16, exact_f32: bool = False,
                 metric: str = "inner_product"):
        self._lib = _native.load_library()
        if not torch.cuda.is_available():
            raise _native.NativeLibraryError("HipNodeIndex needs a ROCm device (torch.cuda.is_available() is False)")
        if dtype not in (torch.float16, torch.bfloat16):
            raise TypeError("store dtype must be torch.float16 or torch.bfloat16")
        if not devices:
            raise ValueError("devices must list at least one device ordinal")
        self.dim, self.capacity, self.dtype, self.devices = int(dim), int(capacity), dtype, [int(d) for d in devices]
        self.device = torch.device("cuda", self.devices[0])
        self.exact_f32 = bool(exact_f32)  # every shard keeps its float32 rows (HipFlatIndex): the merged result is the float32 brute force
        handle = ctypes.c_void_p()
        arr = (ctypes.c_int32 * len(self.devices))(*self.devices)
        self.metric = metric  # (the library refuses VODHIP_L2 here: the shards' lists are merged by inner product)
        code = _native.torch_dtype_code(dtype) | (_native.EXACT_F32 if self.exact_f32 else 0) | _native.metric_flag(metric)
        _native.check(self._lib.vodhip_node_index_create(len(self.devices), arr, self.dim, code, self.capacity, ctypes.byref(handle)))
        self._h = handle

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vodhip_node_index_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "HipNodeIndex":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    @property
    def ntotal(self) -> int:
        out = ctypes.c_int64()
        _native.check(self._lib.vodhip_node_index_ntotal(self._h, ctypes.byref(out)))
        return out.value

    def reset(self) -> None:
        _native.check(self._lib.vodhip_node_index_reset(self._h))

    def set_param(self, key: str, value: int) -> None:
        _native.check(self._lib.vodhip_node_index_set_param(self._h, key.encode(), int(value)))

    def get_stat(self, key: str) -> int:
        """Node-level stats: of the last search with `set_param("profile", 1)`, "last_merge_ns" and "last_copy_ns_max" (HIP events); of
        the last `update_rows` / `add_to_rows`, "last_update_written", "last_update_skipped", "last_update_duplicates", of the last `remove_rows`
        "last_remove_removed", "last_remove_skipped", "last_remove_duplicates" (sums over the shards)."""
        out = ctypes.c_int64()
        _native.check(self._lib.vodhip_node_index_get_stat(self._h, key.encode(), ctypes.byref(out)))
        return out.value

    def shard_stat(self, g: int, key: str) -> int:
        """`vodhip_index_get_stat` of shard g's own handle (e.g. "last_filter_ns" with profiling on)."""
        out = ctypes.c_int64()
        _native.check(self._lib.vodhip_index_get_stat(ctypes.c_void_p(self.shard(g)[0]), key.encode(), ctypes.byref(out)))
        return out.value

    def peer_access(self) -> list[int]:
        """Per shard: 2 = on `devices[0]`, 1 = direct peer copies with it, 0 = staged through pinned host memory (no peer access, or
        `set_param("host_staging", 1)`)."""
        out = (ctypes.c_int32 * len(self.devices))()
        _native.check(min(0, self._lib.vodhip_node_index_peer_access(self._h, out, len(self.devices))))
        return list(out)

    def shard(self, g: int) -> tuple[int, int, int]:
        """(raw `vodhip_index_t*` of shard g, its id offset, its device) - for stats / params of one shard."""
        h, base, dev = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int32()
        _native.check(self._lib.vodhip_node_index_shard(self._h, int(g), ctypes.byref(h), ctypes.byref(base), ctypes.byref(dev)))
        return h.value, base.value, dev.value

    def add(self, vectors: np.ndarray) -> None:
        """Append host rows (float32 / float16 NumPy, [n, dim]); the shards the batch straddles ingest concurrently."""
        v = np.ascontiguousarray(vectors)
        if v.ndim != 2 or v.shape[1] != self.dim:
            raise ValueError(f"expected [n, {self.dim}] vectors, got {tuple(v.shape)}")
        if v.dtype not in (np.float32, np.float16):
            v = v.astype(np.float32)
        code = 2 if v.dtype == np.float32 else 0
        _native.check(self._lib.vodhip_node_index_add(self._h, v.ctypes.data, v.shape[0], code))

    def _update(self, mode: int, vectors, alpha: float, ids, begin: int) -> None:
        v, ida = _host_update_args(vectors, ids, self.dim)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_update_rows(
                self._h, ida.ctypes.data if ida is not None and ida.size else None, int(begin), v.ctypes.data if v.size else None, v.shape[0],
                _native.numpy_dtype_code(v.dtype), mode, float(alpha)))

    def update_rows(self, vectors: np.ndarray, ids=None, begin: int = 0) -> None:
        """Overwrite stored rows in place from host arrays (global row ids, or the global rows `begin .. begin + n`): see
        `HipFlatIndex.update_rows`.  The call is routed on the host: every shard receives its own slots and rows only."""
        self._update(_native.UPDATE_SET, vectors, 1.0, ids, begin)

    def add_to_rows(self, delta: np.ndarray, alpha: float = 1.0, ids=None, begin: int = 0, check: bool = True) -> None:
        """`x[ids] += alpha * delta` in place from host arrays: see `HipFlatIndex.add_to_rows` (the 16-bit master copy of a plain
        store, unique ids, `check`)."""
        self._update(_native.UPDATE_ADD, delta, alpha, ids, begin)
        if check and ids is not None and (dup := self.get_stat("last_update_duplicates")):
            raise ValueError(f"add_to_rows: {dup} slots repeat an id that a later slot lists too; only the last slot of an id was applied")

    def remove_rows(self, ids=None, begin: int = 0, n: int | None = None, mask=None, return_map: bool = False):
        """Remove stored rows (global row ids, the global range `begin .. begin + n`, or a boolean mask) and restore the layout `add`
        fills - every shard full before the next one starts: see `HipFlatIndex.remove_rows`.  Each shard compacts on its device, the
        survivors then move between the shards device to device.  `return_map=True` adds the host int64 array `[old ntotal]` of new
        global ids (-1: removed)."""
        old = self.ntotal
        ida, begin, n = remove_rows_args(ids, begin, n, mask, old)
        if isinstance(ida, torch.Tensor):
            ida = ida.cpu().numpy()
        new_ids = np.arange(old, dtype=np.int64) if return_map else None
        removed = ctypes.c_int64()
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_remove_rows(
                self._h, ida.ctypes.data if ida is not None and n else None, begin, n, new_ids.ctypes.data if return_map and old else None,
                ctypes.byref(removed)))
        return (removed.value, new_ids) if return_map else removed.value

    def set_row_labels(self, labels: np.ndarray | None) -> None:
        """One int32 subset label per stored row (global row order; None clears): see `HipFlatIndex.set_row_labels`."""
        if labels is None:
            _native.check(self._lib.vodhip_node_index_set_row_labels(self._h, None, 0))
            return
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        _native.check(self._lib.vodhip_node_index_set_row_labels(self._h, lab.ctypes.data, lab.size))

    def set_row_values(self, values: np.ndarray | None) -> None:
        """One value row per stored row (global row order, `[ntotal, n_cols]`, 1 <= n_cols <= 256; None clears), split by shard row
        ranges: see `HipFlatIndex.set_row_values`."""
        if values is None:
            _native.check(self._lib.vodhip_node_index_set_row_values(self._h, None, 0, 0, 0))
            return
        if isinstance(values, torch.Tensor):
            values = values.detach().float().cpu().numpy()
        v = np.asarray(values)
        v = v.reshape(-1, 1) if v.ndim == 1 else v
        if v.ndim != 2:
            raise ValueError(f"expected [ntotal, n_cols] values, got {tuple(v.shape)}")
        if v.dtype not in (np.float32, np.float16):
            v = v.astype(np.float32)
        v = np.ascontiguousarray(v)
        src = v if v.size else np.zeros(1, dtype=v.dtype)  # (a table of no rows is still a table: NULL would clear it)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_set_row_values(self._h, src.ctypes.data, v.shape[0], v.shape[1],
                                                                     2 if v.dtype == np.float32 else 0))

    @property
    def row_values_shape(self) -> tuple[int, int] | None:
        """`(n_rows, n_cols)` of the value table, or None when there is none."""
        return _row_values_shape(self._lib.vodhip_node_index_row_values_info, self._h)

    def _set_subset(self, subset: np.ndarray | None, nq: int):
        if subset is None:
            _native.check(self._lib.vodhip_node_index_set_query_labels(self._h, None, 0, 0))
            return None
        sub = np.ascontiguousarray(subset, dtype=np.int32)
        if sub.ndim != 2 or sub.shape[0] != nq:
            raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
        _native.check(self._lib.vodhip_node_index_set_query_labels(self._h, sub.ctypes.data, int(sub.shape[1]), 0))
        return sub  # kept alive by the caller's frame until the search has returned

    def search_async(self, queries: np.ndarray | torch.Tensor, k: int, subset: np.ndarray | None = None) -> None:
        """The first half of `search` (round 6): the batch is replicated and every shard's search enqueued; `finish()` completes the OLDEST
        pending search and returns its (scores, ids).  Up to two searches may be pending, so a caller that runs one batch ahead keeps every
        device busy while the host enqueues the next batch's launches on all shards.  Inputs / outputs as in `search`."""
        keep = self._set_subset(subset, int(queries.shape[0]))
        if isinstance(queries, torch.Tensor):
            if queries.device != self.device:
                raise ValueError(f"queries live on {queries.device}, the merge device is {self.device}")
            q = queries.contiguous()
            if q.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                q = q.float()
            if q.ndim != 2 or q.shape[1] != self.dim:
                raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
            out_s = torch.empty((q.shape[0], k), dtype=torch.float32, device=self.device)
            out_i = torch.empty((q.shape[0], k), dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                _native.check(self._lib.vodhip_node_index_search_async(self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), q.shape[0], int(k), 1,
                                                                       out_s.data_ptr(), out_i.data_ptr(), _native.current_stream_ptr(self.device)))
        else:
            q = np.ascontiguousarray(queries)
            if q.dtype not in (np.float32, np.float16):
                q = q.astype(np.float32)
            if q.ndim != 2 or q.shape[1] != self.dim:
                raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
            out_s = np.empty((q.shape[0], k), dtype=np.float32)
            out_i = np.empty((q.shape[0], k), dtype=np.int64)
            _native.check(self._lib.vodhip_node_index_search_async(self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, q.shape[0], int(k), 0,
                                                                   out_s.ctypes.data, out_i.ctypes.data, None))
        if not hasattr(self, "_pending"):
            self._pending = []
        self._pending.append((q, keep, out_s, out_i))  # (queries, labels and outputs stay alive until the finish)

    def finish(self):
        """Complete the oldest pending `search_async`; returns its (scores, ids)."""
        if not getattr(self, "_pending", None):
            raise RuntimeError("no search is pending on this node index")
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_search_finish(self._h))
        _q, _keep, out_s, out_i = self._pending.pop(0)
        return out_s, out_i

    def search(self, queries: np.ndarray | torch.Tensor, k: int, subset: np.ndarray | None = None):
        """NumPy in -> NumPy out (host buffers, synchronous); a tensor on `devices[0]` in -> tensors there, complete on the current stream.
        `subset`: int32 [nq, n_per_query] allowed row labels per query (-1 = empty slot; host array)."""
        _keep = self._set_subset(subset, int(queries.shape[0]))  # noqa: F841
        if isinstance(queries, torch.Tensor):
            if queries.device != self.device:
                raise ValueError(f"queries live on {queries.device}, the merge device is {self.device}")
            q = queries.contiguous()
            if q.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                q = q.float()
            if q.ndim != 2 or q.shape[1] != self.dim:
                raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
            out_s = torch.empty((q.shape[0], k), dtype=torch.float32, device=self.device)
            out_i = torch.empty((q.shape[0], k), dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                _native.check(self._lib.vodhip_node_index_search(self._h, q.data_ptr(), _native.torch_dtype_code(q.dtype), q.shape[0], int(k), 1,
                                                                 out_s.data_ptr(), out_i.data_ptr(), _native.current_stream_ptr(self.device)))
            return out_s, out_i
        q = np.ascontiguousarray(queries)
        if q.dtype not in (np.float32, np.float16):
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        out_s = np.empty((q.shape[0], k), dtype=np.float32)
        out_i = np.empty((q.shape[0], k), dtype=np.int64)
        _native.check(self._lib.vodhip_node_index_search(self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, q.shape[0], int(k), 0,
                                                         out_s.ctypes.data, out_i.ctypes.data, None))
        return out_s, out_i

    def log_partition(self, queries, temperature: float = 1.0, subset: np.ndarray | None = None) -> LogPartition:
        """`HipFlatIndex.log_partition` over every shard: each shard scans its rows on its own device, the per-shard pairs are folded on
        the host in shard order.  Host queries (NumPy, or a tensor that is copied to the host) -> `LogPartition` of float32 NumPy arrays
        `[nq]`; `max_score` equals one index holding all the rows bit for bit."""
        if isinstance(queries, torch.Tensor):
            queries = queries.detach().float().cpu().numpy()
        q = np.ascontiguousarray(queries)
        if q.dtype not in (np.float32, np.float16):
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        nq = int(q.shape[0])
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        max_score = np.empty((nq,), dtype=np.float32)
        log_rel = np.empty((nq,), dtype=np.float32)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_log_partition(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, beta, None if sub is None else sub.ctypes.data, n_sub,
                max_score.ctypes.data, log_rel.ctypes.data))
        with np.errstate(invalid="ignore"):
            log_z = (max_score * np.float32(beta) + log_rel).astype(np.float32)
        return LogPartition(log_z, max_score, log_rel)

    def posterior_stats(self, queries, temperature: float = 1.0, subset: np.ndarray | None = None) -> "PosteriorStats":
        """`HipFlatIndex.posterior_stats` over every shard: each shard runs the flat call on its own device, the four words per shard
        are folded on the host in shard order, in double (a mixture of the shards' posteriors).  Host queries -> `PosteriorStats` of
        float32 NumPy arrays `[nq]`; `max_score` equals one index holding all the rows bit for bit."""
        q = self._host_queries(queries)
        nq = int(q.shape[0])
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = self._host_subset(subset, nq)
        max_score, log_rel, mean_rel, var = (np.empty((nq,), dtype=np.float32) for _ in range(4))
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_posterior_stats(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, beta, None if sub is None else sub.ctypes.data, n_sub,
                max_score.ctypes.data, log_rel.ctypes.data, mean_rel.ctypes.data, var.ctypes.data))
        with np.errstate(invalid="ignore"):
            log_z = (max_score * np.float32(beta) + log_rel).astype(np.float32)
            entropy = (log_rel - np.float32(beta) * mean_rel).astype(np.float32)
            mean_score = (max_score + mean_rel).astype(np.float32)
        return PosteriorStats(entropy, mean_score, var, mean_rel, LogPartition(log_z, max_score, log_rel))

    def posterior_divergence(self, queries_a, queries_b, temperature_a: float = 1.0, temperature_b: float | None = None,
                             subset: np.ndarray | None = None, out=None) -> "PosteriorDivergence":
        """`HipFlatIndex.posterior_divergence` over every shard: each shard runs the flat call on its own device, the eight words per
        shard are folded on the host in shard order, in double (a mixture of the shards' posteriors on each side).  Host queries ->
        `PosteriorDivergence` of float32 NumPy arrays `[nq]`; `max_score` of each side equals one index holding all the rows bit for
        bit.  `out`: eight float32 NumPy arrays `[nq]` to write the library words into."""
        qa = self._host_queries(queries_a)
        qb = self._host_queries(queries_b)
        if qb.dtype != qa.dtype:
            qa, qb = qa.astype(np.float32), qb.astype(np.float32)
        nq = int(qa.shape[0])
        if qb.shape[0] != nq:
            raise ValueError(f"expected {nq} queries on each side, got {qb.shape[0]} for b")
        beta_a = 1.0 / float(temperature_a) if temperature_a else float("nan")
        beta_b = beta_a if temperature_b is None else (1.0 / float(temperature_b) if temperature_b else float("nan"))
        sub, n_sub = self._host_subset(subset, nq)
        words = tuple(np.empty((nq,), dtype=np.float32) for _ in range(8)) if out is None else tuple(out)
        if len(words) != 8 or any(w.dtype != np.float32 or w.shape != (nq,) or not w.flags.c_contiguous for w in words):
            raise ValueError("expected eight contiguous float32 [nq] arrays as out")
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_posterior_divergence(
                self._h, qa.ctypes.data, qb.ctypes.data, 2 if qa.dtype == np.float32 else 0, nq, beta_a, beta_b,
                None if sub is None else sub.ctypes.data, n_sub, *[w.ctypes.data for w in words]))
        return posterior_divergence_words(words, beta_a, beta_b)

    def kl_to(self, teacher_queries, student_queries: torch.Tensor, temperature: float = 1.0, temperature_teacher: float | None = None,
              subset=None) -> torch.Tensor:
        """`HipFlatIndex.kl_to` over every shard: a float32 host tensor `[nq]`, differentiable in `student_queries`."""
        t_teacher = float(temperature) if temperature_teacher is None else float(temperature_teacher)
        teacher = teacher_queries.detach() if isinstance(teacher_queries, torch.Tensor) else teacher_queries
        return _KlTo.apply(student_queries, self, teacher, float(temperature), t_teacher, subset)

    def _host_queries(self, queries) -> np.ndarray:
        if isinstance(queries, torch.Tensor):
            queries = queries.detach().float().cpu().numpy()
        q = np.ascontiguousarray(queries)
        if q.dtype not in (np.float32, np.float16):
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        return q

    @staticmethod
    def _host_subset(subset, nq: int):
        if subset is None:
            return None, 0
        sub = np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
        if sub.ndim != 2 or sub.shape[0] != nq:
            raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
        return sub, int(sub.shape[1])

    def rank_ids(self, queries, ids, *, subset=None) -> "ListedRanks":
        """`HipFlatIndex.rank_ids` over every shard, `ids` GLOBAL row ids: each shard picks the scan scores of the ids it owns, the
        host combines them by ownership, each shard counts its rows against the combined (score, id) pairs and the host adds the
        counts.  Host inputs -> `ListedRanks` of NumPy arrays `[nq, m]` that equal one index holding all the rows bit for bit."""
        q = self._host_queries(queries)
        nq = int(q.shape[0])
        if isinstance(ids, torch.Tensor):
            ids = ids.detach().cpu().numpy()
        lst = np.ascontiguousarray(ids, dtype=np.int64) if isinstance(ids, np.ndarray) else pad_listed_ids(ids, nq)
        if lst.ndim != 2 or lst.shape[0] != nq:
            raise ValueError(f"expected ids of shape [{nq}, m], got {tuple(lst.shape)}")
        m = int(lst.shape[1])
        sub, n_sub = self._host_subset(subset, nq)
        rank = np.empty((nq, m), dtype=np.int64)
        score = np.empty((nq, m), dtype=np.float32)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_rank_ids(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, lst.ctypes.data, m, None if sub is None else sub.ctypes.data,
                n_sub, rank.ctypes.data, score.ctypes.data))
        return ListedRanks(rank, score)

    def count_above(self, queries, thresholds, *, tie_ids=None, subset=None) -> np.ndarray:
        """`HipFlatIndex.count_above` over every shard (`tie_ids` GLOBAL row ids): the shards' counts added on the host in int64.  Host
        inputs -> int64 NumPy array `[nq, m]` that equals one index holding all the rows."""
        q = self._host_queries(queries)
        nq = int(q.shape[0])
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.detach().cpu().numpy()
        thr = np.ascontiguousarray(thresholds, dtype=np.float32)
        if thr.ndim != 2 or thr.shape[0] != nq:
            raise ValueError(f"expected thresholds of shape [{nq}, m], got {tuple(thr.shape)}")
        m = int(thr.shape[1])
        tie = None
        if tie_ids is not None:
            if isinstance(tie_ids, torch.Tensor):
                tie_ids = tie_ids.detach().cpu().numpy()
            tie = np.ascontiguousarray(tie_ids, dtype=np.int64)
            if tie.shape != (nq, m):
                raise ValueError(f"expected tie_ids of shape {(nq, m)}, got {tuple(tie.shape)}")
        sub, n_sub = self._host_subset(subset, nq)
        out = np.empty((nq, m), dtype=np.int64)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_count_above(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, thr.ctypes.data, None if tie is None else tie.ctypes.data, m,
                None if sub is None else sub.ctypes.data, n_sub, out.ctypes.data))
        return out

    def range_search(self, queries, thresholds, *, tie_ids=None, inclusive: bool = False, subset=None, max_results: int | None = None,
                     order: str = "id") -> "RangeResult":
        """`HipFlatIndex.range_search` over every shard (`tie_ids` GLOBAL row ids): each shard runs the flat call with its own id base,
        the host concatenates a query's per-shard lists in shard order, which is ascending ids.  Host inputs -> `RangeResult` of NumPy
        arrays that equals one index holding all the rows byte for byte.  With `max_results` the outputs are sized up front and more
        hits raise with the needed size; without it a sizing call runs first."""
        q = self._host_queries(queries)
        nq = int(q.shape[0])
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.detach().cpu().numpy()
        thr = np.ascontiguousarray(thresholds, dtype=np.float32)
        tie = None
        if tie_ids is not None:
            if isinstance(tie_ids, torch.Tensor):
                tie_ids = tie_ids.detach().cpu().numpy()
            tie = np.ascontiguousarray(tie_ids, dtype=np.int64)
        check_range_args(nq, tuple(thr.shape), None if tie is None else tuple(tie.shape), inclusive, max_results, order)
        if inclusive:  # a tie row past every row
            tie = np.full((nq,), np.iinfo(np.int64).max, dtype=np.int64)
        sub, n_sub = self._host_subset(subset, nq)
        lims = np.zeros((nq + 1,), dtype=np.int64)

        def call(scores, ids, capacity):
            with torch.cuda.device(self.device):
                return self._lib.vodhip_node_index_range_search(
                    self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, thr.ctypes.data, None if tie is None else tie.ctypes.data,
                    None if sub is None else sub.ctypes.data, n_sub, lims.ctypes.data, None if scores is None else scores.ctypes.data,
                    None if ids is None else ids.ctypes.data, int(capacity))

        if max_results is None:
            _native.check(call(None, None, 0))
            capacity = int(lims[-1])
        else:
            capacity = int(max_results)
        scores = np.empty((max(capacity, 1),), dtype=np.float32)  # (never a NULL pointer: NULL outputs mean the sizing call)
        ids = np.empty((max(capacity, 1),), dtype=np.int64)
        status = call(scores, ids, capacity)
        if status != 0 and int(lims[-1]) > capacity:
            msg = self._lib.vodhip_last_error().decode("utf-8", "replace")
            raise _native.NativeLibraryError(f"{msg}: call range_search with max_results >= {int(lims[-1])}")
        _native.check(status)
        total = int(lims[-1])
        res = RangeResult(lims, scores[:total], ids[:total])
        return sort_range_by_score(res) if order == "score" else res

    def outranking(self, queries, ids, *, subset=None, order: str = "score") -> "RangeResult":
        """`HipFlatIndex.outranking` over every shard (`ids` GLOBAL row ids, int64 `[nq]`): NumPy arrays."""
        if isinstance(ids, torch.Tensor):
            ids = ids.detach().cpu().numpy()
        tgt = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        ranks = self.rank_ids(queries, tgt[:, None], subset=subset)
        thr = np.where(ranks.rank[:, 0] >= 0, ranks.score[:, 0], np.float32(np.nan)).astype(np.float32)
        return self.range_search(queries, thr, tie_ids=tgt, subset=subset, order=order)

    def posterior_support(self, queries, min_prob: float, temperature: float = 1.0, subset=None) -> "PosteriorSupport":
        """`HipFlatIndex.posterior_support` over every shard: the folded `log_partition`, the same rounded threshold (membership is
        defined by it), `range_search`; NumPy arrays."""
        if not 0.0 < float(min_prob) <= 1.0:
            raise ValueError(f"min_prob must be in (0, 1], got {min_prob}")
        t = float(temperature)
        lp = self.log_partition(queries, temperature=t, subset=subset)
        log_z = np.asarray(lp.max_score, dtype=np.float64) / t + np.asarray(lp.log_rel, dtype=np.float64)
        thr = (t * (log_z + math.log(float(min_prob)))).astype(np.float32)
        res = self.range_search(queries, thr, subset=subset)
        seg = np.repeat(np.arange(thr.shape[0]), np.diff(res.lims))
        log_p = (res.scores.astype(np.float64) / t - log_z[seg]).astype(np.float32)
        return PosteriorSupport(res.lims, res.scores, res.ids, log_p, lp)

    def posterior_mean(self, queries, temperature: float = 1.0, subset: np.ndarray | None = None) -> "PosteriorMean":
        """`HipFlatIndex.posterior_mean` over every shard: each shard runs the flat call on its own device, the shards are folded on the
        host in shard order, in double (`mean = sum_g w_g mean_g`).  Host queries -> `PosteriorMean` of float32 NumPy arrays;
        `max_score` equals one index holding all the rows bit for bit."""
        if isinstance(queries, torch.Tensor):
            queries = queries.detach().float().cpu().numpy()
        q = np.ascontiguousarray(queries)
        if q.dtype not in (np.float32, np.float16):
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        nq = int(q.shape[0])
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        max_score = np.empty((nq,), dtype=np.float32)
        log_rel = np.empty((nq,), dtype=np.float32)
        mean = np.empty((nq, self.dim), dtype=np.float32)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_posterior_mean(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, beta, None if sub is None else sub.ctypes.data, n_sub,
                max_score.ctypes.data, log_rel.ctypes.data, mean.ctypes.data))
        with np.errstate(invalid="ignore"):
            log_z = (max_score * np.float32(beta) + log_rel).astype(np.float32)
        return PosteriorMean(mean, LogPartition(log_z, max_score, log_rel))

    def posterior_expectation(self, queries, temperature: float = 1.0, subset: np.ndarray | None = None) -> "PosteriorExpectation":
        """`HipFlatIndex.posterior_expectation` over every shard: each shard reads out its rows of the value table on its own device, the
        shards are folded on the host in shard order, in double (`values = sum_g w_g values_g`).  Host queries ->
        `PosteriorExpectation` of float32 NumPy arrays; `max_score` equals one index holding all the rows bit for bit."""
        if isinstance(queries, torch.Tensor):
            queries = queries.detach().float().cpu().numpy()
        q = np.ascontiguousarray(queries)
        if q.dtype not in (np.float32, np.float16):
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        nq = int(q.shape[0])
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        shape = self.row_values_shape
        n_cols = shape[1] if shape else 0
        max_score = np.empty((nq,), dtype=np.float32)
        log_rel = np.empty((nq,), dtype=np.float32)
        values = np.empty((nq, max(n_cols, 1)), dtype=np.float32)[:, :n_cols]
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_posterior_expectation(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, beta, None if sub is None else sub.ctypes.data, n_sub,
                max_score.ctypes.data, log_rel.ctypes.data, values.ctypes.data))
        with np.errstate(invalid="ignore"):
            log_z = (max_score * np.float32(beta) + log_rel).astype(np.float32)
        return PosteriorExpectation(values, LogPartition(log_z, max_score, log_rel))

    def posterior_expectation_backward(self, queries, grad_values, expectation: "PosteriorExpectation", temperature: float = 1.0,
                                       subset: np.ndarray | None = None) -> np.ndarray:
        """`HipFlatIndex.posterior_expectation_backward` over every shard: each shard runs the flat call on its own rows with the GLOBAL
        `expectation` (what this index's `posterior_expectation` returned), so the shard results add; they are folded on the host in
        shard order, in double.  Host arrays -> a float32 NumPy array `[nq, dim]`."""
        if isinstance(queries, torch.Tensor):
            queries = queries.detach().float().cpu().numpy()
        q = np.ascontiguousarray(queries)
        if q.dtype not in (np.float32, np.float16):
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        nq = int(q.shape[0])
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])

        def host(a):
            return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)

        y, g = host(expectation.values), host(grad_values)
        if y.ndim != 2 or y.shape[0] != nq or g.shape != y.shape:
            raise ValueError(f"expected values and grad_values of one shape [{nq}, n_cols], got {tuple(y.shape)} and {tuple(g.shape)}")
        shape = self.row_values_shape
        if shape is not None and y.shape[1] != shape[1]:
            raise ValueError(f"expected grad_values of shape [{nq}, {shape[1]}] (the table's columns), got {tuple(g.shape)}")
        max_score, log_rel = host(expectation.log_partition.max_score), host(expectation.log_partition.log_rel)
        if max_score.shape != (nq,) or log_rel.shape != (nq,):
            raise ValueError(f"expected max_score and log_rel of shape ({nq},)")
        grad = np.empty((nq, self.dim), dtype=np.float32)
        spare = np.zeros(1, dtype=np.float32)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_posterior_expectation_backward(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, beta, None if sub is None else sub.ctypes.data, n_sub,
                max_score.ctypes.data, log_rel.ctypes.data, (y if y.size else spare).ctypes.data, (g if g.size else spare).ctypes.data,
                grad.ctypes.data))
        return grad

    def expected_values(self, queries: torch.Tensor, temperature: float = 1.0, subset=None) -> torch.Tensor:
        """`HipFlatIndex.expected_values` over every shard: a float32 `[nq, n_cols]` tensor on the device of `queries`, differentiable
        with respect to them (forward `posterior_expectation`, backward `posterior_expectation_backward`, both through the host)."""
        return _ExpectedValues.apply(queries, self, float(temperature), subset)

    def posterior_adjoint(self, queries, weights, log_partition: "LogPartition | None" = None, temperature: float = 1.0,
                          subset: np.ndarray | None = None, out: np.ndarray | None = None, accumulate: bool = False) -> np.ndarray:
        """`HipFlatIndex.posterior_adjoint` over every shard: each shard computes its own rows of `P^T W` on its own device from the
        GLOBAL `log_partition` (this index's, from any forward call; None runs `log_partition` first), and the slabs are concatenated:
        nothing is folded, and handed the words of one index holding all the rows the result equals that index's bit for bit.  Host
        arrays -> a float32 NumPy array `[ntotal, n_cols]`; `accumulate=True` adds the result to `out` on the host."""
        q = self._host_queries(queries)
        nq = int(q.shape[0])
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = self._host_subset(subset, nq)

        def host(a):
            return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)

        w = host(weights)
        w = np.ascontiguousarray(w.reshape(-1, 1) if w.ndim == 1 else w)
        if w.ndim != 2 or w.shape[0] != nq:
            raise ValueError(f"expected weights of shape [{nq}, n_cols], got {tuple(w.shape)}")
        n_cols = int(w.shape[1])
        if log_partition is None:
            log_partition = self.log_partition(q, temperature, sub)
        max_score, log_rel = host(log_partition.max_score), host(log_partition.log_rel)
        if max_score.shape != (nq,) or log_rel.shape != (nq,):
            raise ValueError(f"expected max_score and log_rel of shape ({nq},)")
        ntotal = self.ntotal
        if accumulate and out is None:
            raise ValueError("accumulate=True needs `out`")
        if out is not None and (out.shape != (ntotal, n_cols) or out.dtype != np.float32 or not out.flags.c_contiguous):
            raise ValueError(f"expected `out` a contiguous float32 [{ntotal}, {n_cols}] array")
        res = np.empty((ntotal, n_cols), dtype=np.float32) if out is None or accumulate else out
        spare = np.zeros(1, dtype=np.float32)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_posterior_adjoint(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, beta, None if sub is None else sub.ctypes.data, n_sub,
                max_score.ctypes.data, log_rel.ctypes.data, (w if w.size else spare).ctypes.data, n_cols, (res if res.size else spare).ctypes.data))
        if accumulate:
            out += res
            return out
        return res

    def row_mass(self, queries, temperature: float = 1.0, query_weights=None, subset=None, log_partition: "LogPartition | None" = None) -> np.ndarray:
        """`HipFlatIndex.row_mass` over every shard: a float32 NumPy array `[ntotal]`."""
        q = self._host_queries(queries)
        w = np.ones((q.shape[0],), dtype=np.float32) if query_weights is None else query_weights
        return self.posterior_adjoint(q, w, log_partition, temperature, subset).reshape(-1)

    def read_out(self, queries: torch.Tensor, values: torch.Tensor, temperature: float = 1.0, subset=None, keys=None) -> torch.Tensor:
        """`HipFlatIndex.read_out` over every shard: a float32 `[nq, n_cols]` tensor on the device of `queries`, differentiable in them
        and in `values` (every call through the host); `keys` as there."""
        if keys is None:
            return _ReadOut.apply(queries, values, self, float(temperature), subset)
        return _ReadOutKeys.apply(queries, values, _checked_keys(self, keys), self, float(temperature), subset)

    def key_gradient(self, queries, *, grad_log_z=None, grad_values=None, expectation: "PosteriorExpectation | None" = None,
                     log_partition: "LogPartition | None" = None, temperature: float = 1.0, subset: np.ndarray | None = None,
                     out: np.ndarray | None = None, accumulate: bool = False) -> np.ndarray:
        """`HipFlatIndex.key_gradient` over every shard: each shard computes its own rows on its own device from the GLOBAL forward
        words (this index's; with none handed in the forward runs first) and the batch-wide scales the node call forms once - the
        column maxima of the table are taken over all the shards - and the slabs are concatenated: nothing is folded, and handed the
        words of one index holding all the rows the result equals that index's bit for bit.  Host arrays -> a float32 NumPy array
        `[ntotal, dim]`; `accumulate=True` adds the result to `out` on the host."""
        q = self._host_queries(queries)
        nq = int(q.shape[0])
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = self._host_subset(subset, nq)

        def host(a):
            return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)

        a = g = y = None
        if grad_log_z is not None:
            a = host(grad_log_z).reshape(-1)
            if a.shape != (nq,):
                raise ValueError(f"expected grad_log_z of shape ({nq},), got {tuple(a.shape)}")
        if grad_values is not None:
            g = host(grad_values)
            if expectation is None and self.row_values_shape is not None:
                expectation = self.posterior_expectation(q, temperature, sub)
            if expectation is not None:
                y = host(expectation.values)
                if y.ndim != 2 or y.shape[0] != nq or g.shape != y.shape:
                    raise ValueError(f"expected values and grad_values of one shape [{nq}, n_cols], got {tuple(y.shape)} and {tuple(g.shape)}")
            shape = self.row_values_shape
            if shape is not None and (g.ndim != 2 or g.shape[1] != shape[1]):
                raise ValueError(f"expected grad_values of shape [{nq}, {shape[1]}] (the table's columns), got {tuple(g.shape)}")
        if expectation is not None and log_partition is None:
            log_partition = expectation.log_partition
        if log_partition is None:
            log_partition = self.log_partition(q, temperature, sub)
        max_score, log_rel = host(log_partition.max_score), host(log_partition.log_rel)
        if max_score.shape != (nq,) or log_rel.shape != (nq,):
            raise ValueError(f"expected max_score and log_rel of shape ({nq},)")
        ntotal = self.ntotal
        if accumulate and out is None:
            raise ValueError("accumulate=True needs `out`")
        if out is not None and (out.shape != (ntotal, self.dim) or out.dtype != np.float32 or not out.flags.c_contiguous):
            raise ValueError(f"expected `out` a contiguous float32 [{ntotal}, {self.dim}] array")
        res = np.empty((ntotal, self.dim), dtype=np.float32) if out is None or accumulate else out
        spare = np.zeros(1, dtype=np.float32)

        def ptr(t):
            return None if t is None else (t if t.size else spare).ctypes.data

        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_posterior_key_gradient(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, beta, None if sub is None else sub.ctypes.data, n_sub,
                max_score.ctypes.data, log_rel.ctypes.data, ptr(a), ptr(g if y is None else y), ptr(g), (res if res.size else spare).ctypes.data))
        if accumulate:
            out += res
            return out
        return res

    def sample_posterior(self, queries, k: int, temperature: float = 1.0, *, seed: int, query_offset: int = 0,
                         subset: np.ndarray | None = None) -> "PosteriorSample":
        """`HipFlatIndex.sample_posterior` over every shard: each shard draws with `id_base` = its first global row, the lists are merged
        on the host by (key desc, id asc) and `log_p` / `log_weight` recomputed in double from the folded `LogPartition`.  Host queries
        -> `PosteriorSample` of NumPy arrays; `ids`, `scores` and `keys` equal one index holding all the rows bit for bit."""
        if isinstance(queries, torch.Tensor):
            queries = queries.detach().float().cpu().numpy()
        q = np.ascontiguousarray(queries)
        if q.dtype not in (np.float32, np.float16):
            q = q.astype(np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        nq = int(q.shape[0])
        k = int(k)
        if not 1 <= k <= 255:
            raise ValueError(f"k must be in [1, 255], got {k}")
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed must be in [0, 2^64), got {seed}")
        beta = 1.0 / float(temperature) if temperature else float("nan")
        sub, n_sub = None, 0
        if subset is not None:
            sub = np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
            if sub.ndim != 2 or sub.shape[0] != nq:
                raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
            n_sub = int(sub.shape[1])
        max_score, log_rel = np.empty((nq,), dtype=np.float32), np.empty((nq,), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        scores, log_p, log_weight = (np.empty((nq, k), dtype=np.float32) for _ in range(3))
        keys = np.empty((nq, k + 1), dtype=np.float32)
        with torch.cuda.device(self.device):
            _native.check(self._lib.vodhip_node_index_sample_posterior(
                self._h, q.ctypes.data, 2 if q.dtype == np.float32 else 0, nq, k, beta, int(seed), int(query_offset),
                None if sub is None else sub.ctypes.data, n_sub, max_score.ctypes.data, log_rel.ctypes.data, ids.ctypes.data,
                scores.ctypes.data, log_p.ctypes.data, log_weight.ctypes.data, keys.ctypes.data))
        with np.errstate(invalid="ignore"):
            log_z = (max_score * np.float32(beta) + log_rel).astype(np.float32)
            log_tau = ((keys[:, k] - max_score * np.float32(beta)) - log_rel).astype(np.float32)
        log_tau[np.isnan(log_tau)] = -np.inf
        return PosteriorSample(ids, scores, log_p, log_weight, log_tau, keys, LogPartition(log_z, max_score, log_rel))

    def score_ids(self, queries, ids, k: int | None = None, *, subset=None, out=None):
        """`HipFlatIndex.score_ids` over every shard: `ids` are global row ids; results equal one index holding all the rows.
        NumPy queries -> NumPy results (host buffers); a tensor on `devices[0]` -> tensors there, complete on the current stream.
        `ids` / `subset` may be host arrays, ragged lists (ids) or tensors on `devices[0]` whatever the queries are."""
        nq = int(queries.shape[0])
        on_device = isinstance(queries, torch.Tensor)
        if on_device:
            if queries.device != self.device:
                raise ValueError(f"queries live on {queries.device}, the merge device is {self.device}")
            q = queries.contiguous()
            if q.dtype not in (torch.float16, torch.bfloat16, torch.float32):
                q = q.float()
            code = _native.torch_dtype_code(q.dtype)
        else:
            q = np.ascontiguousarray(queries)
            if q.dtype not in (np.float32, np.float16):
                q = q.astype(np.float32)
            code = 2 if q.dtype == np.float32 else 0
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"expected [nq, {self.dim}] queries, got {tuple(q.shape)}")
        if on_device:
            lst = ids.to(self.device, torch.int64).contiguous() if isinstance(ids, torch.Tensor) else torch.from_numpy(pad_listed_ids(ids, nq)).to(self.device)
            sub = None if subset is None else (subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))).to(self.device, torch.int32).contiguous()
        else:
            lst = pad_listed_ids(ids.cpu().numpy() if isinstance(ids, torch.Tensor) else ids, nq)
            sub = None if subset is None else np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
        if lst.ndim != 2 or lst.shape[0] != nq:
            raise ValueError(f"expected ids of shape [{nq}, m], got {tuple(lst.shape)}")
        if sub is not None and (sub.ndim != 2 or sub.shape[0] != nq):
            raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
        m = int(lst.shape[1])
        n_sub = 0 if sub is None else int(sub.shape[1])
        ptr = (lambda t: None if t is None else t.data_ptr()) if on_device else (lambda a: None if a is None else a.ctypes.data)
        shape = (nq, m) if k is None else (nq, int(k))
        if out is not None:
            scores, top = (out, None) if k is None else out
        elif on_device:
            scores = torch.empty(shape, dtype=torch.float32, device=self.device)
            top = None if k is None else torch.empty(shape, dtype=torch.int64, device=self.device)
        else:
            scores = np.empty(shape, dtype=np.float32)
            top = None if k is None else np.empty(shape, dtype=np.int64)
        loc = _native.DEVICE if on_device else _native.HOST
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device) if on_device else None
            if k is None:
                _native.check(self._lib.vodhip_node_index_score_ids(self._h, ptr(q), code, nq, ptr(lst), m, ptr(sub), n_sub, loc, ptr(scores), stream))
                return scores
            _native.check(self._lib.vodhip_node_index_search_ids(self._h, ptr(q), code, nq, ptr(lst), m, int(k), ptr(sub), n_sub, loc,
                                                                 ptr(scores), ptr(top), stream))
        return scores, top

    def sum_ids(self, ids, weights, *, subset=None, out=None):
        """`HipFlatIndex.sum_ids` over every shard: `ids` are global row ids; every shard sums the rows it owns, the per-shard sums are
        added on `devices[0]` in increasing shard order - deterministic for a given sharding, the flat index's bits where every sum is
        exact.  `weights` a tensor on `devices[0]` -> a tensor there, complete on the current stream; host weights (NumPy, a CPU tensor,
        ragged lists) -> a NumPy array.  `ids` / `subset` may be host arrays, ragged lists (ids) or tensors whatever the weights are."""
        on_device = isinstance(weights, torch.Tensor) and weights.is_cuda
        if on_device:
            if weights.device != self.device:
                raise ValueError(f"weights live on {weights.device}, the merge device is {self.device}")
            lst = ids.to(self.device, torch.int64).contiguous() if isinstance(ids, torch.Tensor) else torch.from_numpy(pad_listed_ids(ids)).to(self.device)
            w = weights.to(torch.float32).contiguous()
            sub = None if subset is None else (subset if isinstance(subset, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(subset))).to(self.device, torch.int32).contiguous()
        else:
            lst = pad_listed_ids(ids.cpu().numpy() if isinstance(ids, torch.Tensor) else ids)
            w = pad_listed_weights(weights.detach().float().numpy() if isinstance(weights, torch.Tensor) else weights, lst.shape)
            sub = None if subset is None else np.ascontiguousarray(subset.cpu().numpy() if isinstance(subset, torch.Tensor) else subset, dtype=np.int32)
        if lst.ndim != 2:
            raise ValueError(f"expected ids of shape [nq, m], got {tuple(lst.shape)}")
        nq, m = int(lst.shape[0]), int(lst.shape[1])
        if tuple(w.shape) != (nq, m):
            raise ValueError(f"expected weights of shape {(nq, m)}, got {tuple(w.shape)}")
        if sub is not None and (sub.ndim != 2 or sub.shape[0] != nq):
            raise ValueError(f"subset must be int32 [nq, n_per_query], got {tuple(sub.shape)}")
        n_sub = 0 if sub is None else int(sub.shape[1])
        ptr = (lambda t: None if t is None else t.data_ptr()) if on_device else (lambda a: None if a is None else a.ctypes.data)
        if out is not None:
            res = out
        elif on_device:
            res = torch.empty((nq, self.dim), dtype=torch.float32, device=self.device)
        else:
            res = np.empty((nq, self.dim), dtype=np.float32)
        with torch.cuda.device(self.device):
            stream = _native.current_stream_ptr(self.device) if on_device else None
            _native.check(self._lib.vodhip_node_index_sum_ids(self._h, ptr(lst), ptr(w), nq, m, ptr(sub), n_sub,
                                                              _native.DEVICE if on_device else _native.HOST, ptr(res), stream))
        return res

    def listed_scores(self, queries: torch.Tensor, ids, *, subset=None) -> torch.Tensor:
        """`HipFlatIndex.listed_scores` over every shard: the bits of `score_ids`, differentiable (once) with respect to `queries`;
        backward is this index's `sum_ids`.  The scores live on `devices[0]` (queries elsewhere are copied there); the gradient arrives
        in the dtype and on the device of `queries`."""
        if not isinstance(ids, torch.Tensor):
            ids = torch.from_numpy(pad_listed_ids(ids, int(queries.shape[0]))).to(self.device)
        return _ListedScores.apply(queries.to(self.device), self, ids, {"subset": subset})
