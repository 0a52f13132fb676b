"""Retrieval metrics on the GPU (host wrapper over `vodhip_retrieval_metrics`).

Mirror of `RetrievalMonitor` (the reference's src/vod_models/monitoring/monitor.py:35-117) with its `MeanAggregator`s
(aggregator.py:26-59) and of the `compute_*` classes (functional.py:181-254): same metric names, same `update(batch,
model_output)` / `get()` / `reset()` / `synchronize()` / `compute()` interface, same values.  The reference ranks once with
argsort + two gathers, runs a dozen small kernels per metric and synchronises with the host once per metric (the boolean
index in `MeanAggregator.update`); here one update is two launches - a row kernel that ranks each row once and evaluates
every (metric, topk), and a fixed-order float64 reduction into the packed `[M, 2]` (total, count) state - with no host
synchronisation, so the update can be captured into the hipGraph of `GraphedRetrievalStep` behind the loss.

There is no CPU path: the scores must be device tensors.
"""
from __future__ import annotations

import ctypes
import typing as typ

import torch

from vod_amd import _native

# VODHIP_METRIC_* of include/vodhip.h
METRIC_IDS: dict[str, int] = {"mrr": 0, "hitrate": 1, "precision": 2, "recall": 3, "ndcg": 4, "kldiv": 5, "min": 6, "max": 7, "entropy": 8}
MAX_SPECS = 32  # VODHIP_MAX_METRIC_SPECS
MAX_WIDTH = 4096


def parse_metric_name(name: str) -> tuple[str, None | int]:
    """`"hitrate_01"` -> ("hitrate", 1), `"kldiv"` -> ("kldiv", None); an unknown metric raises KeyError (monitor.py:108-117)."""
    if "_" in name:
        *parts, k = name.split("_")
        top_k: None | int = int(k)
        name = "_".join(parts)
    else:
        top_k = None
    if name not in METRIC_IDS:
        raise KeyError(name)
    return name, top_k


def _field(obj: typ.Any, key: str) -> typ.Any:
    if isinstance(obj, typ.Mapping):
        return obj[key]
    return getattr(obj, key)


def _as(t: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    return t if (t.dtype is dt and t.is_contiguous()) else t.to(dt).contiguous()


class _Specs:
    """The host-side (metric, topk) list of one call."""

    def __init__(self, ops: typ.Iterable[tuple[str, None | int]]):
        ops = list(ops)
        if not 1 <= len(ops) <= MAX_SPECS:
            raise ValueError(f"between 1 and {MAX_SPECS} metrics per monitor, got {len(ops)}")
        flat: list[int] = []
        for name, topk in ops:
            if topk is not None and topk < 0:
                raise ValueError(f"negative topk for `{name}`")
            flat += [METRIC_IDS[name], int(topk or 0)]
        self.n = len(ops)
        self.array = (ctypes.c_int32 * len(flat))(*flat)


def _launch(scores: torch.Tensor, relevances: torch.Tensor, specs: _Specs, values: torch.Tensor | None, state: torch.Tensor | None) -> None:
    lib = _native.load_library()
    B, width = scores.shape
    dev = scores.device
    if torch.cuda.current_device() == dev.index:
        _native.check(lib.vodhip_retrieval_metrics(
            scores.data_ptr(), relevances.data_ptr(), B, width, specs.array, specs.n,
            None if values is None else values.data_ptr(), None if state is None else state.data_ptr(), None, 0,
            _native.current_stream_ptr(dev)))
        return
    with torch.cuda.device(dev):
        _launch(scores, relevances, specs, values, state)


def _inputs(relevances: torch.Tensor, scores: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    if not scores.is_cuda:
        raise _native.NativeLibraryError("retrieval metrics need device tensors (there is no CPU path)")
    if scores.shape != relevances.shape or scores.dim() < 1:
        raise ValueError(f"scores {tuple(scores.shape)} and relevances {tuple(relevances.shape)} must have the same shape")
    width = scores.shape[-1]
    if not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"rows of 1..{MAX_WIDTH} sections, got {width}")
    sc = _as(scores.detach(), torch.float32).reshape(-1, width)
    rl = _as(relevances.to(scores.device), torch.int64).reshape(-1, width)
    if sc.shape[0] < 1:
        raise ValueError("empty batch")
    return rl, sc


def compute_metrics(relevances: torch.Tensor, scores: torch.Tensor, metrics: typ.Sequence[str]) -> dict[str, torch.Tensor]:
    """Per-row values of every metric name, `dict[name, Tensor[B]]`: the counterpart of `functional.compute_*.compute` (float32;
    `hitrate` is bool, as in the reference)."""
    ops = {m: parse_metric_name(m) for m in metrics}
    rl, sc = _inputs(relevances, scores)
    specs = _Specs(ops.values())
    values = torch.empty((specs.n, sc.shape[0]), dtype=torch.float32, device=sc.device)
    _launch(sc, rl, specs, values, None)
    lead = scores.shape[:-1]
    return {m: (values[i] != 0 if base == "hitrate" else values[i]).reshape(lead) for i, (m, (base, _)) in enumerate(ops.items())}


class RetrievalMonitor:
    """Monitor retrieval performances: running means of retrieval metrics, computed and aggregated on the device."""

    def __init__(self, metrics: list[str]) -> None:
        self.ops: dict[str, tuple[str, None | int]] = {m: parse_metric_name(m) for m in metrics}
        self._specs = _Specs(self.ops.values())
        self._state: torch.Tensor | None = None     # float64 [M, 2]: (total, count) of every metric
        self._values: dict[tuple, torch.Tensor] = {}  # (device index, B) -> float32 [M, B] row values of the last update

    # ---- placement ------------------------------------------------------------------------------------------------------
    @property
    def state(self) -> torch.Tensor | None:
        """The packed float64 `[M, 2]` (total, count) state, or None before the first update / `to(device)`."""
        return self._state

    def to(self, device: typ.Any = None, dtype: torch.dtype | None = None) -> "RetrievalMonitor":  # noqa: ARG002
        """Place the state on `device`.  The state is float64 whatever `dtype` says (the training loop asks for float64,
        vod_ops/loops/train.py:59)."""
        if device is not None:
            self._place(torch.device(device))
        return self

    def _place(self, dev: torch.device) -> torch.Tensor:
        if dev.type != "cuda":
            raise _native.NativeLibraryError("RetrievalMonitor lives on the device (there is no CPU path)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._state is None:
            self._state = torch.zeros((self._specs.n, 2), dtype=torch.float64, device=dev)
        elif self._state.device != dev:
            self._state = self._state.to(dev)
            self._values.clear()
        return self._state

    # ---- the reference's interface -----------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, batch: typ.Any, model_output: typ.Any) -> None:
        """Compute every metric of the batch and add it to the running state: two launches, no host synchronisation."""
        rl, sc = _inputs(_field(batch, "section__relevance"), _field(model_output, "retriever_scores"))
        state = self._place(sc.device)
        key = (sc.device.index, sc.shape[0])
        values = self._values.get(key)
        if values is None:
            # (kept for the monitor's lifetime: a captured graph replays on this buffer)
            values = self._values[key] = torch.empty((self._specs.n, sc.shape[0]), dtype=torch.float32, device=sc.device)
        _launch(sc, rl, self._specs, values, state)

    def synchronize(self) -> None:
        """Sum the state over the ranks: ONE all-reduce of the packed `[M, 2]` state (the reference: a barrier + 2 M all-reduces)."""
        import torch.distributed as dist

        if self._state is None or not (dist.is_available() and dist.is_initialized()):
            return
        if dist.get_backend() == "gloo":  # no device collectives: the 16 * M bytes are staged through the host
            host = self._state.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM)
            self._state.copy_(host)
        else:
            dist.all_reduce(self._state, op=dist.ReduceOp.SUM)

    def reset(self) -> None:
        if self._state is not None:
            self._state.zero_()

    def get(self) -> dict[str, torch.Tensor]:
        """`{name: total / count}` as 0-dim float64 device tensors (NaN for a metric that never saw a non-NaN value)."""
        if self._state is None:
            return {name: torch.tensor(float("nan"), dtype=torch.float64) for name in self.ops}
        mean = self._state[:, 0] / self._state[:, 1]
        return {name: mean[i] for i, name in enumerate(self.ops)}

    def compute(self, synchronize: bool = True) -> dict[str, torch.Tensor]:
        """Sync, get values and reset."""
        if synchronize:
            self.synchronize()
        out = self.get()
        self.reset()
        return out

    def last_values(self, batch_size: int, device: typ.Any = None) -> dict[str, torch.Tensor]:
        """The per-row float32 values of the last update of `batch_size` rows (views of the monitor's buffer)."""
        idx = torch.device(device).index if device is not None else (self._state.device.index if self._state is not None else None)
        values = self._values[(idx, int(batch_size))]
        return {name: values[i] for i, name in enumerate(self.ops)}
