"""`VodPooler`: the encoder's pooling head (sequence pooling, activation, norm, scale) fused on the GPU, forward and backward.

Mirror of the reference's `VodPooler` (src/vod_models/vod_encoder/modeling.py:63-181): the same constructor arguments, the same
keyword-only `forward(hidden_states, *, attention_mask)`, the same state-dict keys, so that a reference checkpoint loads with
`strict=True`.  The kernels are in vod_amd/csrc/kernels_pool.hip (C-ABI section H5p of include/vodhip.h).

Two things differ from the reference, on purpose:
  * `mask_mode`.  The reference's mean aggregator sums EVERY position, padded ones included, and divides by the number of live ones.
    `mask_mode="reference"` (the default) is that arithmetic; `mask_mode="masked"` sums the live positions only and does not read the
    padded token rows at all.
  * a row without a live token gets a zero gradient (the reference's backward gives 0 / 0 = NaN for that row).
The reference's "max" aggregator returns a [N, 1, 1] tensor (its gather index lacks the hidden dimension) and "none" does not pool:
neither is offered.
"""
from __future__ import annotations

import math
import typing as typ

import torch
from torch import nn

from vod_amd import _native
from vod_amd.gradients import _on_device

AGG_CODES = {"mean": 0, "cls": 1}
MASK_MODES = {"reference": 0, "masked": 1}
ACT_CODES = {None: 0, "relu": 1, "tanh": 2, "sigmoid": 3, "gelu": 4}
NORM_CODES = {None: 0, "l2": 1, "l1": 2}
_FLOATS = (torch.float16, torch.bfloat16, torch.float32)
_CONFIG_FIELDS = ("projection_size", "output_activation", "output_norm", "agg_method", "scaler", "learn_scaler")
_CONFIG_DEFAULTS = {"projection_size": None, "output_activation": None, "output_norm": None, "agg_method": "mean", "scaler": 1.0,
                    "learn_scaler": False}


def _as(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    return (x if x.dtype is dtype else x.to(dtype)).contiguous()


def _device_mask(mask: torch.Tensor) -> torch.Tensor:
    # the kernels test a mask element for any set bit: bool and integer masks are read as they are
    m = mask if not (mask.is_floating_point() or mask.is_complex()) else mask != 0
    return m.contiguous()


def _scale_word(log_scaler: torch.Tensor) -> torch.Tensor:
    return _as(log_scaler.detach().reshape(1), torch.float32)


class _PoolAggregate(torch.autograd.Function):
    """hidden [N, L, H] -> y [N, H] (`finish`: aggregate, activation, norm and scale in one call) or a [N, H] float32 (aggregate only)."""

    @staticmethod
    def forward(ctx, hidden, mask, log_scaler, agg, mode, finish, act, norm, out_dtype, l_chunk):  # noqa: ANN001
        lib = _native.load_library()
        N, L, H = hidden.shape
        hdt = hidden.dtype if hidden.dtype in _FLOATS else torch.float32
        x = _as(hidden, hdt)
        m = _device_mask(mask)
        dev = x.device
        ls = _scale_word(log_scaler)
        a = torch.empty((N, H), dtype=torch.float32, device=dev)
        y = torch.empty((N, H), dtype=out_dtype, device=dev) if finish else None
        with _on_device(dev):
            n_work = 0 if agg == AGG_CODES["cls"] else int(lib.vodhip_pool_workspace_floats(N, L, H, l_chunk))
            if n_work < 0:
                _native.check(-1)
            work = torch.empty((n_work,), dtype=torch.float32, device=dev) if n_work else None
            _native.check(
                lib.vodhip_pool_forward(
                    x.data_ptr(), _native.torch_dtype_code(hdt), N, L, H, m.data_ptr(), m.element_size(), agg, mode, int(finish), act,
                    norm, ls.data_ptr(), l_chunk, a.data_ptr(), y.data_ptr() if finish else None,
                    _native.torch_dtype_code(out_dtype) if finish else 0, work.data_ptr() if n_work else None, n_work,
                    _native.current_stream_ptr(dev),
                )
            )
        ctx.save_for_backward(m, a, ls)
        ctx.meta = (N, L, H, hdt, hidden.dtype, agg, mode, finish, act, norm, l_chunk, log_scaler.dtype)
        return y if finish else a

    @staticmethod
    def backward(ctx, g):  # noqa: ANN001
        lib = _native.load_library()
        m, a, ls = ctx.saved_tensors
        N, L, H, hdt, in_dt, agg, mode, finish, act, norm, l_chunk, ls_dt = ctx.meta
        dev = a.device
        gdt = g.dtype if (finish and g.dtype in _FLOATS) else torch.float32
        gc = _as(g, gdt)
        d_hidden = d_ls = None
        need_ls = finish and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[0] or need_ls:
            d_hidden = torch.empty((N, L, H), dtype=hdt, device=dev)  # the one hidden-sized tensor of the backward
            gy = torch.empty((N,), dtype=torch.float32, device=dev) if finish else None
            with _on_device(dev):
                _native.check(
                    lib.vodhip_pool_backward(
                        gc.data_ptr(), _native.torch_dtype_code(gdt), a.data_ptr(), N, L, H, m.data_ptr(), m.element_size(), agg, mode,
                        int(finish), act, norm, ls.data_ptr(), l_chunk, d_hidden.data_ptr(), _native.torch_dtype_code(hdt),
                        gy.data_ptr() if finish else None, _native.current_stream_ptr(dev),
                    )
                )
            if need_ls:
                d_ls = (0.5 * gy.sum()).to(ls_dt)
            d_hidden = d_hidden if in_dt is hdt else d_hidden.to(in_dt)
        return d_hidden, None, d_ls, None, None, None, None, None, None, None


class _PoolFinish(torch.autograd.Function):
    """z [N, P] -> y [N, P]: activation, norm and scale, behind the projection."""

    @staticmethod
    def forward(ctx, z, log_scaler, act, norm, out_dtype):  # noqa: ANN001
        lib = _native.load_library()
        N, P = z.shape
        zdt = z.dtype if z.dtype in _FLOATS else torch.float32
        zc = _as(z, zdt)
        dev = zc.device
        ls = _scale_word(log_scaler)
        y = torch.empty((N, P), dtype=out_dtype, device=dev)
        with _on_device(dev):
            _native.check(
                lib.vodhip_pool_finish_forward(
                    zc.data_ptr(), _native.torch_dtype_code(zdt), N, P, act, norm, ls.data_ptr(), y.data_ptr(),
                    _native.torch_dtype_code(out_dtype), _native.current_stream_ptr(dev),
                )
            )
        ctx.save_for_backward(zc, ls)
        ctx.meta = (N, P, zdt, z.dtype, act, norm, log_scaler.dtype)
        return y

    @staticmethod
    def backward(ctx, g):  # noqa: ANN001
        lib = _native.load_library()
        zc, ls = ctx.saved_tensors
        N, P, zdt, in_dt, act, norm, ls_dt = ctx.meta
        dev = zc.device
        gdt = g.dtype if g.dtype in _FLOATS else torch.float32
        gc = _as(g, gdt)
        dz = torch.empty((N, P), dtype=zdt, device=dev)
        gy = torch.empty((N,), dtype=torch.float32, device=dev)
        with _on_device(dev):
            _native.check(
                lib.vodhip_pool_finish_backward(
                    zc.data_ptr(), _native.torch_dtype_code(zdt), gc.data_ptr(), _native.torch_dtype_code(gdt), N, P, act, norm,
                    ls.data_ptr(), dz.data_ptr(), _native.torch_dtype_code(zdt), gy.data_ptr(), _native.current_stream_ptr(dev),
                )
            )
        d_ls = (0.5 * gy.sum()).to(ls_dt) if ctx.needs_input_grad[1] else None
        return (dz if in_dt is zdt else dz.to(in_dt)), d_ls, None, None, None


class _Aggregator(nn.Module):
    """Holds the reference aggregators' one parameter, so that `aggregator._dtype_marker` is in the state dict."""

    def __init__(self, method: str) -> None:
        super().__init__()
        self.method = method
        self._dtype_marker = nn.Parameter(torch.zeros(1), requires_grad=False)

    def extra_repr(self) -> str:
        return self.method


class VodPooler(nn.Module):
    """Pool the hidden states of a transformer encoder: `[..., L, H]` and a `[..., L]` mask give `[..., P]` encodings.

    `config` is a dict or an object with the reference's six fields (projection_size, output_activation, output_norm, agg_method,
    scaler, learn_scaler).  Without a projection the whole head is ONE launch forward (two when L is cut into chunks, see `l_chunk`)
    and one backward; with a projection it is aggregate -> `nn.Linear` (torch) -> finish.  `out_dtype` selects the dtype of the
    encodings (default: the dtype of `hidden_states`, or of the projection's output), e.g. float16 to feed `HipFlatIndex.add`
    without a cast.  `l_chunk` forces the tokens per workgroup (default: chosen from the shape alone).
    There is no CPU path: tensors that are not on one ROCm device are refused.
    """

    def __init__(self, config: typ.Any, backbone_output_size: int, *, mask_mode: str = "reference",
                 out_dtype: torch.dtype | None = None, l_chunk: int | None = None) -> None:
        super().__init__()
        if isinstance(config, dict):
            unknown = set(config) - set(_CONFIG_FIELDS)
            if unknown:
                raise ValueError(f"unknown pooler config fields {sorted(unknown)}; expected {list(_CONFIG_FIELDS)}")
            conf = {**_CONFIG_DEFAULTS, **config}
        else:
            conf = {k: getattr(config, k) for k in _CONFIG_FIELDS}
        agg = conf["agg_method"]
        if agg == "max":
            raise ValueError("agg_method='max' is not supported: the reference's MaxAgg gathers with an index of shape [N, 1, 1] and "
                             "returns [N, 1, 1] instead of a pooled [N, H] vector, so there is no behaviour to reproduce")
        if agg == "none":
            raise ValueError("agg_method='none' is not supported: the reference's IdentityAgg returns the hidden states unpooled, "
                             "it is not a pooling")
        if agg not in AGG_CODES:
            raise ValueError(f"unknown agg_method {agg!r}; expected 'mean' or 'cls'")
        if conf["output_activation"] not in ACT_CODES:
            raise ValueError(f"unknown output_activation {conf['output_activation']!r}; expected None, 'relu', 'tanh', 'sigmoid' or 'gelu'")
        if conf["output_norm"] not in NORM_CODES:
            raise ValueError(f"unknown output_norm {conf['output_norm']!r}; expected None, 'l2' or 'l1'")
        if mask_mode not in MASK_MODES:
            raise ValueError(f"unknown mask_mode {mask_mode!r}; expected 'reference' or 'masked'")
        if out_dtype is not None and out_dtype not in _FLOATS:
            raise ValueError(f"out_dtype must be float16, bfloat16 or float32, got {out_dtype}")
        if l_chunk is not None and int(l_chunk) < 1:
            raise ValueError("l_chunk must be a positive number of tokens (or None)")
        self.config = conf
        self.backbone_output_size = int(backbone_output_size)
        self.mask_mode = mask_mode
        self.out_dtype = out_dtype
        self.l_chunk = 0 if l_chunk is None else int(l_chunk)
        self.aggregator = _Aggregator(agg)
        if conf["projection_size"] is None:
            self.output_vector_size = self.backbone_output_size
            self.projection = None
        else:
            self.output_vector_size = int(conf["projection_size"])
            self.projection = nn.Linear(self.backbone_output_size, self.output_vector_size)
        self.log_scaler = nn.Parameter(torch.tensor(float(conf["scaler"])).log(), requires_grad=bool(conf["learn_scaler"]))
        self._codes = (AGG_CODES[agg], MASK_MODES[mask_mode], ACT_CODES[conf["output_activation"]], NORM_CODES[conf["output_norm"]])

    def get_encoding_shape(self) -> tuple[int, ...]:
        return (self.output_vector_size,)

    def extra_repr(self) -> str:
        c = self.config
        return (f"agg={c['agg_method']}, activation={c['output_activation']}, norm={c['output_norm']}, scaler={c['scaler']}, "
                f"mask_mode={self.mask_mode}")

    def forward(self, hidden_states: torch.Tensor, *, attention_mask: torch.Tensor) -> torch.Tensor:
        if not hidden_states.is_cuda:
            raise _native.NativeLibraryError("VodPooler needs device tensors (there is no CPU path)")
        dev = hidden_states.device
        others = [("attention_mask", attention_mask), ("log_scaler", self.log_scaler)]
        if self.projection is not None:
            others.append(("projection.weight", self.projection.weight))
        for name, x in others:
            if x.device != dev:  # the kernels get raw pointers: a host or other-device tensor must never reach them
                raise _native.NativeLibraryError(f"`{name}` is on {x.device}, `hidden_states` on {dev}: all tensors must share one GPU")
        if hidden_states.dim() < 2 or hidden_states.shape[-1] != self.backbone_output_size:
            raise ValueError(f"`hidden_states` must be [..., L, {self.backbone_output_size}], got {tuple(hidden_states.shape)}")
        lead, (L, H) = hidden_states.shape[:-2], hidden_states.shape[-2:]
        if attention_mask.shape != hidden_states.shape[:-1]:
            raise ValueError(f"`attention_mask` must be {tuple(hidden_states.shape[:-1])}, got {tuple(attention_mask.shape)}")
        N = math.prod(lead)
        if N == 0 or L == 0:
            raise ValueError(f"`hidden_states` {tuple(hidden_states.shape)} has no rows or no positions")
        x = hidden_states.reshape(N, L, H)
        m = attention_mask.reshape(N, L)
        agg, mode, act, norm = self._codes
        if self.projection is None:
            out_dt = self.out_dtype or (x.dtype if x.dtype in _FLOATS else torch.float32)
            y = _PoolAggregate.apply(x, m, self.log_scaler, agg, mode, True, act, norm, out_dt, self.l_chunk)
        else:
            a = _PoolAggregate.apply(x, m, self.log_scaler, agg, mode, False, 0, 0, torch.float32, self.l_chunk)
            z = self.projection(a.to(self.projection.weight.dtype))
            out_dt = self.out_dtype or (z.dtype if z.dtype in _FLOATS else torch.float32)
            y = _PoolFinish.apply(z, self.log_scaler, act, norm, out_dt)
        return y.reshape(*lead, self.output_vector_size)
