"""In-batch retrieval scoring + loss, and the marginal likelihood and the Renyi VOD objective through the reader LM, on the GPU (host
wrappers over `vodhip_retrieval_forward/backward` and `vodhip_lm_token_logprob_forward/backward` + `vodhip_marginal_forward` /
`vodhip_vod_forward`).

Mirror of `RetrievalGradients` (/root/reference/src/vod_models/vod_gradients/retrieval.py:14-92): same
constructor, same keyword-only call `(batch, query_encoding, section_encoding)`, same outputs (`loss`,
`retriever_scores`, `diagnostics` with kl_score / kl_sparse / kl_dense).  The ~15 torch kernels of the
reference's forward (einsum, masked_fill, log_softmax, targets, loss, three KLs) and the autograd backward
become one fused forward launch (+ finalize) and two backward launches, wrapped in a
`torch.autograd.Function` so `loss.backward()` keeps working.  The auxiliary losses (guidance,
self-supervision, score decay: retrieval.py:94-150; all weight 0 in the shipped config) are extra terms of the same
row kernel: values in `diagnostics`, gradients folded into the same dLoss/dScores.
"""
from __future__ import annotations

import dataclasses
import math
import typing as typ

import torch

from vod_amd import _native


@dataclasses.dataclass
class RealmOutput:
    """`loss`, `retriever_scores [B, D]`, `diagnostics` -- fields of the reference's RealmOutput (vod_types/batch.py:106-114)."""

    loss: torch.Tensor
    retriever_scores: torch.Tensor
    diagnostics: dict[str, typ.Any] = dataclasses.field(default_factory=dict)


_ENC = (torch.float16, torch.bfloat16, torch.float32)
_scratch: dict = {}  # (device index, stream, floats) -> the forward's device scratch (row words + split-K slabs), consumed in stream order


def _as(t: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """`t` itself when it already has the dtype and layout the kernels read (no new tensor object: this sits on a ~100 us host path)."""
    return t if (t.dtype is dt and t.is_contiguous()) else t.to(dt).contiguous()


class _on_device:
    """`torch.cuda.device(dev)` only when `dev` is not current already (the context manager costs ~5 us per entry)."""

    __slots__ = ("ctx",)

    def __init__(self, dev: torch.device):
        self.ctx = None if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            self.ctx.__exit__(*exc)


class _RetrievalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, s, score, relevance, sparse, dense, aux_cfg=(0, 0.0, 0.0, 0.0)):  # noqa: ANN001
        lib = _native.load_library()
        if not q.is_cuda:
            raise _native.NativeLibraryError("RetrievalGradients needs device tensors (there is no CPU path)")
        enc = q.dtype if q.dtype in _ENC else torch.float32
        qc, sc = _as(q, enc), _as(s, enc)  # (autograd is off inside `forward`: no detach needed)
        three_d = sc.dim() == 3
        if sc.dim() not in (2, 3):
            raise ValueError(f"Invalid dimension for `section_encoding`: {tuple(sc.shape)}")
        B, H = qc.shape
        D = sc.shape[1] if three_d else sc.shape[0]
        score_c, rel_c = _as(score, torch.float32), _as(relevance, torch.int64)
        if score_c.shape != (B, D) or rel_c.shape != (B, D):
            raise ValueError(f"section__score / section__relevance must be [{B}, {D}]")
        sparse_c = None if sparse is None else _as(sparse, torch.float32)
        dense_c = None if dense is None else _as(dense, torch.float32)
        dev = q.device
        stream = _native.current_stream_ptr(dev)
        # outputs: retriever scores | dLoss/dScores, and loss [1] | kl [3] | auxiliary terms [3] (NaN where the weight is 0) - fresh per
        # call (the caller keeps them); the kernels' scratch (16 row words per query + the split-K slabs of the in-batch contraction)
        # is cached per (device, stream, size): the next forward on the stream runs after this one has consumed it
        both = torch.empty((2, B, D), dtype=torch.float32, device=dev)
        small = torch.empty((8,), dtype=torch.float32, device=dev)
        n_work = 16 * B + (4 * B * D if not three_d else 0)
        if torch.cuda.is_current_stream_capturing():
            # under hipGraph capture the scratch must come from the graph's own pool (and must not leak into the cache)
            work = torch.empty((n_work,), dtype=torch.float32, device=dev)
        else:
            key = (dev.index, stream, n_work)
            work = _scratch.get(key)
            if work is None:
                if len(_scratch) > 64:
                    _scratch.clear()
                work = _scratch[key] = torch.empty((n_work,), dtype=torch.float32, device=dev)
        g_type, w_g, w_ss, w_sd = aux_cfg
        aux_grad = torch.empty((3, B, D), dtype=torch.float32, device=dev) if (w_g > 0 or w_ss > 0 or w_sd > 0) else None
        p_both, p_small = both.data_ptr(), small.data_ptr()
        with _on_device(dev):
            _native.check(
                lib.vodhip_retrieval_forward_aux(
                    qc.data_ptr(), sc.data_ptr(), _native.torch_dtype_code(enc), int(three_d), B, D, H,
                    score_c.data_ptr(), rel_c.data_ptr(),
                    None if sparse_c is None else sparse_c.data_ptr(), None if dense_c is None else dense_c.data_ptr(),
                    int(g_type), float(w_g), float(w_ss), float(w_sd),
                    p_both, p_both + 4 * B * D, p_small, p_small + 4, p_small + 16,
                    None if aux_grad is None else aux_grad.data_ptr(), work.data_ptr(), n_work, stream,
                )
            )
        scores, d_scores = both[0], both[1]
        ctx.save_for_backward(qc, sc, d_scores)
        ctx.meta = (enc, three_d, B, D, H, q.dtype, s.dtype)
        loss, kl, aux = small[0], small[1:4], small[4:7]
        ctx.mark_non_differentiable(scores, kl, aux)
        return loss, scores, kl, aux

    @staticmethod
    def backward(ctx, g_loss, _g_scores, _g_kl, _g_aux):  # noqa: ANN001
        lib = _native.load_library()
        qc, sc, d_scores = ctx.saved_tensors
        enc, three_d, B, D, H, q_dt, s_dt = ctx.meta
        dev = qc.device
        go = g_loss if (g_loss.dtype is torch.float32 and g_loss.is_contiguous()) else g_loss.float().contiguous()
        dq = torch.empty((B, H), dtype=torch.float32, device=dev)
        ds = torch.empty(sc.shape, dtype=torch.float32, device=dev)
        with _on_device(dev):
            _native.check(
                lib.vodhip_retrieval_backward(
                    qc.data_ptr(), sc.data_ptr(), _native.torch_dtype_code(enc), int(three_d), B, D, H,
                    d_scores.data_ptr(), go.data_ptr(), dq.data_ptr(), ds.data_ptr(), _native.current_stream_ptr(dev),
                )
            )
        return (dq if q_dt is torch.float32 else dq.to(q_dt)), (ds if s_dt is torch.float32 else ds.to(s_dt)), None, None, None, None, None


class RetrievalGradients:
    """KL-style retrieval objective with in-batch scoring, fused on the GPU."""

    def __init__(self, guidance: str = "zero", guidance_weight: float = 0.0, self_supervision_weight: float = 0.0,
                 score_decay: float = 0.0):
        if guidance not in ("zero", "sparse"):
            raise ValueError(f"guidance must be 'zero' or 'sparse', got {guidance!r}")  # the reference's GuidanceType (:11)
        self.guidance = guidance
        self.guidance_weight = guidance_weight
        self.self_supervision_weight = self_supervision_weight
        self.score_decay = score_decay

    def __call__(self, *, batch: typ.Any, query_encoding: torch.Tensor, section_encoding: torch.Tensor,
                 lm_logits: None | torch.Tensor = None) -> RealmOutput:  # noqa: ARG002
        get = (lambda k: batch.get(k)) if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
        loss, scores, kl, aux = _RetrievalLoss.apply(
            query_encoding, section_encoding, get("section__score"), get("section__relevance"),
            get("section__sparse"), get("section__dense"),
            (1 if self.guidance == "sparse" else 0, float(self.guidance_weight), float(self.self_supervision_weight), float(self.score_decay)),
        )
        diagnostics = {}
        if self.guidance_weight > 0:  # insertion order and keys of the reference's `_auxiliary_losses` (:104-118)
            diagnostics[f"{self.guidance}_guidance"] = aux[0]
        if self.self_supervision_weight > 0:
            diagnostics["self_supervision"] = aux[1]
        if self.score_decay > 0:
            diagnostics["score_decay"] = aux[2]
        diagnostics["kl_score"] = kl[0]
        if get("section__sparse") is not None:
            diagnostics["kl_sparse"] = kl[1]
        if get("section__dense") is not None:
            diagnostics["kl_dense"] = kl[2]
        return RealmOutput(loss=loss, retriever_scores=scores, diagnostics=diagnostics)


def _lm_step_inputs(who, q, s, lm_logits, input_ids, attention_mask, pair_words):  # noqa: ANN001
    """What the objectives through the reader LM share: every tensor on `q`'s GPU, shapes checked, in the layout the kernels read.

    `pair_words` is a list of `(name, tensor | None)` that must be float32 `[B, D]` words of the batch (`section__score`, ...).
    """
    if not q.is_cuda:
        raise _native.NativeLibraryError(f"{who} needs device tensors (there is no CPU path)")
    for name, x in (("section_encoding", s), *pair_words, ("lm_logits", lm_logits), ("lm__input_ids", input_ids),
                    ("lm__attention_mask", attention_mask)):
        if x is not None and x.device != q.device:  # the kernels get raw pointers: a host or other-device tensor must never reach them
            raise _native.NativeLibraryError(f"`{name}` is on {x.device}, `query_encoding` on {q.device}: all tensors must share one GPU")
    if lm_logits.dim() != 4:
        raise ValueError(f"`lm_logits` must be [B, D, L, V], got {tuple(lm_logits.shape)}")
    enc = q.dtype if q.dtype in _ENC else torch.float32
    ldt = lm_logits.dtype if lm_logits.dtype in _ENC else torch.float32
    qc, sc, lg = _as(q, enc), _as(s, enc), _as(lm_logits, ldt)
    if sc.dim() not in (2, 3):
        raise ValueError(f"Invalid dimension for `section_encoding`: {tuple(sc.shape)}")
    three_d = sc.dim() == 3
    B, H = qc.shape
    D = sc.shape[1] if three_d else sc.shape[0]
    _, _, L, V = lg.shape
    if L < 2:
        raise ValueError(f"`lm_logits` has L={L} positions: the shifted sequence needs L >= 2")
    if lg.shape[:2] != (B, D) or input_ids.shape != (B, D, L) or attention_mask.shape != (B, D, L):
        raise ValueError(f"lm_logits must be [{B}, {D}, L, V], lm__input_ids / lm__attention_mask [{B}, {D}, {L}]")
    words = []
    for name, x in pair_words:
        xc = None if x is None else _as(x, torch.float32)
        if xc is not None and xc.shape != (B, D):
            raise ValueError(f"{name} must be [{B}, {D}]")
        words.append(xc)
    ids = _as(input_ids, torch.int64)
    # the kernels test a mask element for any set bit: bool and integer masks are read as they are
    mask = attention_mask if not (attention_mask.is_floating_point() or attention_mask.is_complex()) else attention_mask != 0
    mask = mask.contiguous()
    return enc, ldt, qc, sc, lg, three_d, (B, D, H, L, V), words, ids, mask


def _lm_step_backward(ctx, g_loss, logits_arg):  # noqa: ANN001
    """`(dq, ds, d_logits)` from the forward's `d_scores` and `coef`; `lm_logits` was argument `logits_arg` of the forward."""
    lib = _native.load_library()
    qc, sc, lg, ids, mask, tok_lse, coef, d_scores = ctx.saved_tensors
    enc, ldt, three_d, B, D, H, L, V, q_dt, s_dt, lg_dt, mask_eb = ctx.meta
    dev = qc.device
    stream = _native.current_stream_ptr(dev)
    go = g_loss if (g_loss.dtype is torch.float32 and g_loss.is_contiguous()) else g_loss.float().contiguous()
    need_q, need_s, need_lg = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[logits_arg]
    dq = ds = d_lg = None
    with _on_device(dev):
        if need_q or need_s:
            dq = torch.empty((B, H), dtype=torch.float32, device=dev)
            ds = torch.empty(sc.shape, dtype=torch.float32, device=dev)
            _native.check(
                lib.vodhip_retrieval_backward(
                    qc.data_ptr(), sc.data_ptr(), _native.torch_dtype_code(enc), int(three_d), B, D, H,
                    d_scores.data_ptr(), go.data_ptr(), dq.data_ptr(), ds.data_ptr(), stream,
                )
            )
            dq = dq if q_dt is torch.float32 else dq.to(q_dt)
            ds = ds if s_dt is torch.float32 else ds.to(s_dt)
        if need_lg:
            d_lg = torch.empty_like(lg)  # the one logits-sized tensor of the step
            _native.check(
                lib.vodhip_lm_token_logprob_backward(
                    lg.data_ptr(), _native.torch_dtype_code(ldt), B * D, L, V, ids.data_ptr(), mask.data_ptr(), mask_eb,
                    tok_lse.data_ptr(), coef.data_ptr(), go.data_ptr(), d_lg.data_ptr(), stream,
                )
            )
            d_lg = d_lg if lg_dt is ldt else d_lg.to(lg_dt)
    return dq, ds, d_lg


class _MarginalLikelihood(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, s, score, lm_logits, input_ids, attention_mask):  # noqa: ANN001
        lib = _native.load_library()
        enc, ldt, qc, sc, lg, three_d, (B, D, H, L, V), (score_c,), ids, mask = _lm_step_inputs(
            "MarginalLikelihoodGradients", q, s, lm_logits, input_ids, attention_mask, [("section__score", score)])
        mask_eb = mask.element_size()
        dev = q.device
        stream = _native.current_stream_ptr(dev)
        N = B * D
        # per-token words: log-prob | (row max, log sum-exp); per-pair words: retriever scores | dLoss/dScores | coef
        tok = torch.empty((3, N, L - 1), dtype=torch.float32, device=dev)
        pairs = torch.empty((3, B, D), dtype=torch.float32, device=dev)
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        n_work = B + (4 * B * D if (not three_d and H >= 512) else 0)
        work = torch.empty((n_work,), dtype=torch.float32, device=dev)
        p_tok, p_pairs = tok.data_ptr(), pairs.data_ptr()
        with _on_device(dev):
            _native.check(
                lib.vodhip_lm_token_logprob_forward(
                    lg.data_ptr(), _native.torch_dtype_code(ldt), N, L, V, ids.data_ptr(), mask.data_ptr(), mask_eb,
                    p_tok, p_tok + 4 * N * (L - 1), stream,
                )
            )
            _native.check(
                lib.vodhip_marginal_forward(
                    qc.data_ptr(), sc.data_ptr(), _native.torch_dtype_code(enc), int(three_d), B, D, H, score_c.data_ptr(),
                    p_tok, mask.data_ptr(), mask_eb, L, p_pairs, p_pairs + 4 * N, p_pairs + 8 * N, loss.data_ptr(),
                    work.data_ptr(), n_work, stream,
                )
            )
        scores, d_scores, coef = pairs[0], pairs[1], pairs[2]
        tok_lse = tok[1:].view(N, L - 1, 2)  # (row max, log sum-exp) per token, the block behind tok_logp
        ctx.save_for_backward(qc, sc, lg, ids, mask, tok_lse, coef, d_scores)
        ctx.meta = (enc, ldt, three_d, B, D, H, L, V, q.dtype, s.dtype, lm_logits.dtype, mask_eb)
        ctx.mark_non_differentiable(scores)
        return loss[0], scores

    @staticmethod
    def backward(ctx, g_loss, _g_scores):  # noqa: ANN001
        dq, ds, d_lg = _lm_step_backward(ctx, g_loss, 3)
        return dq, ds, None, d_lg, None, None


class MarginalLikelihoodGradients:
    """Marginal likelihood of a retrieval-augmented LM (REALM) with the in-batch approximation, fused on the GPU.

    Mirror of the reference's `MarginalLikelihoodGradients` (src/vod_models/vod_gradients/marginal_likelihood.py:9-66): the same
    keyword-only call `(batch, query_encoding, section_encoding, lm_logits)`, reading `section__score`, `lm__input_ids` and
    `lm__attention_mask` from `batch`, the same outputs (`loss`, `retriever_scores`).  `lm_logits [B, D, L, V]` is read once forward
    (masked positions not at all) and read once / written once backward; between the two the step keeps three floats per token.
    `loss.backward()` fills the gradients of the two encodings and of `lm_logits`, each in its own dtype.  Where the reference
    raises on a target id outside [0, V-2] (a host synchronisation), a live one makes the loss NaN and a masked one is ignored.
    """

    def __call__(self, *, batch: typ.Any, query_encoding: torch.Tensor, section_encoding: torch.Tensor,
                 lm_logits: torch.Tensor) -> RealmOutput:
        get = (lambda k: batch.get(k)) if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
        score, ids, mask = get("section__score"), get("lm__input_ids"), get("lm__attention_mask")
        if score is None or ids is None or mask is None or lm_logits is None:
            raise ValueError("MarginalLikelihoodGradients needs section__score, lm__input_ids, lm__attention_mask and lm_logits")
        loss, scores = _MarginalLikelihood.apply(query_encoding, section_encoding, score, lm_logits, ids, mask)
        return RealmOutput(loss=loss, retriever_scores=scores)


class _Vod(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, s, score, log_weight, log_proposal, lm_logits, input_ids, attention_mask, cfg):  # noqa: ANN001
        lib = _native.load_library()
        alpha, temperature, reduction = cfg
        enc, ldt, qc, sc, lg, three_d, (B, D, H, L, V), (score_c, logw_c, logc_c), ids, mask = _lm_step_inputs(
            "VodGradients", q, s, lm_logits, input_ids, attention_mask,
            [("section__score", score), ("section__log_weight", log_weight), ("section__log_proposal", log_proposal)])
        mask_eb = mask.element_size()
        dev = q.device
        stream = _native.current_stream_ptr(dev)
        N = B * D
        # per-token words: log-prob | (row max, log sum-exp); per-pair words: retriever scores | dLoss/dScores | coef; loss [1] | diag [3]
        tok = torch.empty((3, N, L - 1), dtype=torch.float32, device=dev)
        pairs = torch.empty((3, B, D), dtype=torch.float32, device=dev)
        small = torch.empty((4,), dtype=torch.float32, device=dev)
        n_work = 4 * B + (4 * B * D if (not three_d and H >= 512) else 0)
        work = torch.empty((n_work,), dtype=torch.float32, device=dev)
        p_tok, p_pairs, p_small = tok.data_ptr(), pairs.data_ptr(), small.data_ptr()
        with _on_device(dev):
            _native.check(
                lib.vodhip_lm_token_logprob_forward(
                    lg.data_ptr(), _native.torch_dtype_code(ldt), N, L, V, ids.data_ptr(), mask.data_ptr(), mask_eb,
                    p_tok, p_tok + 4 * N * (L - 1), stream,
                )
            )
            _native.check(
                lib.vodhip_vod_forward(
                    qc.data_ptr(), sc.data_ptr(), _native.torch_dtype_code(enc), int(three_d), B, D, H, score_c.data_ptr(),
                    logw_c.data_ptr(), None if logc_c is None else logc_c.data_ptr(), p_tok, mask.data_ptr(), mask_eb, L,
                    alpha, temperature, reduction, p_pairs, p_pairs + 4 * N, p_pairs + 8 * N, p_small, p_small + 4,
                    work.data_ptr(), n_work, stream,
                )
            )
        scores, d_scores, coef = pairs[0], pairs[1], pairs[2]
        tok_lse = tok[1:].view(N, L - 1, 2)
        ctx.save_for_backward(qc, sc, lg, ids, mask, tok_lse, coef, d_scores)
        ctx.meta = (enc, ldt, three_d, B, D, H, L, V, q.dtype, s.dtype, lm_logits.dtype, mask_eb)
        diag = small[1:]
        ctx.mark_non_differentiable(scores, diag)
        return small[0], scores, diag

    @staticmethod
    def backward(ctx, g_loss, _g_scores, _g_diag):  # noqa: ANN001
        dq, ds, d_lg = _lm_step_backward(ctx, g_loss, 5)
        return dq, ds, None, None, None, d_lg, None, None, None


class VodGradients:
    """The Renyi VOD objective (Lievin et al., arXiv 2210.06345) over the priority-sampled sections of a batch, fused on the GPU.

    The reference's `VodGradients` (src/vod_models/vod_gradients/vod.py:14-26) raises `NotImplementedError`; this is the objective
    its collate was built for: the self-normalised importance-sampling estimate of the Renyi bound of order `alpha`, differentiated
    with respect to the model with the sampler held constant (include/vodhip.h H5v has the formulas).  `alpha = 0` is the
    importance-weighted bound, `alpha = 1` the ELBO; `alpha` is a plain attribute, so a schedule may set it between steps.
    The keyword-only call `(batch, query_encoding, section_encoding, lm_logits)` reads `section__score`, `section__log_weight`
    (what `vodhip_priority_sample` / the collate emit), `lm__input_ids`, `lm__attention_mask` and, when present,
    `section__log_proposal`: the sampler's log proposal up to a per-row constant.  Without it the proposal is taken to be
    `softmax(temperature * section__score)`, which is exact for a single-softmax sampler only.
    `token_reduction` is "mean" (the convention of the reference's `_compute_lm_logprobs`) or "sum" (the paper's log p(x | z)).
    Returns `loss`, `retriever_scores` and the detached diagnostics `iw_bound`, `elbo` and `ess` of the same launch.
    """

    def __init__(self, alpha: float = 0.0, temperature: float = 1.0, token_reduction: str = "mean"):
        if token_reduction not in ("mean", "sum"):
            raise ValueError(f"token_reduction must be 'mean' or 'sum', got {token_reduction!r}")
        self.alpha = alpha
        self.temperature = temperature
        self.token_reduction = token_reduction

    def __call__(self, *, batch: typ.Any, query_encoding: torch.Tensor, section_encoding: torch.Tensor,
                 lm_logits: torch.Tensor) -> RealmOutput:
        get = (lambda k: batch.get(k)) if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
        alpha, temperature = float(self.alpha), float(self.temperature)
        if not 0.0 <= alpha <= 1.0:  # (false for NaN)
            raise ValueError(f"alpha must be in [0, 1], got {self.alpha!r}")
        if not math.isfinite(temperature):
            raise ValueError(f"temperature must be finite, got {self.temperature!r}")
        score, ids, mask = get("section__score"), get("lm__input_ids"), get("lm__attention_mask")
        if score is None or ids is None or mask is None or lm_logits is None:
            raise ValueError("VodGradients needs section__score, lm__input_ids, lm__attention_mask and lm_logits")
        log_weight = get("section__log_weight")
        if log_weight is None:
            raise ValueError("VodGradients needs section__log_weight, the importance weights of the sampled sections "
                             "(`collate_on_device(...).to_dict('section__')` carries them)")
        loss, scores, diag = _Vod.apply(query_encoding, section_encoding, score, log_weight, get("section__log_proposal"), lm_logits,
                                        ids, mask, (alpha, temperature, 0 if self.token_reduction == "mean" else 1))
        return RealmOutput(loss=loss, retriever_scores=scores, diagnostics={"iw_bound": diag[0], "elbo": diag[1], "ess": diag[2]})


class GraphedRetrievalStep:
    """The fused loss, forward AND autograd backward, captured once as ONE hipGraph and replayed with one host call per step.

    Eager, a step of `RetrievalGradients` costs ~170-190 us of host time (two ctypes calls, four small allocations and ~80 us of torch
    autograd machinery around a custom Function) for ~90 us of kernels; a replay of the captured step is launch-free on the host:
    81 us (3-D, 64 x 32 x 768) / 118 us (in-batch, 64 x 2048 x 768) wall including the device synchronisation (tools/probe_h5_graph.py),
    bit-identical to an eager step that accumulates into zeroed `.grad` buffers, as the captured one does (0 + (-0.0) = +0.0: where a
    16-bit gradient underflows to -0.0, an eager backward into an empty `.grad` keeps the sign and the captured step returns +0.0).
    The captured step owns static buffers: `query_encoding`, `section_encoding`, the `section__*` fields
    of `batch` - write the step's inputs into them (`load(...)` copies, or produce them there), `replay()`, then read `output.loss`,
    `output.retriever_scores`, `output.diagnostics` and the gradients `dq` / `ds` (to continue into the encoders:
    `torch.autograd.backward([q_enc, s_enc], [step.dq, step.ds])`).  Shapes, dtypes and the set of optional fields are fixed at capture.
    With `monitor=` (a `vod_amd.monitoring.RetrievalMonitor`) every replay also updates the monitor from the step's relevances and
    `retriever_scores`: two more kernels in the same graph, no host work; read it with `monitor.get()` / `compute()` as usual.
    """

    def __init__(self, gradients: RetrievalGradients, *, batch_size: int, n_sections: int, hidden: int, sections_3d: bool = False,
                 dtype: torch.dtype = torch.float32, device: torch.device | int = 0, sparse: bool = True, dense: bool = True,
                 monitor: typ.Any = None):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        B, D, H = int(batch_size), int(n_sections), int(hidden)
        self.gradients = gradients
        self.monitor = monitor  # a vod_amd.monitoring.RetrievalMonitor: its update is captured behind the loss and replayed with it
        self.query_encoding = torch.zeros((B, H), dtype=dtype, device=dev, requires_grad=True)
        self.section_encoding = torch.zeros(((B, D, H) if sections_3d else (D, H)), dtype=dtype, device=dev, requires_grad=True)
        self.batch = {"section__score": torch.zeros((B, D), device=dev), "section__relevance": torch.zeros((B, D), dtype=torch.int64, device=dev),
                      "section__sparse": torch.zeros((B, D), device=dev) if sparse else None,
                      "section__dense": torch.zeros((B, D), device=dev) if dense else None}
        self.batch["section__relevance"][:, 0] = 1  # a well-formed batch for the warm-up steps
        self.query_encoding.grad = torch.zeros_like(self.query_encoding)
        self.section_encoding.grad = torch.zeros_like(self.section_encoding)
        # the warm-up steps run the monitor's update for real (its buffers must exist before the capture): its state is put back after them
        kept = None
        if monitor is not None:
            monitor.to(dev)
            kept = monitor.state.clone()
        # warm-up on a side stream (allocator pools, one-time driver calls such as the LDS attribute), then the capture
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                self._step()
        torch.cuda.current_stream(dev).wait_stream(side)
        if monitor is not None:
            monitor.state.copy_(kept)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.output = self._step()

    def _step(self) -> RealmOutput:
        self.query_encoding.grad.zero_()
        self.section_encoding.grad.zero_()
        out = self.gradients(batch=self.batch, query_encoding=self.query_encoding, section_encoding=self.section_encoding)
        out.loss.backward()
        if self.monitor is not None:
            self.monitor.update(self.batch, out)
        return out

    @property
    def dq(self) -> torch.Tensor:
        return self.query_encoding.grad

    @property
    def ds(self) -> torch.Tensor:
        return self.section_encoding.grad

    def load(self, *, batch: typ.Any, query_encoding: torch.Tensor, section_encoding: torch.Tensor) -> None:
        """Copy one step's inputs into the static buffers (device-to-device, no synchronisation)."""
        get = (lambda k: batch.get(k)) if isinstance(batch, dict) else (lambda k: getattr(batch, k, None))
        with torch.no_grad():
            self.query_encoding.copy_(query_encoding)
            self.section_encoding.copy_(section_encoding)
            for key, dst in self.batch.items():
                if dst is None:
                    if get(key) is not None:
                        raise ValueError(f"the step was captured without `{key}`: the set of optional fields is fixed at capture")
                    continue
                src = get(key)
                if src is None:
                    raise ValueError(f"the captured step expects `{key}`")
                dst.copy_(src)

    def replay(self) -> RealmOutput:
        self.graph.replay()
        return self.output

    def __call__(self, *, batch: typ.Any, query_encoding: torch.Tensor, section_encoding: torch.Tensor) -> tuple[RealmOutput, torch.Tensor, torch.Tensor]:
        self.load(batch=batch, query_encoding=query_encoding, section_encoding=section_encoding)
        return self.replay(), self.dq, self.ds
