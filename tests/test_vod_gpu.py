"""`VodGradients` (vod_row_kernel in vod_amd/csrc/kernels_marginal.hip) on the GPU against the float64 restatement (tests/vod_ref.py).

No reference implementation exists, so there is no reference run to take the unit of the tolerance from.  It is `e32` instead: the
scaled error `max |f32 - f64| / max |f64|` of the SAME restatement evaluated in float32 by torch on the CPU, computed here for every
(case, alpha, reduction, output).

Tolerances (the scheme of tests/test_marginal_gpu.py)
  * float32 runs, every output (loss, retriever_scores, dq, ds, dlogits, iw_bound, elbo, ess): scaled error at most
    GATE = max(4 * e32, 32 * 2^-24).  The factor 4 covers summation-order differences between two float32 pipelines; the floor is
    the 32 float32 ulps of a tree reduction plus exp / log.
  * fp16 / bf16 runs (logits and encodings rounded first, both restatements on the rounded values): loss, scores and diagnostics
    against the same GATE; every gradient is cast to its input's format, so elementwise `|g - g64| <= h * |g64| + GATE * max |g64|`
    (+ 2^-24 for fp16 subnormals) with h = 2^-11 (fp16) or 2^-8 (bf16), half an ulp of the format.
Non-finite positions must match exactly.  Each test prints `VODERR <case> <dtype> <alpha> <output> err=... gate=...` before it asserts
(run with `-s`); profiles/vod_gradients.json is where the lines of a run on an MI355X are kept (profiles/README.md).

Every case carries a padded section, a section of finite score whose log-weight is -inf, and 25 % masked tokens - except `one`
(D = 1), where either would empty the row: it keeps the token mask, and `test_rows_without_a_live_section` covers its padded and
excluded rows.
"""
import functools

import numpy as np
import pytest

import marginal_ref

torch = pytest.importorskip("torch")
import vod_ref  # noqa: E402

pytestmark = pytest.mark.gpu

#        name: (B, D, H, L, V, 3-D sections)
CASES = {"3d": (3, 5, 8, 4, 11, True),          # 3-D sections
         "2d": (3, 5, 8, 4, 11, False),         # 2-D sections
         "one": (2, 1, 8, 4, 11, True),         # one section
         "wave": (2, 65, 8, 4, 11, False),      # D past one wavefront
         "stride": (2, 257, 8, 4, 11, True),    # D past the workgroup stride of 256
         "splitk": (2, 9, 768, 4, 11, False),   # 2-D, the H >= 512 split-K slab path
         "longl": (2, 4, 8, 70, 515, True)}     # L - 1 > 64, odd V: the unaligned row path
ALPHAS = (0.0, 0.5, 1 - 1e-4, 1.0)
OUTPUTS = ("loss", "retriever_scores", "dq", "ds", "dlogits", "iw_bound", "elbo", "ess")
GRADS = ("dq", "ds", "dlogits")
FLOOR = 32 * 2.0 ** -24
HALF_ULP = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
TDT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _round(a, dtype):
    """float32 array -> the values the GPU sees after a cast to `dtype` (as float32)."""
    return a if dtype == "float32" else torch.from_numpy(a).to(TDT[dtype]).float().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(name, dtype="float32", excluded=True):
    """Seeded float32 inputs of a case, as the GPU sees them: computed once, shared, never modified."""
    B, D, H, L, V, three_d = CASES[name]
    rng = np.random.default_rng(9000 + sorted(CASES).index(name))
    f = np.float32
    inp = {"q": (rng.normal(size=(B, H)) * 2 * H ** -0.5).astype(f), "s": rng.normal(size=(B, D, H) if three_d else (D, H)).astype(f),
           "score": (rng.normal(size=(B, D)) * 2).astype(f), "logw": (rng.normal(size=(B, D)) * 1.5).astype(f),
           "logits": (rng.normal(size=(B, D, L, V)) * 2).astype(f), "ids": rng.integers(0, V - 1, size=(B, D, L)).astype(np.int64)}
    mask = np.ones((B, D, L - 1), dtype=np.int64)
    flat = mask.reshape(B * D, L - 1)
    n_dead = max(1, round(0.25 * (L - 1)))  # 25 % of the shifted positions of every sequence, holes included
    for row in flat:
        row[rng.choice(L - 1, size=n_dead, replace=False)] = 0
    inp["mask"] = np.concatenate([np.ones((B, D, 1), dtype=np.int64), mask], axis=-1)
    if D > 1:
        inp["score"][0, D - 1] = inp["logw"][0, D - 1] = -np.inf   # a padded section (the sampler leaves -inf weights there)
        inp["score"][B - 1, 0] = inp["logw"][B - 1, 0] = -np.inf
        if excluded:
            inp["logw"][0, 0] = inp["logw"][1, D // 2] = -np.inf   # a finite score that was not sampled
    for k in ("q", "s", "logits"):
        inp[k] = _round(inp[k], dtype)
    for v in inp.values():
        v.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def _want(name, dtype, alpha, reduction, excluded=True, marginal_weights=False):
    """(inputs, float64 restatement, e32 per output) of one configuration."""
    inp = _inputs(name, dtype, excluded)
    kw = {"alpha": alpha, "token_reduction": reduction}
    if marginal_weights:
        inp = dict(inp)
        inp["logw"] = vod_ref.log_softmax_live(np.float32(0.7) * np.where(np.isinf(inp["score"]), 0, inp["score"]), inp["score"])
        kw["temperature"] = 0.7
    args = (inp["q"], inp["s"], inp["score"], inp["logw"], inp["logits"], inp["ids"], inp["mask"])
    w64 = vod_ref.vod(*args, **kw)
    w32 = vod_ref.vod(*args, dtype=torch.float32, **kw)
    return inp, w64, _e32(w32, w64)


def _e32(w32, w64):
    return {k: marginal_ref.scaled_error(w32[k], w64[k]) for k in OUTPUTS + ("d_scores", "coef")}


def _run(inp, dtype="float32", *, mask_dtype=torch.int64, upstream=None, gradients=None, log_proposal=None, **kw):
    """Forward + backward -> (dict of float64 NumPy outputs, the raw tensors)."""
    from vod_amd.gradients import VodGradients

    dt = TDT[dtype]
    q = torch.tensor(inp["q"], device="cuda", dtype=dt).requires_grad_()
    s = torch.tensor(inp["s"], device="cuda", dtype=dt).requires_grad_()
    lg = torch.tensor(inp["logits"], device="cuda", dtype=dt).requires_grad_()
    batch = {"section__score": torch.tensor(inp["score"], device="cuda"), "section__log_weight": torch.tensor(inp["logw"], device="cuda"),
             "lm__input_ids": torch.tensor(inp["ids"], device="cuda"),
             "lm__attention_mask": torch.tensor(inp["mask"] != 0, device="cuda").to(mask_dtype)}
    if log_proposal is not None:
        batch["section__log_proposal"] = torch.tensor(log_proposal, device="cuda")
    out = (gradients or VodGradients(**kw))(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lg)
    (out.loss if upstream is None else out.loss * upstream).backward()
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0 and out.retriever_scores.dtype == torch.float32
    assert q.grad.dtype == dt and s.grad.dtype == dt and lg.grad.dtype == dt
    assert list(out.diagnostics) == ["iw_bound", "elbo", "ess"]
    assert all(v.dtype == torch.float32 and v.dim() == 0 and not v.requires_grad for v in out.diagnostics.values())
    raw = {"loss": out.loss.detach(), "retriever_scores": out.retriever_scores, "dq": q.grad, "ds": s.grad, "dlogits": lg.grad,
           **out.diagnostics}
    return {k: v.double().cpu().numpy() for k, v in raw.items()}, raw


def _same_bytes(a, b):
    """Bitwise equality: NaN-safe, and +0.0 is not -0.0."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _exact_zeros(got, inp):
    """Sections outside the live set, masked positions and t = L-1 carry exactly 0."""
    dead = np.isinf(inp["score"]) | np.isinf(inp["logw"])
    live = inp["mask"][..., 1:] != 0
    dl = got["dlogits"]
    assert np.all(dl[..., -1, :] == 0) and np.all(dl[..., :-1, :][~live] == 0), "masked / last positions must carry exactly 0"
    assert np.all(dl[dead] == 0), "sections outside the live set must carry exactly 0"
    if inp["s"].ndim == 3:
        assert np.all(got["ds"][dead] == 0)


def _check(tag, dtype, got, inp, want, e32, outputs=OUTPUTS):
    failures = []
    for key in outputs:
        g, w = got[key], np.asarray(want[key])
        assert g.shape == w.shape, key
        gate = max(4 * e32[key], FLOOR)
        fin = np.isfinite(w)
        assert np.array_equal(g[~fin], w[~fin], equal_nan=True), f"{tag} {key}: non-finite positions differ"
        scale = float(np.abs(w[fin]).max()) if fin.any() else 0.0
        err = np.abs(np.where(fin, g, 0.0) - np.where(fin, w, 0.0))
        if dtype == "float32" or key not in GRADS:
            e = float(err.max()) / (scale if scale > 0 else 1.0)
            print(f"VODERR {tag} {key} err={e:.3e} gate={gate:.3e}")
            if not e <= gate:
                failures.append(f"{key}: scaled error {e:.3e} > {gate:.3e}")
        else:
            bound = HALF_ULP[dtype] * np.abs(np.where(fin, w, 0.0)) + gate * scale + (2.0 ** -24 if dtype == "float16" else 0.0)
            worst = float(np.max(err / np.where(bound > 0, bound, 1.0)))
            print(f"VODERR {tag} {key} err={float(err.max()):.3e} bound_used={worst:.4f} gate={gate:.3e}")
            if not np.all(err <= bound):
                failures.append(f"{key}: {int((err > bound).sum())} elements beyond the bound (worst {worst:.2f} x)")
    _exact_zeros(got, inp)
    assert not failures, f"{tag}: " + "; ".join(failures)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", list(CASES))
def test_float32_cases_match_the_restatement(name, alpha, reduction):
    inp, want, e32 = _want(name, "float32", alpha, reduction)
    got, _ = _run(inp, alpha=alpha, token_reduction=reduction)
    _check(f"{name} float32 {alpha:g} {reduction}", "float32", got, inp, want, e32)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", ["3d", "splitk"])
def test_16bit_cases_match_the_restatement_on_rounded_inputs(name, dtype, alpha, reduction):
    inp, want, e32 = _want(name, dtype, alpha, reduction)
    got, _ = _run(inp, dtype, alpha=alpha, token_reduction=reduction)
    _check(f"{name} {dtype} {alpha:g} {reduction}", dtype, got, inp, want, e32)


@pytest.mark.parametrize("name", ["3d", "2d", "splitk"])
def test_exact_weights_give_the_marginal_likelihood_on_the_device(name):
    """alpha = 0, mean reduction, log_weight = log_softmax(0.7 * score) over the live set, temperature 0.7: the estimator is the exact
    marginal likelihood, so every output sits within GATE of `MarginalLikelihoodGradients` on the same tensors."""
    from vod_amd.gradients import MarginalLikelihoodGradients

    inp, want, e32 = _want(name, "float32", 0.0, "mean", excluded=False, marginal_weights=True)
    got, _ = _run(inp, alpha=0.0, temperature=0.7)
    _check(f"{name}-marginal float32 0 mean", "float32", got, inp, want, e32)
    q = torch.tensor(inp["q"], device="cuda").requires_grad_()
    s = torch.tensor(inp["s"], device="cuda").requires_grad_()
    lg = torch.tensor(inp["logits"], device="cuda").requires_grad_()
    batch = {"section__score": torch.tensor(inp["score"], device="cuda"), "lm__input_ids": torch.tensor(inp["ids"], device="cuda"),
             "lm__attention_mask": torch.tensor(inp["mask"], device="cuda")}
    out = MarginalLikelihoodGradients()(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lg)
    out.loss.backward()
    ml = {"loss": out.loss.detach(), "retriever_scores": out.retriever_scores, "dq": q.grad, "ds": s.grad, "dlogits": lg.grad}
    for key, v in ml.items():
        e = marginal_ref.scaled_error(got[key], v.double().cpu().numpy())
        gate = max(4 * e32[key], FLOOR)
        print(f"VODERR {name}-vs-marginal float32 0 mean {key} err={e:.3e} gate={gate:.3e}")
        assert e <= gate, key
    assert abs(got["iw_bound"] + got["loss"]) <= FLOOR * abs(got["loss"])


def test_rows_without_a_live_section():
    """D = 1 with a live, a padded and an excluded row: a NaN loss, the score pattern of the padding alone, and no gradient from the
    two rows that take no part."""
    rng = np.random.default_rng(9100)
    B, D, H, L, V = 3, 1, 8, 4, 11
    f = np.float32
    inp = {"q": rng.normal(size=(B, H)).astype(f), "s": rng.normal(size=(B, D, H)).astype(f), "score": np.zeros((B, D), dtype=f),
           "logw": np.zeros((B, D), dtype=f), "logits": rng.normal(size=(B, D, L, V)).astype(f),
           "ids": rng.integers(0, V - 1, size=(B, D, L)), "mask": np.ones((B, D, L), dtype=np.int64)}
    inp["score"][1, 0] = inp["logw"][1, 0] = inp["logw"][2, 0] = -np.inf
    got, _ = _run(inp, alpha=0.5)
    want = vod_ref.vod(inp["q"], inp["s"], inp["score"], inp["logw"], inp["logits"], inp["ids"], inp["mask"], alpha=0.5)
    assert np.isnan(got["loss"]) and np.isnan(want["loss"]) and all(np.isnan(got[k]) for k in ("iw_bound", "elbo", "ess"))
    assert np.array_equal(np.isinf(got["retriever_scores"]), np.isinf(inp["score"]))
    assert np.all(got["dq"][1:] == 0) and np.all(got["ds"][1:] == 0) and np.all(got["dlogits"][1:] == 0)
    # the live row: one section, omega = pi = 1 exactly, so no gradient reaches the encodings; the logits get -(1 / B n) (1[tgt] - softmax)
    assert np.all(got["dq"][0] == 0) and np.all(got["ds"][0] == 0) and np.all(want["dq"][0] == 0) and np.all(want["ds"][0] == 0)
    w = want["dlogits"][0]
    assert np.abs(w).max() > 1e-3 and np.abs(got["dlogits"][0] - w).max() <= FLOOR * np.abs(w).max()


RULES = ["nan_weight", "nan_proposal", "no_tokens_mean", "no_tokens_sum", "bad_id", "ninf_target"]


@pytest.mark.parametrize("rule", RULES)
def test_corner_rules_on_the_device(rule):
    """One rule of include/vodhip.h H5v at a time, at the live section (1, 1) of the `3d` case, alpha = 0.5: every output against the
    restatement on the same inputs, non-finite positions included.  A NaN goes through the formulas as written: the loss, the
    diagnostics and the gradients of every live section of row 1 are NaN, the other rows' gradients are what they were."""
    base = _inputs("3d")
    inp = {k: v.copy() for k, v in base.items()}
    assert np.isfinite(inp["score"][1, 1]) and np.isfinite(inp["logw"][1, 1])
    t_live = int(np.flatnonzero(inp["mask"][1, 1, 1:])[0])  # a live shifted position of that section
    kw = {"alpha": 0.5, "token_reduction": "sum" if rule == "no_tokens_sum" else "mean"}
    if rule == "nan_weight":
        inp["logw"][1, 1] = np.nan
    elif rule == "nan_proposal":
        kw["log_proposal"] = np.where(np.isinf(inp["score"]), 0, inp["score"]).astype(np.float32)
        kw["log_proposal"][1, 1] = np.nan
    elif rule.startswith("no_tokens"):
        inp["mask"][1, 1, 1:] = 0
    elif rule == "bad_id":
        inp["ids"][1, 1, t_live + 1] = inp["logits"].shape[-1] - 1
    else:
        inp["logits"][1, 1, t_live, inp["ids"][1, 1, t_live + 1]] = -np.inf
    args = (inp["q"], inp["s"], inp["score"], inp["logw"], inp["logits"], inp["ids"], inp["mask"])
    want = vod_ref.vod(*args, **kw)
    e32 = _e32(vod_ref.vod(*args, dtype=torch.float32, **kw), want)
    if rule == "bad_id":
        # coef of the section is NaN, so the kernel writes NaN at each of its live positions; the restatement's `where` that makes
        # the token NaN stops the gradient at the invalid position itself
        assert np.all(want["dlogits"][1, 1, t_live] == 0)
        want["dlogits"][1, 1, t_live] = np.nan
    got, _ = _run(inp, **kw)
    if rule == "ninf_target":  # legal: omega = 0 there, every gradient finite, the ELBO alone is -inf
        assert np.isfinite(got["loss"]) and got["elbo"] == -np.inf and all(np.isfinite(got[k]).all() for k in GRADS)
        assert np.all(got["dlogits"][1, 1] == 0)
    else:
        assert np.isnan(got["loss"]) and all(np.isnan(got[k]) for k in ("iw_bound", "elbo", "ess"))
        assert np.isfinite(got["dq"][[0, 2]]).all() and np.isnan(got["dq"][1]).all()
        assert np.array_equal(np.isfinite(got["retriever_scores"]), np.isfinite(inp["score"]))
    _check(f"3d-{rule} float32 0.5 {kw['token_reduction']}", "float32", got, inp, want, e32)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("name", ["3d", "2d", "wave", "splitk"])
def test_d_scores_and_coef_of_the_entry_point(name, reduction):
    """`vodhip_vod_forward` called directly: d_scores and coef against their closed forms, and exactly 0 at every section outside the
    live set (through `ds` the 2-D cases would only show a sum over the rows)."""
    from vod_amd import _native

    inp, want, e32 = _want(name, "float32", 0.5, reduction)
    lib = _native.load_library()
    B, D, L, V = inp["logits"].shape
    H, three_d = inp["q"].shape[1], inp["s"].ndim == 3
    dev = {k: torch.tensor(v, device="cuda") for k, v in inp.items()}
    tok = torch.empty((3, B * D, L - 1), device="cuda")
    pairs = torch.full((3, B, D), 7.0, device="cuda")
    small = torch.empty((4,), device="cuda")
    n_work = 4 * B + 4 * B * D
    work = torch.empty((n_work,), device="cuda")
    stream = _native.current_stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    p_tok, p = tok.data_ptr(), pairs.data_ptr()
    _native.check(lib.vodhip_lm_token_logprob_forward(dev["logits"].data_ptr(), _native.F32, B * D, L, V, dev["ids"].data_ptr(),
                                                      dev["mask"].data_ptr(), 8, p_tok, p_tok + 4 * B * D * (L - 1), stream))
    _native.check(lib.vodhip_vod_forward(dev["q"].data_ptr(), dev["s"].data_ptr(), _native.F32, int(three_d), B, D, H,
                                         dev["score"].data_ptr(), dev["logw"].data_ptr(), None, p_tok, dev["mask"].data_ptr(), 8, L,
                                         0.5, 1.0, 0 if reduction == "mean" else 1, p, p + 4 * B * D, p + 8 * B * D,
                                         small.data_ptr(), small.data_ptr() + 4, work.data_ptr(), n_work, stream))
    got = {"d_scores": pairs[1].double().cpu().numpy(), "coef": pairs[2].double().cpu().numpy()}
    dead = np.isinf(inp["score"]) | np.isinf(inp["logw"])
    assert dead.any()
    for key in ("d_scores", "coef"):
        assert np.all(got[key][dead] == 0), key
        assert np.all(got[key][~dead] != 0), key
        e, gate = marginal_ref.scaled_error(got[key], want[key]), max(4 * e32[key], FLOOR)
        print(f"VODERR {name} float32 0.5 {reduction} {key} err={e:.3e} gate={gate:.3e}")
        assert e <= gate, key
    assert abs(float(small[0]) - want["loss"]) <= max(4 * e32["loss"], FLOOR) * abs(want["loss"])


def test_log_proposal_overrides_temperature_times_score():
    inp, _, _ = _want("3d", "float32", 0.5, "mean")
    _, base = _run(inp, alpha=0.5, temperature=0.7)
    same = (np.float32(0.7) * np.where(np.isinf(inp["score"]), 0, inp["score"])).astype(np.float32)
    _, a = _run(inp, alpha=0.5, temperature=0.7, log_proposal=same)
    for key in OUTPUTS:
        assert _same_bytes(a[key], base[key]), key
    other = same.copy()
    other[1, 1] += 0.5
    other[2, 2] = -np.inf  # a proposal of -inf excludes the section as a weight of -inf does
    got, b = _run(inp, alpha=0.5, temperature=0.7, log_proposal=other)
    assert not torch.equal(b["loss"], base["loss"])
    args = (inp["q"], inp["s"], inp["score"], inp["logw"], inp["logits"], inp["ids"], inp["mask"])
    kw = {"alpha": 0.5, "temperature": 0.7, "log_proposal": other}
    want = vod_ref.vod(*args, **kw)
    e32 = _e32(vod_ref.vod(*args, dtype=torch.float32, **kw), want)
    for key in OUTPUTS:
        e, gate = marginal_ref.scaled_error(got[key], want[key]), max(4 * e32[key], FLOOR)
        print(f"VODERR 3d-proposal float32 0.5 mean {key} err={e:.3e} gate={gate:.3e}")
        assert e <= gate, key
    assert np.all(got["ds"][2, 2] == 0) and np.all(got["dlogits"][2, 2] == 0)


def test_upstream_gradient_and_mask_dtypes():
    """`loss * 2.5` scales every gradient; bool, uint8, int32 and int64 masks give bitwise the same step."""
    inp, want, e32 = _want("2d", "float32", 0.5, "sum")
    ref, raw_ref = _run(inp, alpha=0.5, token_reduction="sum", upstream=2.5)
    for key in GRADS:
        w = 2.5 * np.asarray(want[key])
        e = np.abs(ref[key] - w).max() / np.abs(w).max()
        print(f"VODERR 2d float32 0.5 sum {key}*2.5 err={e:.3e}")
        assert e <= max(4 * e32[key], FLOOR), key
    for mdt in (torch.bool, torch.uint8, torch.int32):
        _, raw = _run(inp, alpha=0.5, token_reduction="sum", mask_dtype=mdt, upstream=2.5)
        assert all(torch.equal(raw[k], raw_ref[k]) for k in OUTPUTS), mdt


def test_two_eager_runs_are_bitwise_equal():
    for name, dtype in (("stride", "float32"), ("splitk", "float32"), ("longl", "bfloat16")):
        inp = _inputs(name, dtype)
        _, a = _run(inp, dtype, alpha=0.5)
        _, b = _run(inp, dtype, alpha=0.5)
        for key in OUTPUTS:  # (bytes, not values: NaN-safe and sign-of-zero-exact)
            assert _same_bytes(a[key], b[key]), (name, key)


def test_alpha_is_an_attribute_a_schedule_may_set():
    from vod_amd.gradients import VodGradients

    inp = _inputs("3d")
    one = VodGradients(alpha=0.0)
    _, first = _run(inp, gradients=one)
    one.alpha = 0.75
    _, second = _run(inp, gradients=one)
    _, a = _run(inp, alpha=0.0)
    _, b = _run(inp, alpha=0.75)
    for key in OUTPUTS:
        assert _same_bytes(first[key], a[key]) and _same_bytes(second[key], b[key]), key
    assert not torch.equal(a["loss"], b["loss"])


def test_errors():
    from vod_amd import _native
    from vod_amd.gradients import VodGradients

    inp = _inputs("3d")
    t = {k: torch.tensor(v) for k, v in inp.items()}
    d = {k: v.cuda() for k, v in t.items()}

    def batch(src, **over):
        b = {"section__score": src["score"], "section__log_weight": src["logw"], "lm__input_ids": src["ids"],
             "lm__attention_mask": src["mask"]}
        b.update(over)
        return {k: v for k, v in b.items() if v is not None}

    def call(b, g=None, q=d["q"], s=d["s"], lg=d["logits"]):
        return (g or VodGradients())(batch=b, query_encoding=q, section_encoding=s, lm_logits=lg)

    assert torch.isfinite(call(batch(d)).loss)
    with pytest.raises(ValueError, match="section__log_weight"):
        call(batch(d, section__log_weight=None))
    for alpha in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="alpha"):
            call(batch(d), VodGradients(alpha=alpha))
    for temperature in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            call(batch(d), VodGradients(temperature=temperature))
    with pytest.raises(ValueError):
        VodGradients(token_reduction="max")
    for key in ("section__log_weight", "section__log_proposal", "section__score"):
        with pytest.raises(ValueError, match=key):
            call(batch(d, **{key: d["logw"][:, :-1]}))
        with pytest.raises(ValueError, match=key):
            call(batch(d, **{key: d["logw"].t().contiguous()}))
    with pytest.raises(_native.NativeLibraryError):  # all on the host
        call(batch(t), q=t["q"], s=t["s"], lg=t["logits"])
    for key in ("section__score", "section__log_weight", "section__log_proposal", "lm__input_ids", "lm__attention_mask"):
        host = t["logw"] if key == "section__log_proposal" else batch(t)[key]
        with pytest.raises(_native.NativeLibraryError, match="must share one GPU"):  # one host tensor next to device tensors
            call(batch(d, **{key: host}))
    with pytest.raises(_native.NativeLibraryError):
        call(batch(d), lg=t["logits"])
    # beyond the LDS budget: the C-ABI refuses with a status and a message, before any launch (the pointers are never read)
    lib = _native.load_library()
    p = d["logw"].data_ptr()
    for D, H, word in ((8193, 8, "8192"), (8192, 8192, "160 KiB")):
        status = lib.vodhip_vod_forward(p, p, _native.F32, 1, 1, D, H, p, p, None, p, p, 8, 4, 0.0, 1.0, 0, p, p, p, p, p, p, 4, None)
        assert status != 0 and word in lib.vodhip_last_error().decode()
    for alpha, temperature, red, word in ((1.5, 1.0, 0, "alpha"), (float("nan"), 1.0, 0, "alpha"), (0.0, float("inf"), 0, "temperature"),
                                          (0.0, 1.0, 2, "token_reduction")):
        status = lib.vodhip_vod_forward(p, p, _native.F32, 1, 1, 4, 8, p, p, None, p, p, 8, 4, alpha, temperature, red, p, p, p, p, p, p, 4,
                                        None)
        assert status != 0 and word in lib.vodhip_last_error().decode()
    status = lib.vodhip_vod_forward(p, p, _native.F32, 1, 2, 4, 8, p, p, None, p, p, 8, 4, 0.0, 1.0, 0, p, p, p, p, p, p, 7, None)
    assert status != 0 and "workspace_floats" in lib.vodhip_last_error().decode()
