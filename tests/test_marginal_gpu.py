"""`MarginalLikelihoodGradients` (vod_amd/csrc/kernels_marginal.hip) on the GPU against the float64 restatement (tests/marginal_ref.py).

Inputs come from tests/golden/marginal_likelihood.npz (what the reference computed for them is checked against the same restatement
in tests/test_marginal_cpu.py).  `e_ref` below is the fixture's `max |reference - restatement| / max |restatement|` per case and
output: the float32 reference's own error, the unit of the tolerance.

Tolerances
  * float32 runs, every output (loss, retriever_scores, dq, ds, dlogits): scaled error `max |got - f64| / max |f64|` at most
    GATE = max(4 * e_ref, 32 * 2^-24).  The factor 4 covers summation-order differences between two float32 pipelines; the floor of
    32 float32 ulps is what a V-term tree reduction plus exp / log can cost.  A wrong tail or a wrong shift shows at 1e-3 or more.
  * fp16 / bf16 runs (logits and encodings rounded first, restatement on the rounded values): loss and scores against the same GATE;
    every gradient is cast to its input's format, so elementwise `|g - g64| <= h * |g64| + GATE * max |g64|` (+ 2^-24 for fp16
    subnormals) with h = 2^-11 (fp16) or 2^-8 (bf16), half an ulp of the format.
Where the restatement is not finite (-inf scores of padded sections) the positions must match exactly.
Each test prints `MLERR <case> <dtype> <output> err=... gate=...` before it asserts (run with `-s`); profiles/marginal_likelihood.json
holds the lines of one run on an MI355X (float32: at most 0.65 of the gate).
"""
import functools
import json
import pathlib

import numpy as np
import pytest

import marginal_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "marginal_likelihood.npz"
CASES = ["tiny_3d", "tiny_2d", "mid_3d", "mid_2d", "wide_2d", "oddv_3d", "tailv_2d"]
OUTPUTS = ("loss", "retriever_scores", "dq", "ds", "dlogits")
FLOOR = 32 * 2.0 ** -24
HALF_ULP = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
TDT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _fixture():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["params_json"]))


def _round(a, dtype):
    """float32 array -> the values the GPU sees after a cast to `dtype` (as float32)."""
    return a if dtype == "float32" else torch.from_numpy(a).to(TDT[dtype]).float().numpy()


@functools.lru_cache(maxsize=None)
def _case(name, dtype="float32"):
    """(inputs as the GPU sees them, float64 restatement): computed once per (case, dtype), shared, never modified."""
    z, _ = _fixture()
    inp = {k: z[f"{name}__{k}"] for k in ("q", "s", "score", "logits", "ids", "mask")}
    inp["ids"] = inp["ids"].astype(np.int64)
    for k in ("q", "s", "logits"):
        inp[k] = _round(inp[k], dtype)
    want = marginal_ref.marginal(inp["q"], inp["s"], inp["score"], inp["logits"], inp["ids"], inp["mask"])
    return inp, want


def _run(inp, dtype="float32", mask_dtype=torch.int64, upstream=None):
    """Forward + backward -> (dict of float64 NumPy outputs, the raw tensors)."""
    from vod_amd.gradients import MarginalLikelihoodGradients

    dt = TDT[dtype]
    q = torch.tensor(inp["q"], device="cuda", dtype=dt).requires_grad_()
    s = torch.tensor(inp["s"], device="cuda", dtype=dt).requires_grad_()
    lg = torch.tensor(inp["logits"], device="cuda", dtype=dt).requires_grad_()
    batch = {"section__score": torch.tensor(inp["score"], device="cuda"), "lm__input_ids": torch.tensor(inp["ids"], device="cuda"),
             "lm__attention_mask": torch.tensor(inp["mask"] != 0, device="cuda").to(mask_dtype)}
    out = MarginalLikelihoodGradients()(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lg)
    (out.loss if upstream is None else out.loss * upstream).backward()
    assert out.loss.dtype == torch.float32 and out.loss.dim() == 0 and out.retriever_scores.dtype == torch.float32
    assert q.grad.dtype == dt and s.grad.dtype == dt and lg.grad.dtype == dt
    raw = {"loss": out.loss.detach(), "retriever_scores": out.retriever_scores, "dq": q.grad, "ds": s.grad, "dlogits": lg.grad}
    return {k: v.double().cpu().numpy() for k, v in raw.items()}, raw


def _same_bytes(a, b):
    """Bitwise equality: NaN-safe, and +0.0 is not -0.0."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _same_nonfinite(got, want, tag):
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), f"{tag}: non-finite positions differ"
    return fin


def _check(name, dtype, got, inp, want):
    _, params = _fixture()
    failures = []
    for key in OUTPUTS:
        g, w = got[key], np.asarray(want[key])
        assert g.shape == w.shape, key
        gate = max(4 * params["e_ref"][name][key], FLOOR)
        fin = _same_nonfinite(g, w, f"{name} {dtype} {key}")
        scale = float(np.abs(w[fin]).max()) if fin.any() else 0.0
        err = np.abs(np.where(fin, g, 0.0) - np.where(fin, w, 0.0))
        if dtype == "float32" or key in ("loss", "retriever_scores"):
            e = float(err.max()) / (scale if scale > 0 else 1.0)
            print(f"MLERR {name} {dtype} {key} err={e:.3e} gate={gate:.3e}")
            if not e <= gate:
                failures.append(f"{key}: scaled error {e:.3e} > {gate:.3e}")
        else:
            bound = HALF_ULP[dtype] * np.abs(np.where(fin, w, 0.0)) + gate * scale + (2.0 ** -24 if dtype == "float16" else 0.0)
            worst = float(np.max(err / np.where(bound > 0, bound, 1.0)))
            print(f"MLERR {name} {dtype} {key} err={float(err.max()):.3e} bound_used={worst:.4f} gate={gate:.3e}")
            if not np.all(err <= bound):
                failures.append(f"{key}: {int((err > bound).sum())} elements beyond the bound (worst {worst:.2f} x)")
    live = inp["mask"][..., 1:] != 0
    dl = got["dlogits"]
    assert np.all(dl[..., -1, :] == 0) and np.all(dl[..., :-1, :][~live] == 0), "masked / last positions must carry exactly 0"
    assert not failures, f"{name} {dtype}: " + "; ".join(failures)


@pytest.mark.parametrize("name", CASES)
def test_float32_cases_match_the_restatement(name):
    inp, want = _case(name)
    got, _ = _run(inp)
    _check(name, "float32", got, inp, want)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", CASES)
def test_16bit_cases_match_the_restatement_on_rounded_inputs(name, dtype):
    inp, want = _case(name, dtype)
    got, _ = _run(inp, dtype)
    _check(name, dtype, got, inp, want)


def test_upstream_gradient_and_mask_dtypes():
    """`loss * 2.5` scales every gradient; bool, uint8, int32 and int64 masks give bitwise the same step."""
    inp, want = _case("mid_3d")
    ref, raw_ref = _run(inp, upstream=2.5)
    for key in ("dq", "ds", "dlogits"):
        w = 2.5 * np.asarray(want[key])
        e = np.abs(ref[key] - w).max() / np.abs(w).max()
        print(f"MLERR mid_3d float32 {key}*2.5 err={e:.3e}")
        assert e <= max(4 * _fixture()[1]["e_ref"]["mid_3d"][key], FLOOR), key
    for mdt in (torch.bool, torch.uint8, torch.int32):
        _, raw = _run(inp, mask_dtype=mdt, upstream=2.5)
        assert all(torch.equal(raw[k], raw_ref[k]) for k in OUTPUTS), mdt


def test_real_vocabulary_bf16():
    """(1, 2, 3, 32128, 8) in bf16: 64 KiB rows, 4016 16-byte vectors - the unrolled sweep, its remainder and the cross-wave merge."""
    B, D, L, V, H = 1, 2, 3, 32128, 8
    rng = np.random.default_rng(6001)
    inp = {"q": _round((rng.integers(-64, 65, size=(B, H)) / 64.0).astype(np.float32), "bfloat16"),
           "s": _round((rng.integers(-64, 65, size=(B, D, H)) / 64.0).astype(np.float32), "bfloat16"),
           "score": np.zeros((B, D), dtype=np.float32),
           "logits": _round((rng.normal(size=(B, D, L, V)) * 3.0).astype(np.float32), "bfloat16"),
           "ids": rng.integers(0, V - 1, size=(B, D, L)).astype(np.int64), "mask": np.ones((B, D, L), dtype=np.int64)}
    inp["ids"][0, 0, 1], inp["ids"][0, 1, 2] = V - 2, 0   # the last legal target and the first
    inp["mask"][0, 1, 1] = 0
    want = marginal_ref.marginal(inp["q"], inp["s"], inp["score"], inp["logits"], inp["ids"], inp["mask"])
    got, _ = _run(inp, "bfloat16")
    gate = FLOOR  # no reference run at this size: the floor alone
    for key in ("loss", "retriever_scores"):
        e = marginal_ref.scaled_error(got[key], want[key])
        print(f"MLERR vocab32128 bfloat16 {key} err={e:.3e} gate={gate:.3e}")
        assert e <= gate, key
    for key in ("dq", "ds", "dlogits"):
        w = np.asarray(want[key])
        err = np.abs(got[key] - w)
        bound = HALF_ULP["bfloat16"] * np.abs(w) + gate * np.abs(w).max()
        print(f"MLERR vocab32128 bfloat16 {key} err={err.max():.3e} bound_used={np.max(err / bound):.4f}")
        assert np.all(err <= bound), key
    assert np.all(got["dlogits"][:, :, -1] == 0) and np.all(got["dlogits"][0, 1, 0] == 0)


def test_ids_at_masked_positions_are_ignored():
    inp, _ = _case("mid_3d")
    dead = np.argwhere(inp["mask"] == 0)
    assert len(dead) >= 2
    V = inp["logits"].shape[-1]
    a, b = dict(inp), dict(inp)
    a["ids"], b["ids"] = inp["ids"].copy(), inp["ids"].copy()
    for n, (i, j, k) in enumerate(dead):
        a["ids"][i, j, k] = -100 if n % 2 else V + 5
        b["ids"][i, j, k] = 0
    _, ra = _run(a)
    _, rb = _run(b)
    assert torch.isfinite(ra["loss"])
    for key in OUTPUTS:
        assert _same_bytes(ra[key], rb[key]), key


@pytest.mark.parametrize("bad", ["V-1", "-1", "V+5"])
def test_invalid_live_target_gives_nan_loss_and_finite_scores(bad):
    inp, _ = _case("mid_3d")
    V = inp["logits"].shape[-1]
    x = dict(inp)
    x["ids"] = inp["ids"].copy()
    assert inp["mask"][2, 4, 1] != 0 and np.isfinite(inp["score"][2, 4])
    x["ids"][2, 4, 1] = {"V-1": V - 1, "-1": -1, "V+5": V + 5}[bad]
    got, _ = _run(x)
    assert np.isnan(got["loss"])
    assert np.array_equal(np.isfinite(got["retriever_scores"]), np.isfinite(inp["score"]))


def test_sequence_without_live_tokens_gives_nan_loss():
    inp, _ = _case("mid_3d")
    x = dict(inp)
    x["mask"] = inp["mask"].copy()
    x["mask"][2, 4, 1:] = 0
    got, _ = _run(x)
    assert np.isnan(got["loss"])
    assert np.array_equal(np.isfinite(got["retriever_scores"]), np.isfinite(inp["score"]))


def test_errors():
    from vod_amd import _native
    from vod_amd.gradients import MarginalLikelihoodGradients

    inp, _ = _case("tiny_3d")
    t = {k: torch.tensor(v) for k, v in inp.items()}
    cpu_batch = {"section__score": t["score"], "lm__input_ids": t["ids"], "lm__attention_mask": t["mask"]}
    with pytest.raises(_native.NativeLibraryError):
        MarginalLikelihoodGradients()(batch=cpu_batch, query_encoding=t["q"], section_encoding=t["s"], lm_logits=t["logits"])
    dev_batch = {k: v.cuda() for k, v in cpu_batch.items()}
    for key in cpu_batch:  # one host tensor next to device tensors: refused before any pointer reaches a kernel
        mixed = dict(dev_batch)
        mixed[key] = cpu_batch[key]
        with pytest.raises(_native.NativeLibraryError):
            MarginalLikelihoodGradients()(batch=mixed, query_encoding=t["q"].cuda(), section_encoding=t["s"].cuda(),
                                          lm_logits=t["logits"].cuda())
    with pytest.raises(_native.NativeLibraryError):
        MarginalLikelihoodGradients()(batch=dev_batch, query_encoding=t["q"].cuda(), section_encoding=t["s"].cuda(), lm_logits=t["logits"])
    batch = {k: v[..., :1].cuda() if k.startswith("lm__") else v.cuda() for k, v in cpu_batch.items()}
    with pytest.raises(ValueError):
        MarginalLikelihoodGradients()(batch=batch, query_encoding=t["q"].cuda(), section_encoding=t["s"].cuda(),
                                      lm_logits=t["logits"][:, :, :1].cuda())


def test_two_eager_runs_are_bitwise_equal():
    for name, dtype in (("mid_2d", "float32"), ("wide_2d", "float32"), ("tailv_2d", "bfloat16")):
        inp, _ = _case(name, dtype)
        _, a = _run(inp, dtype)
        _, b = _run(inp, dtype)
        for key in OUTPUTS:  # (bytes, not values: NaN-safe and sign-of-zero-exact)
            assert _same_bytes(a[key], b[key]), (name, key)


def test_captured_step_replays_the_eager_result():
    from vod_amd.gradients import MarginalLikelihoodGradients

    inp, _ = _case("mid_3d")
    q = torch.tensor(inp["q"], device="cuda").requires_grad_()
    s = torch.tensor(inp["s"], device="cuda").requires_grad_()
    lg = torch.tensor(inp["logits"], device="cuda").requires_grad_()
    batch = {"section__score": torch.tensor(inp["score"], device="cuda"), "lm__input_ids": torch.tensor(inp["ids"], device="cuda"),
             "lm__attention_mask": torch.tensor(inp["mask"], device="cuda")}
    for t in (q, s, lg):
        t.grad = torch.zeros_like(t)

    def step():
        for t in (q, s, lg):
            t.grad.zero_()
        out = MarginalLikelihoodGradients()(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lg)
        out.loss.backward()
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            e_out = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # the eager result of the SAME step (it accumulates into zeroed gradients, as the captured one does), copied out
    eager = {"loss": e_out.loss.detach().clone(), "retriever_scores": e_out.retriever_scores.clone(), "dq": q.grad.clone(),
             "ds": s.grad.clone(), "dlogits": lg.grad.clone()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for t in (q, s, lg):  # the replay must recompute everything
        t.grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    got = {"loss": out.loss.detach(), "retriever_scores": out.retriever_scores, "dq": q.grad, "ds": s.grad, "dlogits": lg.grad}
    for key in OUTPUTS:
        assert _same_bytes(got[key], eager[key]), key


def test_step_adds_one_logits_sized_tensor_to_the_peak():
    """Forward + backward of (2, 2, 3, 4104, 8): the allocator's peak grows by the logits gradient plus O(B * D * L) floats.

    Slack: every small tensor of the step (token words, pair words, loss, workspace, the upstream gradient, dq, ds and their casts)
    is below 512 bytes here and occupies one 512-byte allocator block: 32 blocks = 16 KiB, plus 16 floats per token.
    """
    from vod_amd.gradients import MarginalLikelihoodGradients

    inp, _ = _case("tailv_2d")
    B, D, L, V = inp["logits"].shape
    q = torch.tensor(inp["q"], device="cuda").requires_grad_()
    s = torch.tensor(inp["s"], device="cuda").requires_grad_()
    lg = torch.tensor(inp["logits"], device="cuda").requires_grad_()
    batch = {"section__score": torch.tensor(inp["score"], device="cuda"), "lm__input_ids": torch.tensor(inp["ids"], device="cuda"),
             "lm__attention_mask": torch.tensor(inp["mask"], device="cuda")}
    MarginalLikelihoodGradients()(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lg).loss.backward()  # warm-up
    q.grad = s.grad = lg.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    MarginalLikelihoodGradients()(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lg).loss.backward()
    torch.cuda.synchronize()
    added = torch.cuda.max_memory_allocated() - before
    logits_bytes = lg.numel() * lg.element_size()
    slack = 32 * 512 + 16 * 4 * B * D * L
    print(f"MLMEM added={added} logits_bytes={logits_bytes} slack={slack}")
    assert logits_bytes <= added <= logits_bytes + slack
