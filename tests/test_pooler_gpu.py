"""`VodPooler` (vod_amd/csrc/kernels_pool.hip) on the GPU against the float64 restatement (tests/pooler_ref.py).

Inputs come from tests/golden/pooler.npz (what the reference computed for them is checked against the same restatement in
tests/test_pooler_cpu.py).  `e_ref` is the fixture's `max |reference - restatement| / max |restatement|` per case, config, mask mode
and output: the float32 reference's own error, the unit of the tolerance (the rules of tests/test_marginal_gpu.py).

Tolerances
  * float32 runs, every output: scaled error `max |got - f64| / max |f64|` at most GATE = max(4 * e_ref, 32 * 2^-24).
  * fp16 / bf16 runs (hidden rounded first, restatement on the rounded values): y is requested as float32 and meets the same GATE, and
    so does d log_scaler (a float32 sum); d hidden is cast to the format of hidden, so elementwise
    `|g - g64| <= h * |g64| + GATE * max |g64|` (+ 2^-24 for fp16 subnormals) with h = 2^-11 (fp16) or 2^-8 (bf16), half an ulp.
  * every value of the fixture's inputs is a multiple of 1/64 (1/8 for the gradients) in [-1, 1]: sums over L are exact in float32 in
    any order, so a, y and d hidden are compared BYTE FOR BYTE across chunkings, mask dtypes, alignments and graph replay.
The fully masked row of `mid` (the only entries the reference cannot vouch for: its gradient there is NaN) must be exact zeros.
Each check prints `POOLERR <case> <cfg> <mode> <dtype> <output> err=... gate=...` before it asserts (run with `-s`);
profiles/pooler.json holds the lines of one run on an MI355X.
"""
import ctypes
import functools
import json
import pathlib

import numpy as np
import pytest

import pooler_ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "pooler.npz"
CASES = ["tiny", "mid", "oddh", "wideh", "longl"]
CONFIGS = ["mean_l2_s100", "mean_none", "mean_tanh", "mean_l1", "cls_none", "cls_l2"]  # + "proj" on the fixture's proj_cases
MODES = ["reference", "masked"]
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
def _case(name, cfg, mode, dtype="float32"):
    """(inputs as the GPU sees them, float64 restatement): computed once per combination, shared, never modified."""
    z, params = _fixture()
    conf = params["configs"][cfg]
    proj = conf["projection_size"] is not None
    inp = {k: z[f"{name}__{k}"] for k in ("hidden", "mask", "weight", "bias")}
    inp["hidden"] = _round(inp["hidden"], dtype)
    inp["grad"] = z[f"{name}__grad_p"] if proj else z[f"{name}__grad_h"]
    want = pooler_ref.pool(inp["hidden"], inp["mask"], agg=conf["agg_method"], mode=mode, activation=conf["output_activation"],
                           norm=conf["output_norm"], log_scaler=params["log_scaler"][cfg], weight=inp["weight"] if proj else None,
                           bias=inp["bias"] if proj else None, grad=inp["grad"])
    return inp, want


def _pooler(cfg, H, mode, **kw):
    from vod_amd.pooler import VodPooler

    _, params = _fixture()
    pooler = VodPooler(dict(params["configs"][cfg]), H, mask_mode=mode, **kw).cuda()
    pooler.log_scaler.requires_grad_(True)  # its gradient is checked for every config
    return pooler


def _run(inp, cfg, mode, dtype="float32", *, l_chunk=None, mask_dtype=torch.int64, upstream=1.0, hidden=None, out_dtype=torch.float32):
    """Forward + backward -> dict of raw device tensors (y, d_hidden, d_log_scaler, and dW / db with a projection)."""
    x = (torch.tensor(inp["hidden"], device="cuda", dtype=TDT[dtype]) if hidden is None else hidden).detach().requires_grad_()
    pooler = _pooler(cfg, x.shape[-1], mode, l_chunk=l_chunk, out_dtype=out_dtype)
    if pooler.projection is not None:
        with torch.no_grad():
            pooler.projection.weight.copy_(torch.from_numpy(inp["weight"]))
            pooler.projection.bias.copy_(torch.from_numpy(inp["bias"]))
    mask = torch.tensor(inp["mask"] != 0, device="cuda").to(mask_dtype)
    y = pooler(x, attention_mask=mask)
    assert y.dtype == out_dtype and x.dtype == TDT[dtype]
    g = torch.tensor(inp["grad"], device="cuda").to(y.dtype) * upstream
    y.backward(g)
    assert x.grad.dtype == TDT[dtype] and x.grad.shape == x.shape
    raw = {"y": y.detach(), "d_hidden": x.grad, "d_log_scaler": pooler.log_scaler.grad}
    if pooler.projection is not None:
        raw["dW"], raw["db"] = pooler.projection.weight.grad, pooler.projection.bias.grad
    return raw


def _aggregate(inp, cfg, mode, dtype, l_chunk):
    """The float32 aggregate a [N, H] on its own (what the backward keeps)."""
    from vod_amd import pooler as P

    _, params = _fixture()
    conf = params["configs"][cfg]
    x = torch.tensor(inp["hidden"], device="cuda", dtype=TDT[dtype])
    mask = torch.tensor(inp["mask"] != 0, device="cuda")
    return P._PoolAggregate.apply(x, mask, torch.zeros((), device="cuda"), P.AGG_CODES[conf["agg_method"]], P.MASK_MODES[mode], False, 0, 0,
                                  torch.float32, l_chunk or 0)


def _np(t):
    return t.detach().double().cpu().numpy()


def _same_bytes(a, b):
    """Bitwise equality: NaN-safe, and +0.0 is not -0.0."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _check(name, cfg, mode, dtype, raw, want, scale_by=1.0):
    _, params = _fixture()
    failures = []
    for key, t in raw.items():
        g = _np(t)
        w = np.asarray(want[key], np.float64) * (scale_by if key != "y" else 1.0)
        assert g.shape == w.shape, key
        assert np.isfinite(g).all(), f"{name} {cfg} {mode} {dtype} {key}: non-finite values"
        gate = max(4 * params["e_ref"][name][cfg][mode][key], FLOOR)
        scale = float(np.abs(w).max())
        err = np.abs(g - w)
        if dtype == "float32" or key != "d_hidden":
            e = float(err.max()) / (scale if scale > 0 else 1.0)
            print(f"POOLERR {name} {cfg} {mode} {dtype} {key} err={e:.3e} gate={gate:.3e}")
            if not e <= gate:
                failures.append(f"{key}: scaled error {e:.3e} > {gate:.3e}")
        else:
            bound = HALF_ULP[dtype] * np.abs(w) + gate * scale + (2.0 ** -24 if dtype == "float16" else 0.0)
            worst = float(np.max(err / np.where(bound > 0, bound, 1.0)))
            print(f"POOLERR {name} {cfg} {mode} {dtype} {key} err={float(err.max()):.3e} bound_used={worst:.4f} gate={gate:.3e}")
            if not np.all(err <= bound):
                failures.append(f"{key}: {int((err > bound).sum())} elements beyond the bound (worst {worst:.2f} x)")
    assert not failures, f"{name} {cfg} {mode} {dtype}: " + "; ".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", CASES)
def test_float32_cases_match_the_restatement(name, cfg, mode):
    inp, want = _case(name, cfg, mode)
    _check(name, cfg, mode, "float32", _run(inp, cfg, mode), want)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("name", ["mid", "oddh", "wideh"])
def test_16bit_cases_match_the_restatement_on_rounded_inputs(name, cfg, mode, dtype):
    inp, want = _case(name, cfg, mode, dtype)
    _check(name, cfg, mode, dtype, _run(inp, cfg, mode, dtype), want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["tiny", "mid", "oddh"])
def test_projection_path(name, mode):
    """aggregate -> nn.Linear -> finish: y, d hidden, dW, db and d log_scaler."""
    inp, want = _case(name, "proj", mode)
    raw = _run(inp, "proj", mode)
    assert set(raw) == {"y", "d_hidden", "d_log_scaler", "dW", "db"}
    _check(name, "proj", mode, "float32", raw, want)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("name,chunks", [("mid", [None, 1, 5, 16, 17, 64]), ("longl", [None, 7, 128])])
def test_forced_chunking_gives_the_same_bytes(name, chunks, dtype):
    """Every way of cutting L (one launch, partials + reduce, chunks that do not divide L) gives bitwise the same a, y and d hidden."""
    for cfg in ("mean_l2_s100", "mean_tanh"):
        for mode in MODES:
            inp, want = _case(name, cfg, mode, dtype)
            runs = [(_aggregate(inp, cfg, mode, dtype, c), _run(inp, cfg, mode, dtype, l_chunk=c)) for c in chunks]
            e = pooler_ref.scaled_error(_np(runs[0][0]), want["a"])
            print(f"POOLERR {name} {cfg} {mode} {dtype} a err={e:.3e} gate={FLOOR:.3e}")
            assert e <= FLOOR
            for c, (a, raw) in zip(chunks[1:], runs[1:]):
                assert _same_bytes(a, runs[0][0]), (cfg, mode, c, "a")
                assert _same_bytes(raw["y"], runs[0][1]["y"]), (cfg, mode, c, "y")
                assert _same_bytes(raw["d_hidden"], runs[0][1]["d_hidden"]), (cfg, mode, c, "d_hidden")


def test_mask_element_types_give_the_same_bytes():
    inp, _ = _case("mid", "mean_l2_s100", "masked")
    for mode in MODES:
        base = _run(inp, "mean_l2_s100", mode, mask_dtype=torch.int64)
        for mdt in (torch.bool, torch.uint8, torch.int32):
            got = _run(inp, "mean_l2_s100", mode, mask_dtype=mdt)
            assert all(_same_bytes(got[k], base[k]) for k in base), (mode, mdt)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_fully_masked_row_is_exact_zeros(dtype):
    _, params = _fixture()
    (dead,) = params["nonfinite_rows"]["mid"]
    for cfg in ("mean_l2_s100", "mean_none", "mean_tanh", "mean_l1"):
        for mode in MODES:
            inp, _ = _case("mid", cfg, mode, dtype)
            raw = _run(inp, cfg, mode, dtype, out_dtype=TDT[dtype])
            assert not raw["y"][dead].view(torch.uint8).any() and not raw["d_hidden"][dead].view(torch.uint8).any(), (cfg, mode)
            assert all(torch.isfinite(v).all() for v in raw.values()), (cfg, mode)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_masked_mode_never_reads_padded_positions(dtype):
    """d hidden at padded positions is bytewise zero; NaN / +-inf written over the padded positions of hidden change nothing."""
    for name in ("mid", "longl"):
        inp, _ = _case(name, "mean_l2_s100", "masked", dtype)
        live = torch.tensor(inp["mask"] != 0, device="cuda")
        base = _run(inp, "mean_l2_s100", "masked", dtype)
        assert not base["d_hidden"][~live].reshape(-1).view(torch.uint8).any()
        for poison in (float("nan"), float("inf"), float("-inf")):
            x = torch.tensor(inp["hidden"], device="cuda", dtype=TDT[dtype])
            x[~live] = poison
            got = _run(inp, "mean_l2_s100", "masked", dtype, hidden=x)
            assert _same_bytes(got["y"], base["y"]) and _same_bytes(got["d_hidden"], base["d_hidden"]), (name, poison)


def test_cls_ignores_the_mask_and_touches_only_position_0():
    for cfg in ("cls_none", "cls_l2"):
        inp, _ = _case("mid", cfg, "reference")
        base = _run(inp, cfg, "reference")
        assert not base["d_hidden"][:, 1:].reshape(-1).view(torch.uint8).any()
        assert base["d_hidden"][:, 0].abs().sum() > 0
        other = dict(inp, mask=np.ones_like(inp["mask"]))
        for mode in MODES:
            got = _run(other, cfg, mode)
            assert all(_same_bytes(got[k], base[k]) for k in base), (cfg, mode)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", ["mid", "wideh"])
def test_hidden_view_off_the_16_byte_grid(name, dtype):
    """H * 2 bytes is a multiple of 16 but the view starts 2 bytes past a 16-byte boundary: the same values as the aligned copy."""
    for mode in MODES:
        inp, _ = _case(name, "mean_l2_s100", mode, dtype)
        aligned = torch.tensor(inp["hidden"], device="cuda", dtype=TDT[dtype])
        buf = torch.zeros(aligned.numel() + 16, device="cuda", dtype=TDT[dtype])
        view = buf[1:1 + aligned.numel()].view(aligned.shape)
        view.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 2 and view.is_contiguous()
        assert (aligned.shape[-1] * 2) % 16 == 0
        a, b = _run(inp, "mean_l2_s100", mode, dtype, hidden=aligned), _run(inp, "mean_l2_s100", mode, dtype, hidden=view)
        assert all(_same_bytes(a[k], b[k]) for k in a), mode


def test_upstream_gradient_scales_the_gradients():
    for cfg, name in (("mean_l2_s100", "mid"), ("proj", "mid")):
        inp, want = _case(name, cfg, "reference")
        raw = _run(inp, cfg, "reference", upstream=3.0)
        _check(name, cfg, "reference", "float32", raw, want, scale_by=3.0)


def test_two_runs_and_a_graph_replay_give_the_same_bytes():
    inp, _ = _case("longl", "mean_l2_s100", "masked", "bfloat16")
    for l_chunk in (None, 7):  # the single-launch path and partials + reduce
        a = _run(inp, "mean_l2_s100", "masked", "bfloat16", l_chunk=l_chunk)
        b = _run(inp, "mean_l2_s100", "masked", "bfloat16", l_chunk=l_chunk)
        assert all(_same_bytes(a[k], b[k]) for k in a)
        pooler = _pooler("mean_l2_s100", 64, "masked", l_chunk=l_chunk, out_dtype=torch.float32)
        x = torch.tensor(inp["hidden"], device="cuda", dtype=torch.bfloat16).requires_grad_()
        mask = torch.tensor(inp["mask"] != 0, device="cuda")
        g = torch.tensor(inp["grad"], device="cuda")

        def step():
            y = pooler(x, attention_mask=mask)
            dx, dls = torch.autograd.grad(y, [x, pooler.log_scaler], g)
            return y.detach(), dx, dls

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bytes(out[0], a["y"]) and _same_bytes(out[1], a["d_hidden"]) and _same_bytes(out[2], a["d_log_scaler"])


def test_c_abi_refusals():
    """A too-small workspace, a bad dtype and a bad aggregator code return < 0 with a message; nothing is launched."""
    from vod_amd import _native

    lib = _native.load_library()
    N, L, H = 2, 300, 64
    x = torch.zeros((N, L, H), device="cuda")
    mask = torch.ones((N, L), dtype=torch.uint8, device="cuda")
    ls = torch.zeros(1, device="cuda")
    a, y = torch.empty((N, H), device="cuda"), torch.empty((N, H), device="cuda")
    need = lib.vodhip_pool_workspace_floats(N, L, H, 7)
    assert need == N * 43 * H and lib.vodhip_pool_workspace_floats(N, L, H, 300) == 0
    assert lib.vodhip_pool_workspace_floats(N, L, H, 0) == lib.vodhip_pool_workspace_floats(N, L, H, 0) >= 0
    work = torch.empty((need,), device="cuda")
    stream = _native.current_stream_ptr(x.device)

    def forward(dtype=_native.F32, agg=0, l_chunk=7, work_floats=need, act=0, norm=1, n=N):
        return lib.vodhip_pool_forward(x.data_ptr(), dtype, n, L, H, mask.data_ptr(), 1, agg, 0, 1, act, norm, ls.data_ptr(), l_chunk,
                                       a.data_ptr(), y.data_ptr(), _native.F32, work.data_ptr(), work_floats, stream)

    def message():
        return lib.vodhip_last_error().decode()

    assert forward() == 0
    assert forward(work_floats=need - 1) < 0 and "workspace_floats" in message()
    assert forward(dtype=7) < 0 and "hidden_dtype" in message()
    assert forward(agg=2) < 0 and "aggregator" in message()
    assert forward(act=9) < 0 and "activation" in message()
    assert forward(norm=3) < 0 and "norm" in message()
    assert forward(n=1 << 40) < 0 and "N * L" in message()
    assert lib.vodhip_pool_workspace_floats(1 << 40, L, H, 0) < 0 and "N * L" in message()
    assert lib.vodhip_pool_backward(y.data_ptr(), 5, a.data_ptr(), N, L, H, mask.data_ptr(), 1, 0, 0, 1, 0, 1, ls.data_ptr(), 0,
                                    x.data_ptr(), _native.F32, a.data_ptr(), stream) < 0 and "g_dtype" in message()
    assert lib.vodhip_pool_finish_forward(a.data_ptr(), _native.F32, N, H, 7, 0, ls.data_ptr(), y.data_ptr(), _native.F32, stream) < 0
    assert lib.vodhip_pool_finish_backward(a.data_ptr(), _native.F32, y.data_ptr(), _native.F32, N, H, 0, 0, ls.data_ptr(), y.data_ptr(), 9,
                                           a.data_ptr(), stream) < 0 and "dtype" in message()
    torch.cuda.synchronize()
    with pytest.raises(_native.NativeLibraryError, match="share one GPU"):
        _pooler("mean_none", H, "reference")(x, attention_mask=mask.cpu())


def test_pooled_vectors_feed_the_index_without_a_cast():
    """cls pooling of multiples of 1/64 is exact in fp16: add + search equal the CPU oracle on the restatement's vectors bit for bit."""
    from oracle.flat_ip import flat_ip_topk
    from vod_amd.index import HipFlatIndex

    rng = np.random.default_rng(21)
    n, nq, L, H, k = 64, 8, 4, 64, 10
    sections = (rng.integers(-64, 65, size=(n, L, H)) / 64.0).astype(np.float32)
    queries = (rng.integers(-64, 65, size=(nq, L, H)) / 64.0).astype(np.float32)
    mask = np.ones((n, L), np.int64)
    mask[:, 2:] = 0
    pooler = _pooler("cls_none", H, "reference", out_dtype=torch.float16)
    with torch.no_grad():
        s_vec = pooler(torch.tensor(sections, device="cuda", dtype=torch.bfloat16), attention_mask=torch.tensor(mask, device="cuda"))
        q_vec = pooler(torch.tensor(queries, device="cuda", dtype=torch.bfloat16), attention_mask=torch.tensor(mask[:nq], device="cuda"))
    want_s = pooler_ref.pool(sections, mask, agg="cls")["y"]
    want_q = pooler_ref.pool(queries, mask[:nq], agg="cls")["y"]
    assert s_vec.dtype == torch.float16 and np.array_equal(_np(s_vec), want_s) and np.array_equal(_np(q_vec), want_q)
    with HipFlatIndex(H, n, dtype=torch.float16, device=0) as ix:
        ix.add(s_vec)
        scores, ids = ix.search(q_vec, k)
    ref_scores, ref_ids = flat_ip_topk(want_q.astype(np.float16), want_s.astype(np.float16), k)
    assert np.array_equal(ids.cpu().numpy(), ref_ids) and np.array_equal(scores.cpu().numpy(), ref_scores)
