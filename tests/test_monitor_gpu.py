"""GPU tests of the device RetrievalMonitor (`vod_amd.monitoring`, `vodhip_retrieval_metrics`).

Comparators: `tests/golden/monitor_metrics.npz` (what the imported reference computed: tests/golden/make_golden_monitor.py),
`oracle.metrics` (recall / precision / hitrate / mrr / ndcg) and the NumPy restatement of tests/test_monitor_cpu.py (kldiv / min /
max / entropy, ndcg in float64).

hitrate / mrr / recall / precision / min / max are one correctly rounded float32 operation on integers or a selection: compared
bit for bit, NaN positions included.  ndcg / kldiv / entropy are compared with the float64 value of the reference's formula; the
bound is the reference's OWN float32 distance from that value - `f32_dev_<metric>` of the fixture, or |float32 oracle - float64
restatement| of a random case - times 4 (device exp / log / log2 are not correctly rounded and the order of the sums differs
from torch's), and never tighter than 4 float32 ulps of the value.  The order among tied scores is the stable sort's (smaller
column first), which is what the oracle does: random inputs carry ties with DIFFERENT relevances."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_monitor_cpu import CLOSE, CUTS, EXACT, restate, ulp32

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
ALL = EXACT + CLOSE


def _name(metric, tk):
    return f"{metric}_{tk:02d}" if tk else metric


def _device_values(rel, scores):
    """Every metric at every cut -> {(metric, tk): float64 array [B]} (36 specs: two calls of <= 32)."""
    from vod_amd.monitoring import compute_metrics

    t_rel, t_sc = torch.from_numpy(rel).cuda(), torch.from_numpy(scores).cuda()
    out = {}
    for group in (ALL[:5], ALL[5:]):
        names = {_name(m, tk): (m, tk) for m in group for tk in CUTS}
        got = compute_metrics(t_rel, t_sc, list(names))
        for n, key in names.items():
            v = got[n]
            assert v.shape == (rel.shape[0],) and v.dtype == (torch.bool if key[0] == "hitrate" else torch.float32)
            out[key] = v.cpu().numpy().astype(np.float64)
    return out


def _assert_close(got, want64, dev, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want64), err_msg=what)
    ok = ~np.isnan(want64)
    tol = np.maximum(4.0 * dev, 4.0 * ulp32(want64[ok]))
    err = np.abs(got[ok] - want64[ok])
    print(f"{what}: max err {err.max(initial=0.0):.3e}, reference's own deviation {dev:.3e}")
    assert (err <= tol).all(), (what, float(err.max()), float(tol.min()))


def test_fixture_parity_every_metric_every_cut():
    g = np.load(GOLDEN / "monitor_metrics.npz")
    for inp in ("a", "b"):
        rel, scores = g[f"relevances_{inp}"], g[f"scores_{inp}"]
        got = _device_values(rel, scores)
        for tk in CUTS:
            for metric in EXACT:
                np.testing.assert_array_equal(got[metric, tk], g[f"{inp}_{metric}_top{tk}"].astype(np.float64), err_msg=f"{inp} {metric} top{tk}")
            for metric in CLOSE:
                want64 = restate(metric, rel, scores, tk, np.float64)
                np.testing.assert_array_equal(np.isnan(want64), np.isnan(g[f"{inp}_{metric}_top{tk}"]))  # the reference's NaN rows
                _assert_close(got[metric, tk], want64, float(g[f"f32_dev_{metric}"]), f"{inp} {metric} top{tk}")


def _random_case(rng, B, width):
    scores = (rng.normal(size=(B, width)) * 2).astype(np.float32)
    q = rng.random((B, width)) < 0.3
    scores[q] = np.round(scores[q] * 2) / 2          # ties, with different relevances; both signs of zero among them
    scores[rng.random((B, width)) < 0.05] = -0.0
    scores[rng.random((B, width)) < 0.05] = 0.0
    scores[rng.random((B, width)) < 0.04] = np.nan
    scores[rng.random((B, width)) < 0.02] = np.inf
    scores[rng.random((B, width)) < 0.05] = -np.inf
    rel = (rng.random((B, width)) < 0.25).astype(np.int64) * rng.integers(1, 4, size=(B, width))
    for b in range(B):
        kind = rng.integers(0, 6)
        if kind == 0:
            rel[b] = 0                                # no positives
        elif kind == 1:
            cut = int(rng.integers(0, width + 1))     # a padded tail (some pads keep a relevance: -inf is not masked)
            scores[b, cut:] = -np.inf
            rel[b, cut:] *= rng.random(width - cut) < 0.1
        elif kind == 2 and b % 7 == 0:
            scores[b] = np.nan                        # everything masked
    return scores, rel


@pytest.mark.parametrize("B", [1, 64, 300])
@pytest.mark.parametrize("width", [1, 2, 32, 33, 385, 2048, 4096])
def test_random_parity(B, width):
    rng = np.random.default_rng(1000 * B + width)
    scores, rel = _random_case(rng, B, width)
    got = _device_values(rel, scores)
    for tk in CUTS:
        for metric in EXACT:
            want = np.asarray(restate(metric, rel, scores, tk, np.float32), dtype=np.float64)
            np.testing.assert_array_equal(got[metric, tk], want, err_msg=f"{metric} top{tk}")
        for metric in CLOSE:
            want32 = np.asarray(restate(metric, rel, scores, tk, np.float32), dtype=np.float64)
            want64 = restate(metric, rel, scores, tk, np.float64)
            both = np.isfinite(want32) & np.isfinite(want64)
            dev = float(np.abs(want32[both] - want64[both]).max(initial=0.0))
            _assert_close(got[metric, tk], want64, dev, f"B={B} width={width} {metric} top{tk}")


def _fixture_batches():
    import json

    g = np.load(GOLDEN / "monitor_metrics.npz")
    monitored = json.loads(str(g["params_json"]))["monitored"]
    batches = [(g["scores_a"], g["relevances_a"]), (g["scores_b"], g["relevances_b"]), (g["mon_scores_2"], g["mon_relevances_2"])]
    return g, monitored, batches


def _update(monitor, scores, rel):
    monitor.update({"section__relevance": torch.from_numpy(rel).cuda()}, {"retriever_scores": torch.from_numpy(scores).cuda()})


def test_state_is_the_float64_sum_and_count_of_the_row_values():
    from vod_amd.monitoring import RetrievalMonitor

    g, monitored, batches = _fixture_batches()
    m = RetrievalMonitor(monitored)
    total = np.zeros(len(monitored))
    count = np.zeros(len(monitored))
    for scores, rel in batches:
        _update(m, scores, rel)
        vals = m.last_values(scores.shape[0])
        for i, name in enumerate(monitored):
            v = vals[name].cpu().numpy().astype(np.float64)
            with np.errstate(all="ignore"):
                total[i] += v[~np.isnan(v)].sum()
            count[i] += (~np.isnan(v)).sum()
    state = m.state.cpu().numpy()
    assert state.dtype == np.float64 and state.shape == (len(monitored), 2)
    np.testing.assert_array_equal(state[:, 1], count)
    fin = np.isfinite(total)
    np.testing.assert_array_equal(state[~fin, 0], total[~fin])
    np.testing.assert_allclose(state[fin, 0], total[fin], rtol=1e-12, atol=0)
    # get() against the reference's monitor run over the same three updates
    got = m.get()
    assert list(got) == monitored
    for name in monitored:
        v = got[name]
        assert v.dim() == 0 and v.dtype == torch.float64 and v.is_cuda
        want, base = float(g[f"mon_get_{name}"]), name.split("_")[0]
        if not np.isfinite(want):
            np.testing.assert_array_equal(float(v), want, err_msg=name)
            continue
        # ndcg / kldiv / entropy: the per-row bound; the exact metrics: what the reference's float32 `values.sum()` loses (sum_dev)
        dev = float(g[f"f32_dev_{base}"]) if base in CLOSE else float(g[f"sum_dev_{name}"])
        tol = max(4.0 * dev, 4.0 * float(ulp32(want)))
        print(f"get {name}: err {abs(float(v) - want):.3e} tol {tol:.3e}")
        assert abs(float(v) - want) <= tol, (name, float(v), want, tol)
    # compute() returns the same values and resets
    out = m.compute(synchronize=True)
    assert all(torch.equal(out[n], got[n]) or (torch.isnan(out[n]) and torch.isnan(got[n])) for n in monitored)
    assert float(m.state.abs().sum()) == 0.0


def test_all_nan_spec_leaves_the_count_at_zero():
    from vod_amd.monitoring import RetrievalMonitor

    rng = np.random.default_rng(5)
    scores = rng.normal(size=(9, 40)).astype(np.float32)
    rel = np.zeros((9, 40), dtype=np.int64)  # no positives anywhere: recall = 0 / 0, kldiv = NaN on every row
    m = RetrievalMonitor(["recall_10", "kldiv", "mrr"])
    for _ in range(2):
        _update(m, scores, rel)
    state = m.state.cpu().numpy()
    np.testing.assert_array_equal(state[:2], np.zeros((2, 2)))
    np.testing.assert_array_equal(state[2], [0.0, 18.0])
    got = m.get()
    assert torch.isnan(got["recall_10"]) and torch.isnan(got["kldiv"]) and float(got["mrr"]) == 0.0


def test_two_identical_runs_leave_bit_identical_state():
    from vod_amd.monitoring import RetrievalMonitor

    _, monitored, batches = _fixture_batches()
    rng = np.random.default_rng(11)
    big = _random_case(rng, 300, 385)
    states = []
    for _ in range(2):
        m = RetrievalMonitor(monitored)
        for scores, rel in batches + [big]:
            _update(m, scores, rel)
        states.append(m.state.cpu().numpy().copy())
    assert states[0].tobytes() == states[1].tobytes()


def test_update_performs_no_host_synchronisation():
    from vod_amd.monitoring import RetrievalMonitor

    rng = np.random.default_rng(3)
    scores, rel = _random_case(rng, 64, 385)
    batch = {"section__relevance": torch.from_numpy(rel).cuda()}
    out = {"retriever_scores": torch.from_numpy(scores).cuda()}
    m = RetrievalMonitor(["kldiv", "ndcg_10", "mrr_10", "hitrate_01", "hitrate_03", "hitrate_10"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")  # any host synchronisation inside update() raises
    try:
        for _ in range(3):
            m.update(batch, out)
        mean = m.get()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(m.state[0, 1]) > 0 and set(mean) == set(m.ops)


def test_update_accepts_the_realm_output_of_the_gradients():
    from vod_amd.gradients import RealmOutput
    from vod_amd.monitoring import RetrievalMonitor

    rng = np.random.default_rng(4)
    scores, rel = _random_case(rng, 16, 50)
    a, b = RetrievalMonitor(["mrr_10", "ndcg"]), RetrievalMonitor(["mrr_10", "ndcg"])
    t_sc = torch.from_numpy(scores).cuda()
    _update(a, scores, rel)
    b.update({"section__relevance": torch.from_numpy(rel).cuda()}, RealmOutput(loss=torch.zeros((), device="cuda"), retriever_scores=t_sc))
    assert torch.equal(a.state, b.state)


def test_graphed_step_replays_the_monitor_bit_for_bit():
    from vod_amd.gradients import GraphedRetrievalStep, RetrievalGradients
    from vod_amd.monitoring import RetrievalMonitor

    names = ["kldiv", "ndcg_10", "mrr_10", "hitrate_01", "hitrate_03", "hitrate_10", "entropy", "max"]
    B, D, H = 16, 96, 64
    g = torch.Generator().manual_seed(7)
    steps = []
    for _ in range(3):
        q = torch.randn(B, H, generator=g).cuda()
        s = torch.randn(D, H, generator=g).cuda()
        score = torch.randn(B, D, generator=g).masked_fill(torch.rand(B, D, generator=g) < 0.1, -float("inf"))
        rel = (torch.rand(B, D, generator=g) < 0.2).long() * torch.randint(1, 4, (B, D), generator=g)
        rel[:, 0] = 1
        rel[3] = 0
        batch = {"section__score": score.cuda(), "section__relevance": rel.cuda(), "section__sparse": torch.randn(B, D, generator=g).cuda(),
                 "section__dense": torch.randn(B, D, generator=g).cuda()}
        steps.append((batch, q, s))
    fn = RetrievalGradients()
    eager = RetrievalMonitor(names)
    for batch, q, s in steps:
        out = fn(batch=batch, query_encoding=q.clone().requires_grad_(True), section_encoding=s.clone().requires_grad_(True))
        out.loss.backward()
        eager.update(batch, out)
    graphed = RetrievalMonitor(names)
    step = GraphedRetrievalStep(fn, batch_size=B, n_sections=D, hidden=H, device=0, monitor=graphed)
    assert float(graphed.state.abs().sum()) == 0.0  # the warm-up steps and the capture left no trace
    for batch, q, s in steps:
        step(batch=batch, query_encoding=q, section_encoding=s)
    torch.cuda.synchronize()
    assert float(eager.state[:, 1].sum()) > 0
    assert eager.state.cpu().numpy().tobytes() == graphed.state.cpu().numpy().tobytes()
    # without a monitor the step is what it was
    plain = GraphedRetrievalStep(fn, batch_size=B, n_sections=D, hidden=H, device=0)
    assert plain.monitor is None
    o1, _, _ = plain(batch=steps[0][0], query_encoding=steps[0][1], section_encoding=steps[0][2])
    o2 = fn(batch=steps[0][0], query_encoding=steps[0][1], section_encoding=steps[0][2])
    assert torch.equal(o1.retriever_scores, o2.retriever_scores) and torch.equal(o1.loss, o2.loss)


def test_bad_arguments_are_refused_and_the_next_call_works():
    from vod_amd import _native

    lib = _native.load_library()
    B = 4
    scores = torch.randn(B, 4097, device="cuda")
    rel = torch.ones(B, 4097, dtype=torch.int64, device="cuda")
    values = torch.full((33, B), -7.0, device="cuda")
    stream = _native.current_stream_ptr(scores.device)

    state = torch.zeros((33, 2), dtype=torch.float64, device="cuda")

    def call(width, pairs, n=None, vals=values, st=None, ws=None, ws_bytes=0, rows=B):
        arr = (ctypes.c_int32 * (2 * len(pairs)))(*[x for p in pairs for x in p])
        return lib.vodhip_retrieval_metrics(scores.data_ptr(), rel.data_ptr(), rows, width, arr, len(pairs) if n is None else n,
                                            None if vals is None else vals.data_ptr(), None if st is None else st.data_ptr(),
                                            None if ws is None else ws.data_ptr(), ws_bytes, stream)

    bad = {
        "width 4097": lambda: call(4097, [(0, 0)]),
        "33 specs": lambda: call(64, [(0, 0)] * 33),
        "unknown metric": lambda: call(64, [(99, 0)]),
        "no specs": lambda: call(64, [(0, 0)], n=0),
        "B = 0": lambda: call(64, [(0, 0)], rows=0),
        "nothing to write": lambda: call(64, [(0, 0)], vals=None),
        "no workspace": lambda: call(64, [(0, 0), (1, 0)], vals=None, st=state),
        "workspace too small": lambda: call(64, [(0, 0), (1, 0)], vals=None, st=state, ws=values, ws_bytes=2 * B * 4 - 1),
    }
    for what, fn in bad.items():
        status = fn()
        assert status < 0, what
        assert lib.vodhip_last_error(), what
        with pytest.raises(_native.NativeLibraryError):
            _native.check(status)
    assert call(4097, [(0, 0)]) < 0 and b"4097" in lib.vodhip_last_error()
    assert call(64, [(99, 0)]) < 0 and b"99" in lib.vodhip_last_error()
    torch.cuda.synchronize()
    assert float(values.min()) == -7.0 and float(values.max()) == -7.0 and float(state.abs().sum()) == 0.0  # nothing was launched
    assert call(64, [(1, 0), (0, 10)]) == 0  # hitrate, mrr@10 of rows whose every entry is relevant (row stride 64 of the buffer)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(values[:2].cpu().numpy(), np.ones((2, B), dtype=np.float32))
    # the row values in the caller's workspace, the aggregate in `state`
    assert call(64, [(1, 0), (0, 10)], vals=None, st=state, ws=values, ws_bytes=2 * B * 4) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(state[:2].cpu().numpy(), np.full((2, 2), float(B)))


_TWO_RANKS = """
import os
import sys
import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, {root!r})
from vod_amd.monitoring import RetrievalMonitor

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
names = ["kldiv", "ndcg_10", "mrr_10", "hitrate_01", "recall_10", "entropy"]


def run(r):
    rng = np.random.default_rng(100 + r)
    m = RetrievalMonitor(names)
    for _ in range(2):
        scores = rng.normal(size=(20 + r, 70)).astype(np.float32)
        rel = (rng.random(scores.shape) < 0.2).astype(np.int64)
        rel[1] = 0
        m.update({{"section__relevance": torch.from_numpy(rel).cuda()}}, {{"retriever_scores": torch.from_numpy(scores).cuda()}})
    return m


mine = run(rank)
want = run(0).state + run(1).state
calls = []
real = dist.all_reduce


def counted(*a, **k):
    calls.append(1)
    return real(*a, **k)


dist.all_reduce = counted
mine.synchronize()
dist.all_reduce = real
assert len(calls) == 1, calls
assert torch.equal(mine.state, want), (mine.state, want)
assert float(mine.state[2, 1]) == 82.0  # 2 * (20 + 21) rows on the two ranks
got = mine.compute(synchronize=False)
assert all(torch.isfinite(v) for v in got.values())
dist.barrier()
dist.destroy_process_group()
print(f"rank {{rank}} ok", flush=True)
"""


def test_synchronize_is_one_collective_over_two_ranks(tmp_path):
    """Two gloo ranks share GPU 0 (RCCL refuses two ranks on one device), each with its own updates: after `synchronize()` both
    hold the sum of the two states, and exactly one all-reduce was issued."""
    script = tmp_path / "two_ranks_monitor.py"
    script.write_text(_TWO_RANKS.format(root=str(ROOT)))
    procs = [subprocess.Popen([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29563", RANK=str(r), WORLD_SIZE="2"))
             for r in range(2)]
    try:
        for r, p in enumerate(procs):
            out, err = p.communicate(timeout=300)
            assert p.returncode == 0, err[-2000:]
            assert f"rank {r} ok" in out
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
