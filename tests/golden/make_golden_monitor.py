"""Generate tests/golden/monitor_metrics.npz by RUNNING the reference's monitoring modules (build container only):

    python tests/golden/make_golden_monitor.py

The fixture is data: seeded inputs, what the reference computed for them, and the generator's parameters (`params_json`).
Reference code exercised (paths relative to the reference's src/):
  per-row values   vod_models/monitoring/functional.py:181-254  all nine `compute_*` at topk in {None, 1, 3, 10}
  monitor run      vod_models/monitoring/monitor.py:73-105 + aggregator.py:26-59, three successive updates in float64
                   (vod_ops/loops/train.py:59), stored as the values of `get()`
  f32_dev_<m>      the largest |reference float32 value - float64 NumPy evaluation of the same formula| for ndcg / kldiv / entropy
                   over every input of the fixture (the restatement of tests/test_monitor_cpu.py)
  sum_dev_<name>   per monitored name: |reference get() - float64 mean of the reference's OWN per-row values|: what the
                   reference's float32 `values.sum()` (aggregator.py:49) costs
"""
from __future__ import annotations

import json
import pathlib
import sys
import warnings

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))          # tests/: the float64 restatement
sys.path.insert(0, str(HERE.parent.parent))   # the repository root: oracle/
import _ref_shim  # noqa: E402

warnings.filterwarnings("ignore")
M = _ref_shim.install()
import torch  # noqa: E402

import test_monitor_cpu as restatement  # noqa: E402

F = M["functional"]
ALL = ("mrr", "hitrate", "precision", "recall", "ndcg", "kldiv", "min", "max", "entropy")
CUTS = (0, 1, 3, 10)
MONITORED = ["kldiv", "ndcg_10", "mrr_10", "hitrate_01", "hitrate_03", "hitrate_10", "recall_10", "precision_03", "min", "max",
             "entropy", "ndcg", "entropy_10", "kldiv_03"]


def make_input(seed: int, B: int, N: int):
    """The corner rows of `gen_metrics` (make_golden.py) at any width; tied scores carry equal relevances."""
    rng = np.random.default_rng(seed)
    scores = rng.normal(size=(B, N)).astype(np.float32)
    rel = (rng.random((B, N)) < 0.2).astype(np.int64) * rng.integers(1, 4, size=(B, N))  # graded relevances 0..3
    scores[1, :5] = np.nan
    scores[2, 3] = np.inf          # masked by the reference (+inf), its relevance zeroed
    rel[2, 3] = 3
    scores[3, N // 2:] = -np.inf   # padding: ranked last, NOT masked, relevance 0
    rel[3, N // 2:] = 0
    rel[4] = 0                     # a row without positives
    rel[5] = 0
    rel[5, 2] = 2
    scores[5, 2] = np.nan          # the only positive is masked
    scores[0, :4] = scores[0, 4]   # ties
    rel[0, :5] = rel[0, 4]
    scores[0, 7] = -0.0
    scores[0, 9] = 0.0             # both signs of zero: a tie
    rel[0, 7] = rel[0, 9] = 1
    rel[1, 0] = 3                  # a masked positive next to unmasked ones
    return scores, rel


def nan_heavy(seed: int, B: int, N: int):
    scores, rel = make_input(seed, B, N)
    scores[6:] = np.nan            # whole rows masked: kldiv / precision NaN, recall 0 or NaN
    rel[7] = 0
    return scores, rel


def dev_against_float64(metric, rel, scores, tk, ref) -> float:
    got = restatement.restate(metric, rel, scores, tk, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (metric, tk)
    ok = ~np.isnan(ref)
    return float(np.abs(got[ok] - ref[ok].astype(np.float64)).max(initial=0.0))


def run_monitor(batches):
    """The reference's RetrievalMonitor when it imports under the shim, else its update driven by hand in the order of monitor.py:93-105."""
    per_update_values = []
    try:
        import importlib

        mon_mod = importlib.import_module("vod_models.monitoring.monitor")
        RealmBatch = M["batch"].RealmBatch
        monitor = mon_mod.RetrievalMonitor(MONITORED)
        monitor.to(dtype=torch.float64)
        dummy = torch.zeros(1, dtype=torch.long)
        for scores, rel in batches:
            nq, nd = scores.shape
            batch = RealmBatch(
                query__input_ids=dummy, query__attention_mask=dummy, query__id="", query__subset_ids=[], query__section_ids=[],
                section__input_ids=dummy, section__attention_mask=dummy, section__id="",
                section__relevance=torch.from_numpy(rel), section__idx=torch.zeros(nq, nd, dtype=torch.long),
                section__score=torch.zeros(nq, nd), section__sparse=None, section__dense=None, section__log_weight=torch.zeros(nq, nd),
                section__lse_pos=torch.zeros(nq), section__lse_neg=torch.zeros(nq),
            )
            monitor.update(batch, {"loss": torch.zeros(()), "retriever_scores": torch.from_numpy(scores)})
        how = "vod_models.monitoring.monitor.RetrievalMonitor"
        got = {k: float(v) for k, v in monitor.get().items()}
    except Exception as exc:  # noqa: BLE001 - vod_types does not import under every container's pydantic
        how = f"by hand (monitor.py:93-105; the class did not run under the shim: {type(exc).__name__})"
        mon_mod = None
        agg_mod = __import__("importlib").import_module("vod_models.monitoring.aggregator")
        aggs = {m: agg_mod.MeanAggregator().to(dtype=torch.float64) for m in MONITORED}
        for scores, rel in batches:
            rr, rs, n_pos = F.prepare_for_metric_computation(relevances=torch.from_numpy(rel), scores=torch.from_numpy(scores), topk=-1)
            for name in MONITORED:
                base, tk = restatement_parse(name)
                aggs[name].update(getattr(F, f"_compute_{base}")(ranked_relevances=rr[..., :tk], ranked_scores=rs[..., :tk], n_positives=n_pos))
        got = {k: float(a.get()) for k, a in aggs.items()}
    # the float64 mean of the reference's own per-row values, for sum_dev_<name>
    tot = {m: [0.0, 0] for m in MONITORED}
    for scores, rel in batches:
        for name in MONITORED:
            base, tk = restatement_parse(name)
            v = getattr(F, f"compute_{base}").compute(relevances=torch.from_numpy(rel), scores=torch.from_numpy(scores), topk=tk)
            v = v.to(torch.float64).numpy()
            per_update_values.append(v)
            tot[name][0] += float(v[~np.isnan(v)].sum())
            tot[name][1] += int((~np.isnan(v)).sum())
    mean64 = {m: (t / c if c else float("nan")) for m, (t, c) in tot.items()}
    return how, got, mean64


def restatement_parse(name: str):
    if "_" in name:
        *parts, k = name.split("_")
        return "_".join(parts), int(k)
    return name, None


def main() -> None:
    inputs = {"a": make_input(4243, 12, 24), "b": make_input(4244, 6, 300)}
    batches = [inputs["a"], inputs["b"], nan_heavy(4245, 8, 24)]
    arrays: dict[str, np.ndarray] = {}
    dev = {"ndcg": 0.0, "kldiv": 0.0, "entropy": 0.0}
    for key, (scores, rel) in inputs.items():
        arrays[f"scores_{key}"], arrays[f"relevances_{key}"] = scores, rel
    everything = list(inputs.items()) + [("m2", batches[2])]
    for key, (scores, rel) in everything:
        for name in ALL:
            fn = getattr(F, f"compute_{name}")
            for tk in CUTS:
                out = fn.compute(relevances=torch.from_numpy(rel), scores=torch.from_numpy(scores), topk=tk or None)
                assert out.dtype in (torch.float32, torch.bool), (name, out.dtype)
                val = out.numpy()
                if key in inputs:
                    arrays[f"{key}_{name}_top{tk}"] = val
                if name in dev:
                    dev[name] = max(dev[name], dev_against_float64(name, rel, scores, tk, val))
    for name, d in dev.items():
        arrays[f"f32_dev_{name}"] = np.float64(d)
    how, got, mean64 = run_monitor(batches)
    arrays["mon_scores_2"], arrays["mon_relevances_2"] = batches[2]
    for name in MONITORED:
        arrays[f"mon_get_{name}"] = np.float64(got[name])
        arrays[f"sum_dev_{name}"] = np.float64(abs(got[name] - mean64[name]) if np.isfinite(mean64[name]) else 0.0)
        assert np.isnan(got[name]) == np.isnan(mean64[name]) or np.isinf(mean64[name]), name
    params = {"seeds": {"a": 4243, "b": 4244, "nan_heavy": 4245}, "shapes": {"a": [12, 24], "b": [6, 300], "nan_heavy": [8, 24]},
              "topk": list(CUTS), "metrics": list(ALL), "monitored": MONITORED, "monitor_batches": ["a", "b", "mon_*_2"],
              "monitor_dtype": "float64", "monitor_run": how, "fn": "vod_models.monitoring.functional.compute_*"}
    arrays["params_json"] = np.array(json.dumps(params, sort_keys=True))
    np.savez_compressed(HERE / "monitor_metrics.npz", **arrays)
    size = (HERE / "monitor_metrics.npz").stat().st_size
    print(f"monitor_metrics.npz: {len(arrays)} arrays, {size / 1024:.1f} KiB; monitor run: {how}")
    print({k: float(v) for k, v in arrays.items() if k.startswith(("f32_dev", "sum_dev", "mon_get"))})


if __name__ == "__main__":
    main()
