#!/usr/bin/env python3
"""What does the monitor update next to the loss cost?  C5 shapes (64 x 32 and 64 x 2048), the shipped metric list.

Times, in one process on one device (median wall microseconds per call, including a device synchronisation, as tools/probe_h5_graph.py):
  device_eager      `vod_amd.monitoring.RetrievalMonitor.update` on existing scores (two launches, no host sync)
  device_events     the same, device time between two events around 50 back-to-back updates
  step_replay       a replay of `GraphedRetrievalStep` without / with the monitor captured behind the loss (the difference is the update)
  reference_ops     a torch restatement of the reference's op sequence (monitor.py:93-105, functional.py, aggregator.py:43-50: argsort, two
                    gathers, the per-metric kernels, and per metric the boolean-index `values[~isnan(values)]` + `numel() == 0`), with
                    the number of host synchronisations it performs per update counted under sync-debug mode "warn"
usage: python tools/bench_monitor.py [--out profiles/r08_monitor.txt]"""
import argparse
import json
import pathlib
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd.gradients import GraphedRetrievalStep, RetrievalGradients  # noqa: E402
from vod_amd.monitoring import RetrievalMonitor, parse_metric_name  # noqa: E402

METRICS = ["kldiv", "ndcg_10", "mrr_10", "hitrate_01", "hitrate_03", "hitrate_10"]
dev = torch.device("cuda", 0)
B, H = 64, 768


def wall(fn, n=200, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def device_us(fn, n=50, reps=9):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / n)
    return statistics.median(out)


# ---- the reference's op sequence, restated in torch (no reference code is imported) ------------------------------------------------
def _rank(relevances, scores):
    n_pos = (relevances > 0).sum(dim=-1)
    mask = scores.isnan() | (scores.isinf() & (scores > 0))
    scores = scores.masked_fill(mask, -torch.inf)
    relevances = relevances.masked_fill(mask, 0)
    ids = torch.argsort(scores, dim=-1, descending=True)
    return torch.gather(relevances, -1, ids), torch.gather(scores, -1, ids), n_pos


def _metric(name, rr, rs, n_pos):
    if name == "mrr":
        ids = torch.arange(rr.shape[-1], device=rr.device)
        first = torch.where(rr > 0, ids, 1 + ids.max()).argmin(dim=-1)
        return torch.where((rr > 0).sum(dim=-1) > 0, 1.0 / (1 + first), 0)
    if name == "hitrate":
        return (rr > 0).any(dim=-1)
    if name == "ndcg":
        r = rr.to(rs)
        lg = torch.arange(2, r.shape[-1] + 2, device=rs.device, dtype=rs.dtype).log2()
        dcg = torch.sum(r / lg, dim=-1)
        idcg = torch.sum(torch.sort(r, descending=True, dim=-1).values / lg, dim=-1)
        return torch.where(idcg > 0, dcg / idcg, 0)
    if name == "kldiv":
        fin = torch.isfinite(rs)
        n_p = (rr > 0).sum(dim=-1)
        r = rr.to(rs)
        data = r.masked_fill(r <= 0, -torch.inf).log_softmax(dim=-1)
        data = torch.where((n_p > 0).unsqueeze(-1), data, fin.sum(dim=-1, keepdim=True))
        model = rs.masked_fill(~fin, -torch.inf).log_softmax(dim=-1)
        kl = torch.where(data.isfinite() & model.isfinite(), data.exp() * (data - model), 0.0).sum(dim=-1)
        return torch.where(n_p > 0, kl, torch.nan)
    raise KeyError(name)


class _RestatedMonitor:
    def __init__(self, metrics):
        self.ops = {m: parse_metric_name(m) for m in metrics}
        self.total = {m: torch.zeros(1, dtype=torch.float64, device=dev) for m in metrics}
        self.count = {m: torch.zeros(1, dtype=torch.float64, device=dev) for m in metrics}

    @torch.no_grad()
    def update(self, relevances, scores):
        rr, rs, n_pos = _rank(relevances, scores)
        for key, (name, topk) in self.ops.items():
            values = _metric(name, rr[..., :topk], rs[..., :topk], n_pos)
            keep = values[~torch.isnan(values)]   # boolean index: a host synchronisation
            if keep.numel() == 0:
                continue
            self.total[key] += keep.sum()
            self.count[key] += keep.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "metrics": METRICS, "unit": "microseconds, median"}
    for name, D, three_d in (("64x32", 32, True), ("64x2048", 2048, False)):
        g = torch.Generator().manual_seed(0)
        scores = torch.randn((B, D), generator=g).to(dev)
        rel = (torch.rand((B, D), generator=g) < 0.05).long().to(dev)
        rel[:, 0] = 1
        batch, output = {"section__relevance": rel}, {"retriever_scores": scores}
        mon = RetrievalMonitor(METRICS)
        r = {"device_eager_wall_us": wall(lambda: mon.update(batch, output)), "device_events_us": device_us(lambda: mon.update(batch, output))}
        ref = _RestatedMonitor(METRICS)
        r["reference_ops_wall_us"] = wall(lambda: ref.update(rel, scores))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            ref.update(rel, scores)
        n_ref = len(caught)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            mon.update(batch, output)
        torch.cuda.set_sync_debug_mode("default")
        r["reference_ops_host_syncs"], r["device_host_syncs"] = n_ref, len(caught)
        # the update inside the captured training step
        kw = dict(batch_size=B, n_sections=D, hidden=H, sections_3d=three_d, device=0)
        plain = GraphedRetrievalStep(RetrievalGradients(), **kw)
        with_mon = GraphedRetrievalStep(RetrievalGradients(), monitor=RetrievalMonitor(METRICS), **kw)
        for st in (plain, with_mon):
            with torch.no_grad():
                st.query_encoding.copy_(torch.randn(st.query_encoding.shape, generator=g).to(dev))
                st.section_encoding.copy_(torch.randn(st.section_encoding.shape, generator=g).to(dev))
                st.batch["section__relevance"].copy_(rel)
        r["step_replay_wall_us"] = wall(plain.replay)
        r["step_replay_with_monitor_wall_us"] = wall(with_mon.replay)
        r["step_replay_device_us"] = device_us(plain.replay)
        r["step_replay_with_monitor_device_us"] = device_us(with_mon.replay)
        rec[name] = {k: (round(v, 1) if isinstance(v, float) else v) for k, v in r.items()}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        pathlib.Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
