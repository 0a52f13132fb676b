#!/usr/bin/env python3
"""What does scoring listed rows cost?  A 1 M x 768 fp16 store, uniformly random listed ids, float32 queries, at the two shapes
`HipFlatIndex.score_ids` exists for:
  collate   64 queries x  385 listed ids   (the merged candidates of a collate batch: 3 engines x 128 + the pad column)
  rerank  1024 queries x 1000 listed ids   (1.57 GB of gathered rows)

In one process on one device, alternating the sides inside every repeat (device milliseconds between two events around `--inner`
back-to-back calls, after `--warmup` untimed calls of each; medians with the minimum and maximum over the repeats = the run-to-run
spread of this run).  These are CALL times on the current stream - the kernel plus its launch - not kernel times.
  aligned   `score_ids(q, ids)`: one launch of score_listed_kernel
  torch     THE YARDSTICK: the same scores by plain torch ops on the same device and data, `torch.bmm(x[ids], q.unsqueeze(2))` over the
            stored fp16 rows and the query rounded to fp16 - it materialises the gather.  The aligned kernel must not be slower than
            this at either shape beyond the spread observed in the run (`verdict`); the largest |aligned - torch| is reported.
  topk      `score_ids(q, ids, k=100)`: score + select, reported separately (the rerank shape lists 1000 ids <= 8192)
Context only, not gates: `gather_tbs` = nq * m * 768 * 2 bytes over the aligned time (the microarchitecture guide's 5.5-5.8 TB/s for
register-gathered 1.1-2.3 KB rows is a figure of ANOTHER kernel, never measured for this one), and `search_ms` = a full
`search(q, 100)` of the same batch over the same store.
usage: python tools/bench_score_ids.py [--out profiles/score_ids.json] [--rows 1000000]"""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd.index import HipFlatIndex  # noqa: E402

DIM = 768
SHAPES = {"collate": (64, 385), "rerank": (1024, 1000)}
dev = torch.device("cuda", 0)


def device_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/score_ids.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score_ids.py needs the GPU: there is no CPU path to time")

    ix = HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0)
    g = torch.Generator(device=dev).manual_seed(0)
    for lo in range(0, args.rows, 250_000):
        ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=g, device=dev).half())
    x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "inner": args.inner, "shapes": {}}
    for name, (nq, m) in SHAPES.items():
        q = torch.randn((nq, DIM), generator=g, device=dev)
        ids = torch.randint(0, args.rows, (nq, m), generator=g, device=dev)
        q16 = q.half()
        out = torch.empty((nq, m), dtype=torch.float32, device=dev)
        topk_out = (torch.empty((nq, 100), dtype=torch.float32, device=dev), torch.empty((nq, 100), dtype=torch.int64, device=dev))
        sides = {
            "aligned": lambda: ix.score_ids(q, ids, out=out),
            "torch": lambda: torch.bmm(x[ids], q16.unsqueeze(2)).squeeze(2),
            "topk": lambda: ix.score_ids(q, ids, 100, out=topk_out),
            "search": lambda: ix.search(q, 100),
        }
        diff = (sides["aligned"]().double() - sides["torch"]().double()).abs().max().item()
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():  # alternating: every repeat times every side once
                ms[k].append(device_ms(fn, args.inner if k != "search" else max(1, args.inner // 5)))
        r = {k: summary(v) for k, v in ms.items()}
        gathered = nq * m * DIM * 2
        spread = max(r["aligned"]["max_ms"] - r["aligned"]["min_ms"], r["torch"]["max_ms"] - r["torch"]["min_ms"])
        r.update({
            "nq": nq, "m": m, "gathered_bytes": gathered, "max_abs_diff_vs_torch": diff,
            "gather_tbs": gathered / (r["aligned"]["median_ms"] * 1e-3) / 1e12,
            "speedup_vs_torch": r["torch"]["median_ms"] / r["aligned"]["median_ms"],
            "spread_ms": spread,
            "verdict": "not slower than torch" if r["aligned"]["median_ms"] <= r["torch"]["median_ms"] + spread else "SLOWER than torch",
        })
        result["shapes"][name] = r
        print(f"{name}: aligned {r['aligned']['median_ms']:.4f} ms [{r['aligned']['min_ms']:.4f}, {r['aligned']['max_ms']:.4f}]  "
              f"torch {r['torch']['median_ms']:.4f} ms [{r['torch']['min_ms']:.4f}, {r['torch']['max_ms']:.4f}]  "
              f"topk {r['topk']['median_ms']:.4f} ms  search {r['search']['median_ms']:.4f} ms  {r['gather_tbs']:.2f} TB/s  "
              f"|diff| {diff:.2e}  {r['verdict']}", flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
