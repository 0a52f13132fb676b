#!/usr/bin/env python3
"""What does the weighted sum of listed rows - the backward of `score_ids` - cost?  The store and the two shapes of
tools/bench_score_ids.py: 1 M x 768 fp16 rows, uniformly random listed ids, float32 weights and queries,
  collate   64 queries x  385 listed ids
  rerank  1024 queries x 1000 listed ids   (1.57 GB of gathered rows)

In one process on one device, alternating the sides inside every repeat (device milliseconds between two events around `--inner`
back-to-back calls, after `--warmup` untimed calls of each; medians with the minimum and maximum over the repeats = the run-to-run
spread of this run).  These are CALL times on the current stream - the kernels plus their launches - not kernel times.
  sum_ids       `sum_ids(ids, w)`: sum_listed_kernel + the fold of the chunks' partial sums
  score_ids     the forward of the same shape, `score_ids(q, ids)`: context for the cost model below
  torch_bmm     THE YARDSTICK of sum_ids: `torch.bmm(w16.unsqueeze(1), x[ids])` over the stored fp16 rows - it materialises the gather
  torch_bag     `torch.nn.functional.embedding_bag(ids, x, per_sample_weights=w16, mode="sum")`, where this build runs it (else null)
  step          the full step `listed_scores(q, ids).backward(g)`
  torch_step    THE YARDSTICK of the step: torch autograd through `torch.bmm(x[ids], q16.unsqueeze(2))` (gradient to the query only)
Gate (`verdict`, the rule of bench_score_ids.py): sum_ids and the step must not be slower than their yardsticks at either shape beyond
the spread observed in the run.  No time is fixed in advance.
Context only: `sum_over_score` = sum_ids / score_ids against `model_ratio` = (gathered + 2 * partial + out bytes) / gathered bytes
(the partials are written and read once); `gather_tbs` = nq * m * 768 * 2 bytes over the sum_ids time (the microarchitecture guide's
5.5-5.8 TB/s for register-gathered 1.1-2.3 KB rows is a figure of ANOTHER kernel).
`accuracy`: on Gaussian data (4096 rows; dim 768 and 4096, both store dtypes, N(0, 1) and softmax weights, 9 x 1000 slots) the largest
|device - float64| over the derived bound of tests/sum_ids_ref.py, per case - recorded, never used to set the bound.
usage: python tools/bench_sum_ids.py [--out profiles/sum_ids.json] [--rows 1000000]"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sum_ids_ref  # noqa: E402
from vod_amd.index import HipFlatIndex  # noqa: E402

DIM = 768
SHAPES = {"collate": (64, 385), "rerank": (1024, 1000)}
CHUNK = 32  # slots of a sum workgroup (kernels_listed.hip, SC)
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


def verdict(ours, yard):
    spread = max(ours["max_ms"] - ours["min_ms"], yard["max_ms"] - yard["min_ms"])
    return spread, "not slower than torch" if ours["median_ms"] <= yard["median_ms"] + spread else "SLOWER than torch"


def accuracy():
    out = {}
    for dim in (768, 4096):
        x = torch.randn(4096, dim, generator=torch.Generator().manual_seed(dim)).numpy()
        rng = np.random.default_rng(dim)
        ids = rng.integers(0, len(x), size=(9, 1000)).astype(np.int64)
        z = rng.standard_normal(ids.shape) * 3
        kinds = {"normal": rng.standard_normal(ids.shape).astype(np.float32),
                 "softmax": (np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)).astype(np.float32)}
        for name, dt in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
            with HipFlatIndex(dim, len(x), dtype=dt, device=0) as ix:
                ix.add(x)
                plane = ix.stored_rows().double().cpu().numpy()
                for kind, w in kinds.items():
                    got = ix.sum_ids(ids, w).double().cpu().numpy()
                    ref, bound = sum_ids_ref.sum_ids(plane, ids, w)
                    out[f"dim{dim}_{name}_{kind}"] = {"max_abs_err": float(np.abs(got - ref).max()),
                                                      "max_fraction_of_bound": float((np.abs(got - ref) / bound).max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sum_ids.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sum_ids.py needs the GPU: there is no CPU path to time")

    ix = HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0)
    g = torch.Generator(device=dev).manual_seed(0)
    for lo in range(0, args.rows, 250_000):
        ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=g, device=dev).half())
    x = ix.stored_rows()  # the yardsticks read the very rows the kernel reads
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "inner": args.inner, "shapes": {}}
    for name, (nq, m) in SHAPES.items():
        q = torch.randn((nq, DIM), generator=g, device=dev)
        ids = torch.randint(0, args.rows, (nq, m), generator=g, device=dev)
        w = torch.randn((nq, m), generator=g, device=dev)
        q16, w16 = q.half(), w.half()
        out = torch.empty((nq, DIM), dtype=torch.float32, device=dev)
        scores = torch.empty((nq, m), dtype=torch.float32, device=dev)
        offsets = torch.arange(0, nq * m, m, device=dev)
        q_leaf, q16_leaf = q.clone().requires_grad_(), q16.clone().requires_grad_()

        def step():
            q_leaf.grad = None
            ix.listed_scores(q_leaf, ids).backward(w)

        def torch_step():
            q16_leaf.grad = None
            torch.bmm(x[ids], q16_leaf.unsqueeze(2)).squeeze(2).backward(w16)

        sides = {
            "sum_ids": lambda: ix.sum_ids(ids, w, out=out),
            "score_ids": lambda: ix.score_ids(q, ids, out=scores),
            "torch_bmm": lambda: torch.bmm(w16.unsqueeze(1), x[ids]).squeeze(1),
            "torch_bag": lambda: torch.nn.functional.embedding_bag(ids.reshape(-1), x, offsets, per_sample_weights=w16.reshape(-1), mode="sum"),
            "step": step,
            "torch_step": torch_step,
        }
        try:
            sides["torch_bag"]()
            torch.cuda.synchronize()
        except Exception as e:  # not every build runs the weighted fp16 form on the device
            print(f"{name}: embedding_bag does not run here ({type(e).__name__}: {str(e)[:120]})", flush=True)
            del sides["torch_bag"]
        # the yardstick sums fp16 weights in fp16 outputs: compare against the kernel fed the same (rounded) weights
        diff = (ix.sum_ids(ids, w16.float()).double() - sides["torch_bmm"]().double()).abs().max().item()
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(args.repeats):
            for k, fn in sides.items():  # alternating: every repeat times every side once
                ms[k].append(device_ms(fn, args.inner))
        r = {k: summary(v) for k, v in ms.items()}
        r.setdefault("torch_bag", None)
        gathered = nq * m * DIM * 2
        chunks = (m + CHUNK - 1) // CHUNK
        partial = nq * chunks * DIM * 4 if chunks > 1 else 0
        spread, v = verdict(r["sum_ids"], r["torch_bmm"])
        step_spread, step_v = verdict(r["step"], r["torch_step"])
        r.update({
            "nq": nq, "m": m, "gathered_bytes": gathered, "partial_bytes": partial, "out_bytes": nq * DIM * 4,
            "max_abs_diff_vs_torch_bmm": diff,
            "gather_tbs": gathered / (r["sum_ids"]["median_ms"] * 1e-3) / 1e12,
            "speedup_vs_torch_bmm": r["torch_bmm"]["median_ms"] / r["sum_ids"]["median_ms"],
            "step_speedup_vs_torch": r["torch_step"]["median_ms"] / r["step"]["median_ms"],
            "sum_over_score": r["sum_ids"]["median_ms"] / r["score_ids"]["median_ms"],
            "model_ratio": (gathered + 2 * partial + nq * DIM * 4) / gathered,
            "spread_ms": spread, "verdict": v, "step_spread_ms": step_spread, "step_verdict": step_v,
        })
        result["shapes"][name] = r
        bag = "n/a" if r["torch_bag"] is None else f"{r['torch_bag']['median_ms']:.4f}"
        print(f"{name}: sum_ids {r['sum_ids']['median_ms']:.4f} ms [{r['sum_ids']['min_ms']:.4f}, {r['sum_ids']['max_ms']:.4f}]  "
              f"torch_bmm {r['torch_bmm']['median_ms']:.4f} ms [{r['torch_bmm']['min_ms']:.4f}, {r['torch_bmm']['max_ms']:.4f}]  "
              f"torch_bag {bag} ms  score_ids {r['score_ids']['median_ms']:.4f} ms  sum/score {r['sum_over_score']:.2f} (model "
              f"{r['model_ratio']:.2f})  {r['gather_tbs']:.2f} TB/s  |diff| {diff:.2e}  {v}", flush=True)
        print(f"{name}: step {r['step']['median_ms']:.4f} ms [{r['step']['min_ms']:.4f}, {r['step']['max_ms']:.4f}]  "
              f"torch_step {r['torch_step']['median_ms']:.4f} ms [{r['torch_step']['min_ms']:.4f}, {r['torch_step']['max_ms']:.4f}]  {step_v}",
              flush=True)
    ix.close()
    del x
    result["accuracy"] = accuracy()
    for k, v in result["accuracy"].items():
        print(f"accuracy {k}: {v['max_abs_err']:.3e}, {v['max_fraction_of_bound']:.3f} of the bound", flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
