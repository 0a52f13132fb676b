#!/usr/bin/env python3
"""What does the gradient of log Z cost?  `HipFlatIndex.posterior_mean` over a 1 M x 768 fp16 store and over a 1 M x 64 one, at nq 256
and 1024, in one process on one device, alternating inside every repeat with two yardsticks:
  log_partition  the forward-only call of the same batch (its three launches are the first half of posterior_mean);
  torch          THE YARDSTICK a user would write today, two passes over chunks of the stored rows: `torch.logsumexp(beta * q16 @
                 x_chunk.T)` folded with `torch.logaddexp`, then `exp(beta * q16 @ x_chunk.T - log Z) @ x_chunk` summed over the chunks
                 (the softmax of a chunk against the global normaliser) - it materialises an nq x chunk block twice per chunk.
Timing as tools/bench_log_partition.py: every side warmed at every shape, a repeat is device milliseconds between two events around `inner`
back-to-back calls, medians with the minimum and maximum over the repeats.  CALL times on the current stream, not kernel times.
Reported per shape: the times, the multiple of log_partition's time next to the cost model's prediction (DESIGN.md 4 "Posterior mean":
ceil(dim_pad / 256) + 2 K-loop equivalents against 1), the ratio to torch, the largest |mean - torch's| and the verdict.  Then the measured
error maxima against float64 on the Gaussian shapes of tests/test_posterior_mean_gpu.py, as a share of the derived bound
(tests/posterior_ref.py::device_bound).
usage: python tools/bench_posterior_mean.py [--out profiles/posterior_mean.json] [--rows 1000000]"""
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
from vod_amd.index import HipFlatIndex  # noqa: E402

BATCHES = (256, 1024)
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


def torch_mean(q16, x, beta, chunk):
    log_z = None
    for lo in range(0, x.shape[0], chunk):
        part = torch.logsumexp(beta * (q16 @ x[lo : lo + chunk].T).float(), dim=1)
        log_z = part if log_z is None else torch.logaddexp(log_z, part)
    mean = torch.zeros((q16.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        xc = x[lo : lo + chunk]
        p = torch.exp(beta * (q16 @ xc.T).float() - log_z[:, None])
        mean += (p.to(x.dtype) @ xc).float()
    return mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/posterior_mean.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_mean.py needs the GPU: there is no CPU path to time")

    g = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "store": "float16", "repeats": args.repeats, "window_s": args.window,
              "torch_chunk_rows": args.chunk, "shapes": {}}
    for dim in (768, 64):
        with HipFlatIndex(dim, args.rows, dtype=torch.float16, device=0) as ix:
            for lo in range(0, args.rows, 250_000):
                ix.add(torch.randn((min(250_000, args.rows - lo), dim), generator=g, device=dev).half())
            x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
            beta = float(torch.tensor(dim ** -0.5, dtype=torch.float32))
            model = ((dim + 63) // 64 * 64 + 255) // 256 + 2  # K loops per column chunk + the second product + the partition scan
            for nq in BATCHES:
                q = torch.randn((nq, dim), generator=g, device=dev)
                q16 = q.half()
                out = tuple(torch.empty((nq,), dtype=torch.float32, device=dev) for _ in range(2))
                out3 = out + (torch.empty((nq, dim), dtype=torch.float32, device=dev),)
                sides = {
                    "posterior_mean": lambda: ix.posterior_mean(q, temperature=1.0 / beta, out=out3),
                    "log_partition": lambda: ix.log_partition(q, temperature=1.0 / beta, out=out),
                    "torch": lambda: torch_mean(q16, x, beta, args.chunk),
                }
                diff = (sides["posterior_mean"]().mean.double() - sides["torch"]().double()).abs().max().item()
                inner = {}
                for name, fn in sides.items():
                    for _ in range(args.warmup):
                        fn()
                    torch.cuda.synchronize()
                    inner[name] = max(1, int(args.window * 1e3 / max(device_ms(fn, 3), 1e-3)) + 1)
                ms = {name: [] for name in sides}
                for _ in range(args.repeats):
                    for name, fn in sides.items():  # alternating: every repeat times every side once
                        ms[name].append(device_ms(fn, inner[name]))
                r = {name: summary(v) for name, v in ms.items()}
                pm, lp, th = r["posterior_mean"], r["log_partition"], r["torch"]
                spread = max(pm["max_ms"] - pm["min_ms"], th["max_ms"] - th["min_ms"])
                flop = 2.0 * nq * args.rows * dim
                r.update({
                    "nq": nq, "dim": dim, "beta": beta, "inner": inner, "useful_flop": 2 * flop,
                    "useful_tflops": 2 * flop / (pm["median_ms"] * 1e-3) / 1e12,
                    "multiple_of_log_partition": pm["median_ms"] / lp["median_ms"], "cost_model_multiple": model,
                    "speedup_vs_torch": th["median_ms"] / pm["median_ms"], "spread_ms": spread, "max_abs_diff_vs_torch": diff,
                    "verdict": "faster than torch by more than the spread" if pm["median_ms"] + spread < th["median_ms"] else "NOT faster than torch",
                })
                result["shapes"][f"dim{dim}_nq{nq}"] = r
                print(f"dim {dim} nq {nq}: posterior_mean {pm['median_ms']:.3f} ms [{pm['min_ms']:.3f}, {pm['max_ms']:.3f}]  log_partition "
                      f"{lp['median_ms']:.3f} ms [{lp['min_ms']:.3f}, {lp['max_ms']:.3f}]  x{r['multiple_of_log_partition']:.2f} (model x{model})  "
                      f"torch {th['median_ms']:.3f} ms [{th['min_ms']:.3f}, {th['max_ms']:.3f}]  {r['speedup_vs_torch']:.2f} x torch  "
                      f"|diff| {diff:.2e}  {r['verdict']}", flush=True)
            del x

    # measured error against float64 on the Gaussian shapes of tests/test_posterior_mean_gpu.py, and its share of the derived bound
    import posterior_ref as R  # noqa: E402  (tests/)
    from test_l2_cpu import GAUSS_CASES, gauss_case  # noqa: E402

    result["accuracy"] = {}
    for dim, dtype, seed in GAUSS_CASES:
        qa, xa = gauss_case(dim, seed)
        b = float(np.float32(1.0 / np.sqrt(dim)))
        with HipFlatIndex(dim, len(xa), dtype=getattr(torch, dtype), device=0) as small:
            small.add(xa)
            got = small.posterior_mean(torch.from_numpy(qa).to(dev), temperature=1.0 / b).mean.cpu().numpy().astype(np.float64)
        ref, _, _ = R.posterior_mean(qa, xa, dtype, b)
        bound = R.device_bound(qa, xa, dtype, b, dot=True)
        err = np.abs(got - ref)
        result["accuracy"][f"gauss_{len(xa)}x{dim}_{dtype}"] = {"beta": b, "max_abs_err_mean": float(err.max()),
                                                                 "max_err_over_bound": float((err / bound).max())}
    print(json.dumps(result["accuracy"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
