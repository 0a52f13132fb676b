#!/usr/bin/env python3
"""What does the exact normaliser cost?  `HipFlatIndex.log_partition` over a 1 M x 768 fp16 store at nq 256 and 1024, in one process on
one device, alternating inside every repeat with two yardsticks:
  search   `index.search(q, 100)` of the same batch - the scan this one shares its K loop with;
  torch    THE YARDSTICK a user would write today: chunks of the stored rows, `torch.logsumexp(beta * (q16 @ x_chunk.T).float(), 1)`,
           folded over the chunks with `torch.logaddexp` - it materialises an nq x chunk score block per chunk.
Every side is warmed at every shape; a repeat is device milliseconds between two events around `inner` back-to-back calls, with `inner`
sized from the warm-up so that a window lasts at least `--window` seconds; medians with the minimum and maximum over the repeats (the
run-to-run spread of this run).  CALL times on the current stream, not kernel times.
Reported per shape: the times, 2 * nq * N * dim FLOP over the log_partition time as a share of the 2.5 PFLOP/s dense fp16 MFMA peak, the
ratio to `search`, the ratio to torch, the largest |log Z - torch's| over the batch, and the verdict: faster than torch by more than the
spread, or not.
usage: python tools/bench_log_partition.py [--out profiles/log_partition.json] [--rows 1000000]"""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd.index import HipFlatIndex  # noqa: E402

DIM = 768
BATCHES = (256, 1024)
MFMA_PEAK = 2.5e15
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


def torch_log_z(q16, x, beta, chunk):
    acc = None
    for lo in range(0, x.shape[0], chunk):
        part = torch.logsumexp(beta * (q16 @ x[lo : lo + chunk].T).float(), dim=1)
        acc = part if acc is None else torch.logaddexp(acc, part)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/log_partition.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_log_partition.py needs the GPU: there is no CPU path to time")

    ix = HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0)
    g = torch.Generator(device=dev).manual_seed(0)
    for lo in range(0, args.rows, 250_000):
        ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=g, device=dev).half())
    x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
    beta = float(torch.tensor(DIM ** -0.5, dtype=torch.float32))
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "beta": beta,
              "repeats": args.repeats, "window_s": args.window, "torch_chunk_rows": args.chunk, "shapes": {}}
    for nq in BATCHES:
        q = torch.randn((nq, DIM), generator=g, device=dev)
        q16 = q.half()
        out = (torch.empty((nq,), dtype=torch.float32, device=dev), torch.empty((nq,), dtype=torch.float32, device=dev))
        sides = {
            "log_partition": lambda: ix.log_partition(q, temperature=1.0 / beta, out=out),
            "search": lambda: ix.search(q, 100),
            "torch": lambda: torch_log_z(q16, x, beta, args.chunk),
        }
        diff = (sides["log_partition"]().log_z.double() - sides["torch"]().double()).abs().max().item()
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
        lp, th = r["log_partition"], r["torch"]
        spread = max(lp["max_ms"] - lp["min_ms"], th["max_ms"] - th["min_ms"])
        flop = 2.0 * nq * args.rows * DIM
        r.update({
            "nq": nq, "inner": inner, "flop": flop, "mfma_frac_of_2.5PF": flop / (lp["median_ms"] * 1e-3) / MFMA_PEAK,
            "tflops": flop / (lp["median_ms"] * 1e-3) / 1e12,
            "ratio_to_search": lp["median_ms"] / r["search"]["median_ms"],
            "speedup_vs_torch": th["median_ms"] / lp["median_ms"],
            "spread_ms": spread, "max_abs_diff_vs_torch": diff,
            "verdict": "faster than torch by more than the spread" if lp["median_ms"] + spread < th["median_ms"] else "NOT faster than torch",
        })
        result["shapes"][f"nq{nq}"] = r
        print(f"nq {nq}: log_partition {lp['median_ms']:.3f} ms [{lp['min_ms']:.3f}, {lp['max_ms']:.3f}] ({r['tflops']:.0f} TFLOP/s, "
              f"{100 * r['mfma_frac_of_2.5PF']:.1f} % of peak)  search {r['search']['median_ms']:.3f} ms  "
              f"torch {th['median_ms']:.3f} ms [{th['min_ms']:.3f}, {th['max_ms']:.3f}]  x{r['ratio_to_search']:.2f} of search  "
              f"{r['speedup_vs_torch']:.2f} x torch  |diff| {diff:.2e}  {r['verdict']}", flush=True)
    # context for the ratio to `search`: the same calls over a store of the same rows at dim 64, where the K loop is ONE slice - the
    # grid, the epilogue (exponentials, reductions, partials) and the finish are those of the dim-768 call, so this time bounds their
    # share of it from above
    del x
    ix.close()
    with HipFlatIndex(64, args.rows, dtype=torch.float16, device=0) as thin:
        for lo in range(0, args.rows, 250_000):
            thin.add(torch.randn((min(250_000, args.rows - lo), 64), generator=g, device=dev).half())
        result["one_slice_dim64"] = {}
        for nq in BATCHES:
            q = torch.randn((nq, 64), generator=g, device=dev)
            fn = lambda: thin.log_partition(q, temperature=8.0)  # noqa: E731
            for _ in range(args.warmup):
                fn()
            inner = max(1, int(0.3 * args.window * 1e3 / max(device_ms(fn, 3), 1e-3)) + 1)
            result["one_slice_dim64"][f"nq{nq}"] = summary([device_ms(fn, inner) for _ in range(args.repeats)])
        print("one-slice store (dim 64):", json.dumps(result["one_slice_dim64"]), flush=True)

    # measured error of the two words against float64 (torch, same device) on the Gaussian shapes of tests/test_log_partition_gpu.py;
    # the derived bound they sit under is tests/partition_ref.py::device_bound
    result["accuracy"] = {}
    for dim in (768, 765):
        for dt in (torch.float16, torch.bfloat16):
            xa = torch.randn((3000, dim), generator=g, device=dev)
            qa = torch.randn((129, dim), generator=g, device=dev)
            b = float(torch.tensor(dim ** -0.5, dtype=torch.float32))
            with HipFlatIndex(dim, 3000, dtype=dt, device=0) as small:
                small.add(xa)
                got = small.log_partition(qa, temperature=1.0 / b)
            s64 = qa.to(dt).double() @ xa.to(dt).double().T
            m64 = s64.max(dim=1).values
            r64 = torch.logsumexp(b * (s64 - m64[:, None]), dim=1)
            result["accuracy"][f"gauss_3000x{dim}_{str(dt).split('.')[-1]}"] = {
                "beta": b, "max_abs_err_log_rel": (got.log_rel.double() - r64).abs().max().item(),
                "max_abs_err_max_score": (got.max_score.double() - m64).abs().max().item()}
    print(json.dumps(result["accuracy"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
