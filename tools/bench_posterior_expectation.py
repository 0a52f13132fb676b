#!/usr/bin/env python3
"""What does the exact softmax read-out of a value table cost?  `HipFlatIndex.posterior_expectation` over a 1 M x 768 fp16 store at nq 256
and 1024 with value tables of 1, 64 and 256 columns, in one process on one device, alternating inside every repeat with three yardsticks:
  log_partition   the scalar call of the same batch: the read-out's scan is that scan plus the second product (the criterion: below
                  2 x log_partition by more than the spread - 2 x is what a two-scan arrangement would cost);
  posterior_mean  the two-scan vector call (768 columns);
  torch           THE YARDSTICK a user would write today, one pass over chunks of the stored rows with a running maximum:
                  `s = beta * q16 @ x_chunk.T`, `m' = max(m, max s)`, `p = exp(s - m')`, `l = l exp(m - m') + sum p`,
                  `acc = acc exp(m - m') + p @ v_chunk`, and `acc / l` at the end - it materialises an nq x chunk block per chunk.
Timing as tools/bench_posterior_mean.py: every side warmed at every shape, a repeat is device milliseconds between two events around
`inner` back-to-back calls, medians with the minimum and maximum over the repeats.  CALL times on the current stream, not kernel times.
Reported per shape: the times, the multiple of log_partition's time next to the cost model's prediction (DESIGN.md 4 "Posterior
read-out": 1 + n_slices / (dim_pad / 64) K-loop equivalents against 1), the ratio to torch, the largest |values - torch's| and the two
verdicts.  Then the measured error maxima against float64 on the Gaussian shapes of tests/test_posterior_expectation_gpu.py, as a
share of the derived bound (tests/readout_ref.py::device_bound).
usage: python tools/bench_posterior_expectation.py [--out profiles/posterior_expectation.json] [--rows 1000000] [--batches 256,1024]
       [--cols 1,64,256] [--no-yardsticks]   (the last three: the short runs behind the choice of VODHIP_READOUT_GROUP_ROWS)"""
import argparse
import json
import pathlib
import re
import statistics
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from vod_amd.index import HipFlatIndex  # noqa: E402

dev = torch.device("cuda", 0)
DIM = 768


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


def torch_readout(q16, x, v, beta, chunk):
    nq = q16.shape[0]
    m = torch.full((nq,), -float("inf"), dtype=torch.float32, device=x.device)
    l = torch.zeros((nq,), dtype=torch.float32, device=x.device)
    acc = torch.zeros((nq, v.shape[1]), dtype=torch.float32, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        s = beta * (q16 @ x[lo : lo + chunk].T).float()
        m_new = torch.maximum(m, s.max(dim=1).values)
        p = torch.exp(s - m_new[:, None])
        scale = torch.exp(m - m_new)
        l = l * scale + p.sum(dim=1)
        acc = acc * scale[:, None] + (p.to(x.dtype) @ v[lo : lo + chunk]).float()
        m = m_new
    return acc / l[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/posterior_expectation.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--cols", default="1,64,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    ap.add_argument("--no-yardsticks", action="store_true", help="time the read-out and log_partition alone, skip the accuracy part")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_expectation.py needs the GPU: there is no CPU path to time")
    batches = [int(b) for b in args.batches.split(",")]
    widths = [int(c) for c in args.cols.split(",")]
    group_rows = int(re.search(r"#define VODHIP_READOUT_GROUP_ROWS (\d+)", (ROOT / "include" / "vodhip.h").read_text()).group(1))

    g = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "window_s": args.window, "torch_chunk_rows": args.chunk, "header_group_rows": group_rows, "shapes": {}}
    with HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0) as ix:
        for lo in range(0, args.rows, 250_000):
            ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=g, device=dev).half())
        x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
        tables = {w: torch.randn((args.rows, w), generator=g, device=dev).half() for w in widths}
        beta = float(torch.tensor(DIM ** -0.5, dtype=torch.float32))
        for nq in batches:
            q = torch.randn((nq, DIM), generator=g, device=dev)
            q16 = q.half()
            out = tuple(torch.empty((nq,), dtype=torch.float32, device=dev) for _ in range(2))
            out_pm = out + (torch.empty((nq, DIM), dtype=torch.float32, device=dev),)
            out_pe = {w: out + (torch.empty((nq, w), dtype=torch.float32, device=dev),) for w in widths}

            def readout(w):
                def run():
                    if ix.row_values_shape != (args.rows, w):  # (outside the timed windows: a width is warmed and timed in one piece)
                        ix.set_row_values(tables[w])
                    return ix.posterior_expectation(q, temperature=1.0 / beta, out=out_pe[w])
                return run

            sides = {"log_partition": lambda: ix.log_partition(q, temperature=1.0 / beta, out=out)}
            if not args.no_yardsticks:
                sides["posterior_mean"] = lambda: ix.posterior_mean(q, temperature=1.0 / beta, out=out_pm)
            for w in widths:
                sides[f"posterior_expectation_{w}"] = readout(w)
                if not args.no_yardsticks:
                    sides[f"torch_{w}"] = (lambda w: lambda: torch_readout(q16, x, tables[w], beta, args.chunk))(w)
            diff = {}
            if not args.no_yardsticks:
                for w in widths:
                    diff[w] = (sides[f"posterior_expectation_{w}"]().values.double() - sides[f"torch_{w}"]().double()).abs().max().item()
            inner = {}
            for name, fn in sides.items():
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                inner[name] = max(1, int(args.window * 1e3 / max(device_ms(fn, 2), 1e-3)) + 1)
            ms = {name: [] for name in sides}
            for _ in range(args.repeats):
                for name, fn in sides.items():  # alternating: every repeat times every side once
                    fn()  # (a read-out of another width sets its table here, outside the window)
                    torch.cuda.synchronize()
                    ms[name].append(device_ms(fn, inner[name]))
            r = {name: summary(v) for name, v in ms.items()}
            lp = r["log_partition"]
            for w in widths:
                pe = r[f"posterior_expectation_{w}"]
                n_slices = (w + 63) // 64
                model = 1.0 + n_slices / (DIM // 64)
                spread = max(pe["max_ms"] - pe["min_ms"], lp["max_ms"] - lp["min_ms"])
                shape = {"nq": nq, "n_cols": w, "beta": beta, "posterior_expectation": pe, "log_partition": lp,
                         "multiple_of_log_partition": pe["median_ms"] / lp["median_ms"], "cost_model_multiple": model, "spread_ms": spread,
                         "verdict_two_scans": "below 2 x log_partition by more than the spread"
                         if pe["median_ms"] + spread < 2 * lp["median_ms"] else "NOT below 2 x log_partition",
                         "useful_tflops": 2.0 * nq * args.rows * (DIM + w) / (pe["median_ms"] * 1e-3) / 1e12,
                         "inner": {k: inner[k] for k in ("log_partition", f"posterior_expectation_{w}")}}
                line = (f"nq {nq} cols {w}: posterior_expectation {pe['median_ms']:.3f} ms [{pe['min_ms']:.3f}, {pe['max_ms']:.3f}]  log_partition "
                        f"{lp['median_ms']:.3f} ms [{lp['min_ms']:.3f}, {lp['max_ms']:.3f}]  x{shape['multiple_of_log_partition']:.2f} (model x{model:.2f})")
                if not args.no_yardsticks:
                    th, pm = r[f"torch_{w}"], r["posterior_mean"]
                    spread_t = max(pe["max_ms"] - pe["min_ms"], th["max_ms"] - th["min_ms"])
                    shape.update({"torch": th, "posterior_mean": pm, "speedup_vs_torch": th["median_ms"] / pe["median_ms"],
                                  "speedup_vs_posterior_mean": pm["median_ms"] / pe["median_ms"], "max_abs_diff_vs_torch": diff[w],
                                  "verdict_torch": "faster than torch by more than the spread"
                                  if pe["median_ms"] + spread_t < th["median_ms"] else "NOT faster than torch"})
                    line += (f"  posterior_mean {pm['median_ms']:.3f} ms  torch {th['median_ms']:.3f} ms [{th['min_ms']:.3f}, {th['max_ms']:.3f}]  "
                             f"{shape['speedup_vs_torch']:.2f} x torch  |diff| {diff[w]:.2e}  {shape['verdict_torch']}")
                result["shapes"][f"nq{nq}_cols{w}"] = shape
                print(line + f"  {shape['verdict_two_scans']}", flush=True)
        del x

    if not args.no_yardsticks:
        # measured error against float64 on the Gaussian shapes of tests/test_posterior_expectation_gpu.py, and its share of the derived bound
        import readout_ref as R  # noqa: E402  (tests/)
        from test_l2_cpu import GAUSS_CASES, gauss_case  # noqa: E402

        result["accuracy"] = {}
        for dim, dtype, seed in GAUSS_CASES:
            qa, xa = gauss_case(dim, seed)
            va = np.random.default_rng(seed).standard_normal((len(xa), 100)).astype(np.float32)
            b = float(np.float32(1.0 / np.sqrt(dim)))
            with HipFlatIndex(dim, len(xa), dtype=getattr(torch, dtype), device=0) as small:
                small.add(xa)
                small.set_row_values(va)
                got = small.posterior_expectation(torch.from_numpy(qa).to(dev), temperature=1.0 / b).values.cpu().numpy().astype(np.float64)
            ref, _, _ = R.posterior_expectation(qa, xa, va, dtype, b)
            bound = R.device_bound(qa, xa, va, dtype, b, dot=True)
            err = np.abs(got - ref)
            result["accuracy"][f"gauss_{len(xa)}x{dim}_{dtype}_cols100"] = {"beta": b, "max_abs_err": float(err.max()),
                                                                           "max_err_over_bound": float((err / bound).max())}
        print(json.dumps(result["accuracy"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
