#!/usr/bin/env python3
"""What does the read-out's gradient in the query cost?  `HipFlatIndex.posterior_expectation_backward` over a 1 M x 768 fp16 store at nq
256 and 1024 with value tables of 1, 64 and 256 columns, in one process on one device, alternating inside every repeat with:
  posterior_mean         the two-scan vector call of the same batch (the cost model's yardstick: DESIGN.md 4 "Read-out gradient");
  posterior_expectation  the forward of the same batch and width;
  torch                  the chunked sequence that does the same job with the forward's log Z given, per chunk of the stored rows:
                         `p = exp(beta q16 @ x_c.T - log_z)`, `w = p * (g @ v_c.T - ubar)`, `grad += w @ x_c` - an nq x chunk block per chunk,
                         the matrix products in fp16 with g and ubar scaled by 2^10 / max |g| first (unscaled, w ~ 1e-9 flushes in fp16
                         and the sequence returns noise: the scale costs the yardstick nothing);
  full step              `expected_values(q).backward(g)` against torch autograd through the chunked running-maximum forward of
                         tools/bench_posterior_expectation.py.
Timing as tools/bench_posterior_expectation.py: every side warmed at every shape, a repeat is device milliseconds between two events
around `inner` back-to-back calls, medians with the minimum and maximum over the repeats.  CALL times on the current stream.
Reported per shape: the times, the ratio to posterior_mean next to the cost model's prediction, the ratio to torch, the largest
|grad - torch's| and the verdicts.  Then the measured error maxima against float64 on the Gaussian shapes of
tests/test_expected_values_gpu.py as a share of the derived bound (tests/readout_grad_ref.py::device_bound), and - with --remarks, the
output of `hipcc -Rpass-analysis=kernel-resource-usage` on kernels_readout_grad.hip - the registers and scratch of every instantiation.
usage: python tools/bench_expected_values.py [--out profiles/expected_values.json] [--rows 1000000] [--batches 256,1024] [--cols 1,64,256]
       [--remarks FILE[,FILE4]]"""
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
sys.path.insert(0, str(ROOT / "tools"))
from bench_posterior_expectation import device_ms, summary, torch_readout  # noqa: E402
from vod_amd.index import HipFlatIndex  # noqa: E402

dev = torch.device("cuda", 0)
DIM = 768


def torch_backward(q16, x, v, g16, ubar, log_z, beta, chunk, scale):
    """g16 and ubar already multiplied by `scale`"""
    grad = torch.zeros((q16.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        xc = x[lo : lo + chunk]
        p = torch.exp(beta * (q16 @ xc.T).float() - log_z[:, None])
        w = p * ((g16 @ v[lo : lo + chunk].T).float() - ubar[:, None])
        grad += (w.to(x.dtype) @ xc).float()
    return (beta / scale) * grad


def parse_remarks(path):
    """{instantiation: {vgprs, agprs, scratch_bytes}} of the scan kernel from a kernel-resource-usage remark log"""
    out, name = {}, None
    for line in pathlib.Path(path).read_text().splitlines():
        m = re.search(r"Function Name: \S*readout_grad_scan_kernelILi(\d)ELb(\d)ELi(\d)E", line)
        if "Function Name:" in line:
            name = f"dt{m.group(1)}_subset{m.group(2)}_slices{m.group(3)}" if m else None
            if name:
                out[name] = {}
        elif name:
            for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch_bytes", r"ScratchSize \[bytes/lane\]: (\d+)")):
                m2 = re.search(pat, line)
                if m2:
                    out[name][key] = int(m2.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/expected_values.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--cols", default="1,64,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequences")
    ap.add_argument("--remarks", default="", help="resource-usage remark logs: the build in use[, the 4-slice build]")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_expected_values.py needs the GPU: there is no CPU path to time")
    batches = [int(b) for b in args.batches.split(",")]
    widths = [int(c) for c in args.cols.split(",")]

    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "window_s": args.window, "torch_chunk_rows": args.chunk, "chunk_slices": 3, "shapes": {}}
    if args.remarks:
        logs = args.remarks.split(",")
        result["registers"] = {"in_use_3_slices": parse_remarks(logs[0])}
        if len(logs) > 1:
            result["registers"]["rejected_4_slices"] = parse_remarks(logs[1])
    with HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0) as ix:
        for lo in range(0, args.rows, 250_000):
            ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=gen, device=dev).half())
        x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
        tables = {w: torch.randn((args.rows, w), generator=gen, device=dev).half() for w in widths}
        beta = float(torch.tensor(DIM ** -0.5, dtype=torch.float32))
        for nq in batches:
            q = torch.randn((nq, DIM), generator=gen, device=dev)
            q16 = q.half()
            out_pm = tuple(torch.empty((nq,), dtype=torch.float32, device=dev) for _ in range(2)) + (torch.empty((nq, DIM), dtype=torch.float32, device=dev),)
            out_grad = torch.empty((nq, DIM), dtype=torch.float32, device=dev)
            gs = {w: torch.randn((nq, w), generator=gen, device=dev) * 1e-3 for w in widths}
            fwd = {}

            def table(w):
                if ix.row_values_shape != (args.rows, w):  # (outside the timed windows: a width is warmed and timed in one piece)
                    ix.set_row_values(tables[w])

            for w in widths:
                table(w)
                fwd[w] = ix.posterior_expectation(q, temperature=1.0 / beta)
            t_scale = {w: float(2.0 ** 10 / gs[w].abs().max()) for w in widths}
            g16 = {w: (gs[w] * t_scale[w]).half() for w in widths}
            ubar = {w: (g16[w].float() * fwd[w].values).sum(dim=1) for w in widths}

            def forward(w):
                def run():
                    table(w)
                    return ix.posterior_expectation(q, temperature=1.0 / beta)
                return run

            def backward(w):
                def run():
                    table(w)
                    return ix.posterior_expectation_backward(q, gs[w], fwd[w], temperature=1.0 / beta, out=out_grad)
                return run

            def full_step(w):
                def run():
                    table(w)
                    qq = q.detach().requires_grad_(True)
                    ix.expected_values(qq, temperature=1.0 / beta).backward(gs[w])
                    return qq.grad
                return run

            def torch_full(w):
                def run():
                    qq = q16.detach().requires_grad_(True)
                    torch_readout(qq, x, tables[w], beta, args.chunk).backward(gs[w])
                    return qq.grad
                return run

            sides = {"posterior_mean": lambda: ix.posterior_mean(q, temperature=1.0 / beta, out=out_pm)}
            for w in widths:
                sides[f"posterior_expectation_{w}"] = forward(w)
                sides[f"backward_{w}"] = backward(w)
                sides[f"torch_backward_{w}"] = (lambda w: lambda: torch_backward(q16, x, tables[w], g16[w], ubar[w], fwd[w].log_partition.log_z, beta,
                                                                                 args.chunk, t_scale[w]))(w)
                sides[f"full_step_{w}"] = full_step(w)
                sides[f"torch_full_step_{w}"] = torch_full(w)
            diff = {w: (sides[f"backward_{w}"]().double() - sides[f"torch_backward_{w}"]().double()).abs().max().item() for w in widths}
            scale = {w: sides[f"backward_{w}"]().abs().max().item() for w in widths}
            inner = {}
            for name, fn in sides.items():
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                inner[name] = max(1, int(args.window * 1e3 / max(device_ms(fn, 2), 1e-3)) + 1)
            ms = {name: [] for name in sides}
            for _ in range(args.repeats):
                for name, fn in sides.items():  # alternating: every repeat times every side once
                    fn()  # (a call of another width sets its table here, outside the window)
                    torch.cuda.synchronize()
                    ms[name].append(device_ms(fn, inner[name]))
            r = {name: summary(v) for name, v in ms.items()}
            pm = r["posterior_mean"]
            for w in widths:
                bw, pe, th, fs, tf = (r[f"{k}_{w}"] for k in ("backward", "posterior_expectation", "torch_backward", "full_step", "torch_full_step"))
                c_slices = (w + 63) // 64
                # per tile and 64 queries: dim_pad / 64 + c_pad / 64 K-loop steps + the chunk's slices, once per chunk of 3 slices, against
                # posterior_mean's (dim_pad / 64 + 4) per chunk of 4 slices + its partition scan (DESIGN.md 4 "Read-out gradient")
                steps = DIM // 64
                model = ((steps // 3) * (steps + c_slices + 3)) / ((steps // 4) * (steps + 4) + steps)
                spread_pm = max(bw["max_ms"] - bw["min_ms"], pm["max_ms"] - pm["min_ms"])
                spread_t = max(bw["max_ms"] - bw["min_ms"], th["max_ms"] - th["min_ms"])
                ratio = bw["median_ms"] / pm["median_ms"]
                shape = {"nq": nq, "n_cols": w, "beta": beta, "backward": bw, "posterior_mean": pm, "posterior_expectation": pe, "torch_backward": th,
                         "full_step": fs, "torch_full_step": tf, "ratio_to_posterior_mean": ratio, "cost_model_ratio_3_slices": model,
                         "model_ratio_4_slices": 0.85 if w == 64 else (1.0 if w == 256 else None),
                         "spread_vs_posterior_mean_ms": spread_pm, "speedup_vs_torch": th["median_ms"] / bw["median_ms"],
                         "full_step_speedup_vs_torch": tf["median_ms"] / fs["median_ms"], "max_abs_diff_vs_torch": diff[w], "max_abs_grad": scale[w],
                         "verdict_torch": "faster than torch by more than the spread" if bw["median_ms"] + spread_t < th["median_ms"] else "NOT faster than torch",
                         "verdict_model": "within the spread of the 3-slice model's ratio to posterior_mean"
                         if bw["median_ms"] - spread_pm <= model * pm["median_ms"] else "ABOVE the 3-slice model's ratio to posterior_mean by more than the spread",
                         "useful_tflops": 2.0 * nq * args.rows * (2 * DIM + w) / (bw["median_ms"] * 1e-3) / 1e12,
                         "inner": {k: inner[k] for k in (f"backward_{w}", f"torch_backward_{w}", f"full_step_{w}", f"torch_full_step_{w}", "posterior_mean")}}
                result["shapes"][f"nq{nq}_cols{w}"] = shape
                print(f"nq {nq} cols {w}: backward {bw['median_ms']:.3f} ms [{bw['min_ms']:.3f}, {bw['max_ms']:.3f}]  posterior_mean {pm['median_ms']:.3f} ms "
                      f"[{pm['min_ms']:.3f}, {pm['max_ms']:.3f}]  x{ratio:.2f} (3-slice model x{model:.2f})  forward {pe['median_ms']:.3f} ms  torch "
                      f"{th['median_ms']:.3f} ms [{th['min_ms']:.3f}, {th['max_ms']:.3f}]  {shape['speedup_vs_torch']:.2f} x torch  |diff| {diff[w]:.2e} of "
                      f"{scale[w]:.2e}  full step {fs['median_ms']:.3f} ms vs torch autograd {tf['median_ms']:.3f} ms  {shape['verdict_torch']}; "
                      f"{shape['verdict_model']}", flush=True)
        del x

    # measured error against float64 on the Gaussian shapes of tests/test_expected_values_gpu.py, and its share of the derived bound
    import readout_grad_ref as G  # noqa: E402  (tests/)
    from test_l2_cpu import GAUSS_CASES, gauss_case  # noqa: E402

    result["accuracy"] = {}
    for dim, dtype, seed in GAUSS_CASES:
        qa, xa = gauss_case(dim, seed)
        rng = np.random.default_rng(seed)
        va = rng.standard_normal((len(xa), 100)).astype(np.float32)
        ga = rng.standard_normal((len(qa), 100)).astype(np.float32)
        b = float(np.float32(1.0 / np.sqrt(dim)))
        with HipFlatIndex(dim, len(xa), dtype=getattr(torch, dtype), device=0) as small:
            small.add(xa)
            small.set_row_values(va)
            qd = torch.from_numpy(qa).to(dev)
            pe = small.posterior_expectation(qd, temperature=1.0 / b)
            got = small.posterior_expectation_backward(qd, torch.from_numpy(ga).to(dev), pe, temperature=1.0 / b).cpu().numpy().astype(np.float64)
        ref = G.expected_values_grad(qa, xa, va, ga, dtype, b)[0]
        bound = G.device_bound(qa, xa, va, ga, dtype, b, dot=True)
        err = np.abs(got - ref)
        result["accuracy"][f"gauss_{len(xa)}x{dim}_{dtype}_cols100"] = {"beta": b, "max_abs_err": float(err.max()), "max_abs_grad": float(np.abs(ref).max()),
                                                                       "max_err_over_bound": float((err / bound).max())}
    print(json.dumps(result["accuracy"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
