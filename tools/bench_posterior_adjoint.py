#!/usr/bin/env python3
"""What does the read-out's adjoint - its gradient in the value table - cost?  `HipFlatIndex.posterior_adjoint` over a 1 M x 768 fp16
store at nq 256 and 1024 with weights of 1, 64 and 256 columns, in one process on one device, alternating inside every repeat with:
  posterior_expectation  the forward of the same batch and width (the cost model's yardstick: the same K loop and second product, no
                         rescaling, no partials - DESIGN.md 4 "Read-out adjoint" predicts about 1.0 x);
  torch                  the chunked sequence that does the same job with the forward's log Z given, per chunk of the stored rows:
                         `p = exp(beta q16 @ x_c.T - log_z)`, `out[chunk] = p.T @ W` - an nq x chunk block and a transposed GEMM per
                         chunk, the products in fp16 with W scaled per column to about 1 first (what the call does itself);
  full step              `read_out(q, V).sum().backward()` (gradients in q AND V; the table is set in the step) against torch autograd
                         through the chunked running-maximum forward of tools/bench_posterior_expectation.py with q and V as leaves.
Timing as tools/bench_posterior_expectation.py: every side warmed at every shape, a repeat is device milliseconds between two events
around `inner` back-to-back calls, medians with the minimum and maximum over the repeats (the run-to-run spread).  CALL times on the
current stream.  Reported per shape: the times, the ratio to posterior_expectation, the ratio to torch, the largest |out - torch's|.
Then the measured error maxima against float64 on the Gaussian shapes of tests/test_posterior_adjoint_gpu.py as a share of the derived
bound (tests/readout_adjoint_ref.py::device_bound).  NOT measured here: bf16 stores, 10 M rows, the node index.
usage: python tools/bench_posterior_adjoint.py [--out profiles/posterior_adjoint.json] [--rows 1000000] [--batches 256,1024] [--cols 1,64,256]"""
import argparse
import json
import pathlib
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


def torch_adjoint(q16, x, w16, col_scale, log_z, beta, chunk):
    """w16 = (W / col_scale) in fp16; the result is multiplied back"""
    out = torch.empty((x.shape[0], w16.shape[1]), dtype=torch.float32, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        p = torch.exp(beta * (q16 @ x[lo : lo + chunk].T).float() - log_z[:, None])
        out[lo : lo + chunk] = (p.to(x.dtype).T @ w16).float()
    return out * col_scale[None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/posterior_adjoint.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--cols", default="1,64,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequences")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_adjoint.py needs the GPU: there is no CPU path to time")
    batches = [int(b) for b in args.batches.split(",")]
    widths = [int(c) for c in args.cols.split(",")]

    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "window_s": args.window, "torch_chunk_rows": args.chunk, "not_measured": ["bf16 stores", "10 M rows", "the node index"], "shapes": {}}
    with HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0) as ix:
        for lo in range(0, args.rows, 250_000):
            ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=gen, device=dev).half())
        x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
        tables = {w: torch.randn((args.rows, w), generator=gen, device=dev).half() for w in widths}
        beta = float(torch.tensor(DIM ** -0.5, dtype=torch.float32))
        for nq in batches:
            q = torch.randn((nq, DIM), generator=gen, device=dev)
            q16 = q.half()
            ws = {w: torch.randn((nq, w), generator=gen, device=dev) * 1e-3 for w in widths}
            outs = {w: torch.empty((args.rows, w), dtype=torch.float32, device=dev) for w in widths}
            lp = ix.log_partition(q, temperature=1.0 / beta)
            col_scale = {w: ws[w].abs().amax(dim=0).clamp_min(1e-30) for w in widths}
            w16 = {w: (ws[w] / col_scale[w][None, :]).half() for w in widths}

            def table(w):
                if ix.row_values_shape != (args.rows, w):  # (outside the timed windows: a width is warmed and timed in one piece)
                    ix.set_row_values(tables[w])

            def forward(w):
                def run():
                    table(w)
                    return ix.posterior_expectation(q, temperature=1.0 / beta)
                return run

            def adjoint(w):
                return lambda: ix.posterior_adjoint(q, ws[w], lp, temperature=1.0 / beta, out=outs[w])

            def full_step(w):
                def run():
                    qq = q.detach().requires_grad_(True)
                    vv = tables[w].detach().requires_grad_(True)
                    ix.read_out(qq, vv, temperature=1.0 / beta).sum().backward()
                    return vv.grad
                return run

            def torch_full(w):
                def run():
                    qq = q16.detach().requires_grad_(True)
                    vv = tables[w].detach().requires_grad_(True)
                    torch_readout(qq, x, vv, beta, args.chunk).sum().backward()
                    return vv.grad
                return run

            sides = {}
            for w in widths:
                sides[f"posterior_expectation_{w}"] = forward(w)
                sides[f"adjoint_{w}"] = adjoint(w)
                sides[f"torch_adjoint_{w}"] = (lambda w: lambda: torch_adjoint(q16, x, w16[w], col_scale[w], lp.log_z, beta, args.chunk))(w)
                sides[f"full_step_{w}"] = full_step(w)
                sides[f"torch_full_step_{w}"] = torch_full(w)
            diff = {w: (sides[f"adjoint_{w}"]().double() - sides[f"torch_adjoint_{w}"]().double()).abs().max().item() for w in widths}
            scale = {w: sides[f"adjoint_{w}"]().abs().max().item() for w in widths}
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
            for w in widths:
                ad, pe, th, fs, tf = (r[f"{k}_{w}"] for k in ("adjoint", "posterior_expectation", "torch_adjoint", "full_step", "torch_full_step"))
                spread_pe = max(ad["max_ms"] - ad["min_ms"], pe["max_ms"] - pe["min_ms"])
                spread_t = max(ad["max_ms"] - ad["min_ms"], th["max_ms"] - th["min_ms"])
                ratio = ad["median_ms"] / pe["median_ms"]
                shape = {"nq": nq, "n_cols": w, "beta": beta, "adjoint": ad, "posterior_expectation": pe, "torch_adjoint": th, "full_step": fs,
                         "torch_full_step": tf, "ratio_to_posterior_expectation": ratio, "cost_model_ratio": 1.0,
                         "ratio_range": [ad["min_ms"] / pe["max_ms"], ad["max_ms"] / pe["min_ms"]],
                         "spread_vs_posterior_expectation_ms": spread_pe, "speedup_vs_torch": th["median_ms"] / ad["median_ms"],
                         "full_step_speedup_vs_torch": tf["median_ms"] / fs["median_ms"], "max_abs_diff_vs_torch": diff[w], "max_abs_out": scale[w],
                         "verdict_torch": "faster than torch by more than the spread" if ad["median_ms"] + spread_t < th["median_ms"] else "NOT faster than torch",
                         "useful_tflops": 2.0 * nq * args.rows * (DIM + w) / (ad["median_ms"] * 1e-3) / 1e12,
                         "inner": {k: inner[k] for k in (f"adjoint_{w}", f"posterior_expectation_{w}", f"torch_adjoint_{w}", f"full_step_{w}", f"torch_full_step_{w}")}}
                result["shapes"][f"nq{nq}_cols{w}"] = shape
                print(f"nq {nq} cols {w}: adjoint {ad['median_ms']:.3f} ms [{ad['min_ms']:.3f}, {ad['max_ms']:.3f}]  posterior_expectation {pe['median_ms']:.3f} ms "
                      f"[{pe['min_ms']:.3f}, {pe['max_ms']:.3f}]  x{ratio:.2f} (model x1.00)  torch {th['median_ms']:.3f} ms [{th['min_ms']:.3f}, {th['max_ms']:.3f}]  "
                      f"{shape['speedup_vs_torch']:.2f} x torch  |diff| {diff[w]:.2e} of {scale[w]:.2e}  full step {fs['median_ms']:.3f} ms "
                      f"[{fs['min_ms']:.3f}, {fs['max_ms']:.3f}] vs torch autograd {tf['median_ms']:.3f} ms [{tf['min_ms']:.3f}, {tf['max_ms']:.3f}]  "
                      f"{shape['verdict_torch']}", flush=True)
            del outs
        del x

    # measured error against float64 on the Gaussian shapes of tests/test_posterior_adjoint_gpu.py, and its share of the derived bound
    import readout_adjoint_ref as A  # noqa: E402  (tests/)
    from test_l2_cpu import GAUSS_CASES, gauss_case  # noqa: E402

    result["accuracy"] = {}
    for dim, dtype, seed in GAUSS_CASES:
        qa, xa = gauss_case(dim, seed)
        wa = np.random.default_rng(seed).standard_normal((len(qa), 100)).astype(np.float32)
        b = float(np.float32(1.0 / np.sqrt(dim)))
        with HipFlatIndex(dim, len(xa), dtype=getattr(torch, dtype), device=0) as small:
            small.add(xa)
            got = small.posterior_adjoint(torch.from_numpy(qa).to(dev), torch.from_numpy(wa).to(dev), None, temperature=1.0 / b).cpu().numpy().astype(np.float64)
        ref = A.posterior_adjoint(qa, xa, wa, dtype, b)[0]
        bound = A.device_bound(qa, xa, wa, dtype, b, dot=True)
        err = np.abs(got - ref)
        result["accuracy"][f"gauss_{len(xa)}x{dim}_{dtype}_cols100"] = {"beta": b, "max_abs_err": float(err.max()), "max_abs_out": float(np.abs(ref).max()),
                                                                       "max_err_over_bound": float((err / bound).max())}
    print(json.dumps(result["accuracy"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
