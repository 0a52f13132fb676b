#!/usr/bin/env python3
"""What does the posterior's gradient in the stored rows cost?  `HipFlatIndex.key_gradient` over a 1 M x 768 fp16 store at nq 256 and
1024, in one process on one device, alternating inside every repeat:
  log Z only             `key_gradient(q, grad_log_z=a)` against THREE `posterior_adjoint` calls of 256 columns with W = a q (the only
                         way to the log Z term before; the cost model says about 1.0 x: the same K loops and slices, one staging
                         instead of three - DESIGN.md 4 "Key gradient");
  with a table           `key_gradient(q, grad_log_z=a, grad_values=G)` at 64 and 256 table columns against the log Z-only call: the
                         cost model is (K + c_pad / 64 + slices) / (K + slices) per chunk with 3-slice chunks against 4-slice ones;
  torch                  the chunked sequence that does the same job with the forward given, per chunk of the stored rows:
                         `p = exp(beta q16 @ x_c.T - log_z)`, `c = a + g16 @ v_c.T - ubar`, `out[chunk] = beta (p c).T @ q16` - the
                         products in fp16 with the gradients scaled to about 1 first (what the call does itself);
  full step              `read_out(q, V, keys=K).sum().backward()` (gradients in q, V AND the rows; the table is set in the step)
                         against torch autograd through the chunked running-maximum forward of tools/bench_posterior_expectation.py
                         with q, V and the rows as leaves.
Timing as tools/bench_posterior_adjoint.py: every side warmed at every shape, a repeat is device milliseconds between two events
around `inner` back-to-back calls, medians with the minimum and maximum over the repeats (the run-to-run spread).  CALL times on the
current stream.  NOT measured here: kernel times, bf16 stores, 10 M rows, the node index.
usage: python tools/bench_key_gradient.py [--out profiles/key_gradient.json] [--rows 1000000] [--batches 256,1024] [--cols 64,256]"""
import argparse
import json
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from bench_posterior_expectation import device_ms, summary, torch_readout  # noqa: E402
from vod_amd.index import HipFlatIndex  # noqa: E402

dev = torch.device("cuda", 0)
DIM = 768


def torch_key_gradient(q16, x, v, a_s, g16, ubar_s, scale, log_z, beta, chunk):
    """a_s, g16, ubar_s: the gradients (and ubar) divided by `scale`; the result is multiplied back"""
    out = torch.empty((x.shape[0], x.shape[1]), dtype=torch.float32, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        p = torch.exp(beta * (q16 @ x[lo : lo + chunk].T).float() - log_z[:, None])
        c = a_s[:, None] if g16 is None else a_s[:, None] + ((g16 @ v[lo : lo + chunk].T).float() - ubar_s[:, None])
        out[lo : lo + chunk] = ((p * c).to(x.dtype).T @ q16).float()
    return out * (beta * scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/key_gradient.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batches", default="256,1024")
    ap.add_argument("--cols", default="64,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.15, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequences")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_key_gradient.py needs the GPU: there is no CPU path to time")
    batches = [int(b) for b in args.batches.split(",")]
    widths = [int(c) for c in args.cols.split(",")]

    gen = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "window_s": args.window, "torch_chunk_rows": args.chunk,
              "not_measured": ["kernel times", "bf16 stores", "10 M rows", "the node index"], "shapes": {}}
    K = DIM // 64
    with HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0) as ix:
        for lo in range(0, args.rows, 250_000):
            ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=gen, device=dev).half())
        x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
        tables = {w: torch.randn((args.rows, w), generator=gen, device=dev).half() for w in widths}
        beta = float(torch.tensor(DIM ** -0.5, dtype=torch.float32))
        out = torch.empty((args.rows, DIM), dtype=torch.float32, device=dev)
        adj_out = [torch.empty((args.rows, 256), dtype=torch.float32, device=dev) for _ in range(3)]
        for nq in batches:
            q = torch.randn((nq, DIM), generator=gen, device=dev)
            q16 = q.half()
            a = torch.randn((nq,), generator=gen, device=dev) * 1e-3
            gs = {w: torch.randn((nq, w), generator=gen, device=dev) * 1e-3 for w in widths}
            lp = ix.log_partition(q, temperature=1.0 / beta)
            w_adj = [(a[:, None] * q16.float())[:, lo : lo + 256].contiguous() for lo in range(0, DIM, 256)]
            pes = {}
            for w in widths:
                ix.set_row_values(tables[w])
                pes[w] = ix.posterior_expectation(q, temperature=1.0 / beta)
            scale = {w: max(a.abs().max().item(), gs[w].abs().max().item()) for w in widths}
            scale[0] = a.abs().max().item()

            def table(w):
                if ix.row_values_shape != (args.rows, w):  # (outside the timed windows: a width is warmed and timed in one piece)
                    ix.set_row_values(tables[w])

            def with_table(w):
                def run():
                    table(w)
                    return ix.key_gradient(q, grad_log_z=a, grad_values=gs[w], expectation=pes[w], temperature=1.0 / beta, out=out)
                return run

            def three_adjoints():
                for i in range(3):
                    ix.posterior_adjoint(q, w_adj[i], lp, temperature=1.0 / beta, out=adj_out[i])
                return adj_out

            def torch_side(w):
                if w == 0:
                    return lambda: torch_key_gradient(q16, x, None, a / scale[0], None, None, scale[0], lp.log_z, beta, args.chunk)
                g16 = (gs[w] / scale[w]).half()
                ubar = (g16.float() * pes[w].values).sum(dim=1)
                return lambda: torch_key_gradient(q16, x, tables[w], a / scale[w], g16, ubar, scale[w], lp.log_z, beta, args.chunk)

            def full_step(w):
                def run():
                    qq = q.detach().requires_grad_(True)
                    vv = tables[w].detach().requires_grad_(True)
                    kk = x.detach().requires_grad_(True)
                    ix.read_out(qq, vv, temperature=1.0 / beta, keys=kk).sum().backward()
                    return kk.grad
                return run

            def torch_full(w):
                def run():
                    qq = q16.detach().requires_grad_(True)
                    vv = tables[w].detach().requires_grad_(True)
                    kk = x.detach().requires_grad_(True)
                    torch_readout(qq, kk, vv, beta, args.chunk).sum().backward()
                    return kk.grad
                return run

            sides = {"log_z_only": lambda: ix.key_gradient(q, grad_log_z=a, log_partition=lp, temperature=1.0 / beta, out=out),
                     "three_adjoints": three_adjoints, "torch_log_z_only": torch_side(0)}
            for w in widths:
                sides[f"table_{w}"] = with_table(w)
                sides[f"torch_table_{w}"] = torch_side(w)
                sides[f"full_step_{w}"] = full_step(w)
                sides[f"torch_full_step_{w}"] = torch_full(w)
            diff = {0: (sides["log_z_only"]().double() - sides["torch_log_z_only"]().double()).abs().max().item()}
            top = {0: sides["log_z_only"]().abs().max().item()}
            for w in widths:
                diff[w] = (sides[f"table_{w}"]().double() - sides[f"torch_table_{w}"]().double()).abs().max().item()
                top[w] = sides[f"table_{w}"]().abs().max().item()
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
            spread = lambda *names: max(r[n]["max_ms"] - r[n]["min_ms"] for n in names)  # noqa: E731
            lz, ta, tz = r["log_z_only"], r["three_adjoints"], r["torch_log_z_only"]
            shape = {"nq": nq, "beta": beta, "log_z_only": lz, "three_adjoints": ta, "torch_log_z_only": tz,
                     "ratio_to_three_adjoints": lz["median_ms"] / ta["median_ms"], "cost_model_ratio_to_three_adjoints": 1.0,
                     "spread_vs_three_adjoints_ms": spread("log_z_only", "three_adjoints"),
                     "spread_vs_three_adjoints_ratio": spread("log_z_only", "three_adjoints") / ta["median_ms"],
                     "speedup_vs_torch": tz["median_ms"] / lz["median_ms"], "max_abs_diff_vs_torch": diff[0], "max_abs_out": top[0],
                     "verdict_torch": "faster than torch by more than the spread" if lz["median_ms"] + spread("log_z_only", "torch_log_z_only") < tz["median_ms"] else "NOT faster than torch",
                     "inner": inner, "tables": {}}
            print(f"nq {nq} log Z only: {lz['median_ms']:.3f} ms [{lz['min_ms']:.3f}, {lz['max_ms']:.3f}]  three adjoints {ta['median_ms']:.3f} ms "
                  f"[{ta['min_ms']:.3f}, {ta['max_ms']:.3f}]  x{shape['ratio_to_three_adjoints']:.2f} (model x1.00, spread {shape['spread_vs_three_adjoints_ratio']:.3f})  "
                  f"torch {tz['median_ms']:.3f} ms [{tz['min_ms']:.3f}, {tz['max_ms']:.3f}]  {shape['speedup_vs_torch']:.2f} x torch  |diff| {diff[0]:.2e} of {top[0]:.2e}  "
                  f"{shape['verdict_torch']}", flush=True)
            for w in widths:
                c_pad = (w + 63) // 64 * 64
                # per row tile and query tile: chunks * (K-loop steps + second-product slices)
                model = (K // 3) * (K + c_pad // 64 + 3) / ((K // 4) * (K + 4))
                tb, tt, fs, tf = r[f"table_{w}"], r[f"torch_table_{w}"], r[f"full_step_{w}"], r[f"torch_full_step_{w}"]
                sp = spread(f"table_{w}", f"torch_table_{w}")
                shape["tables"][str(w)] = {
                    "n_cols": w, "key_gradient": tb, "torch": tt, "full_step": fs, "torch_full_step": tf,
                    "ratio_to_log_z_only": tb["median_ms"] / lz["median_ms"], "cost_model_ratio_to_log_z_only": model,
                    "spread_vs_log_z_only_ms": spread(f"table_{w}", "log_z_only"), "speedup_vs_torch": tt["median_ms"] / tb["median_ms"],
                    "full_step_speedup_vs_torch": tf["median_ms"] / fs["median_ms"], "max_abs_diff_vs_torch": diff[w], "max_abs_out": top[w],
                    "verdict_torch": "faster than torch by more than the spread" if tb["median_ms"] + sp < tt["median_ms"] else "NOT faster than torch",
                    "verdict_full_step": "faster than torch autograd by more than the spread"
                    if fs["median_ms"] + spread(f"full_step_{w}", f"torch_full_step_{w}") < tf["median_ms"] else "NOT faster than torch autograd"}
                t = shape["tables"][str(w)]
                print(f"nq {nq} table {w}: {tb['median_ms']:.3f} ms [{tb['min_ms']:.3f}, {tb['max_ms']:.3f}]  x{t['ratio_to_log_z_only']:.2f} log Z only (model "
                      f"x{model:.2f})  torch {tt['median_ms']:.3f} ms [{tt['min_ms']:.3f}, {tt['max_ms']:.3f}]  {t['speedup_vs_torch']:.2f} x torch  |diff| "
                      f"{diff[w]:.2e} of {top[w]:.2e}  full step {fs['median_ms']:.3f} ms [{fs['min_ms']:.3f}, {fs['max_ms']:.3f}] vs torch autograd "
                      f"{tf['median_ms']:.3f} ms [{tf['min_ms']:.3f}, {tf['max_ms']:.3f}]  {t['verdict_torch']}; {t['verdict_full_step']}", flush=True)
            result["shapes"][f"nq{nq}"] = shape
        del x
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
