#!/usr/bin/env python3
"""What does the pooling head cost?  bf16 hidden states, H = 768, the `mpool-scaled-cosine` config (mean, l2, scaler 100), token
lengths uniform in [L/2, L] (about 25 % padding), on the two sides of a training step:
  sections  2112 x 512 x 768   (64 queries x 32 sections + in-batch extras: 1.66 GB)
  queries     64 x  64 x 768

Times, in one process on one device, alternating the sides inside every repeat (median device milliseconds between two events around
`--inner` back-to-back steps, after `--warmup` untimed steps of each).  These are END-TO-END STEP times of the eager path: the kernels
plus the allocator, autograd and launch gaps between them, not kernel times; the GB/s is a step rate, a lower bound of the kernels' own.
  fused_reference / fused_masked   `vod_amd.pooler.VodPooler` in its two mask modes: forward, and forward + backward
  torch_reference                  a torch restatement of the reference's op sequence (modeling.py:80-82,164-174: mask.sum, x.sum(-2),
                                   the division, masked_fill, F.normalize, log_scaler.mul(0.5).exp(), the product) with torch's autograd
  torch_masked                     the same with `x * mask` in front of the sum (what a user would write to get the masked mean)
Per side: ms with the minimum and maximum over the repeats (the run-to-run spread), the peak of `torch.cuda.max_memory_allocated` above
what the inputs occupy, and GB/s over the bytes the ALGORITHM needs: forward = the token rows read (all N * L in reference mode, the
live ones in masked mode) * H * b + N * H * out bytes; backward = N * L * H * b written + the reads of a and g (N * H * 4 each).  A
torch side is charged the bytes of the fused side it is compared with.
`--poolerr LOG` stores the `POOLERR` lines of a `pytest -s tests/test_pooler_gpu.py` log next to the timings (float32 lines whole,
16-bit lines as the worst share of their bound); a `poolerr` key already in the `--out` file is carried over otherwise.
usage: python tools/bench_pooler.py [--out profiles/pooler.json] [--poolerr LOG]"""
import argparse
import json
import pathlib
import re
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd.pooler import VodPooler  # noqa: E402

STREAM_TBS = 6.29  # measured streaming rate of the MI355X
CONFIG = {"agg_method": "mean", "output_norm": "l2", "scaler": 100.0}
dev = torch.device("cuda", 0)


def reference_ops(x, mask, log_scaler, zero_pads=False):
    """The reference's op sequence, restated in torch (no reference code is imported)."""
    if zero_pads:
        x = x * mask.unsqueeze(-1).to(x.dtype)
    sum_mask = mask.sum(dim=-1, keepdim=True)
    pooled = (x.sum(dim=-2) / sum_mask.to(torch.float32)).masked_fill(sum_mask <= 0, 0.0)
    pooled = torch.nn.functional.normalize(pooled, p=2)
    return pooled * log_scaler.mul(0.5).exp()


def device_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def read_poolerr(path):
    f32, worst16 = [], {}
    for m in re.finditer(r"POOLERR (\S+) (\S+) (\S+) (\S+) (\S+) err=(\S+)(?: bound_used=(\S+))? gate=(\S+)", pathlib.Path(path).read_text()):
        case, cfg, mode, dtype, output, err, used, gate = m.groups()
        if used is None:
            (f32 if dtype == "float32" else worst16.setdefault(f"{dtype} scaled", [])).append(
                f"{case} {cfg} {mode} {dtype} {output} err={err} gate={gate}")
        else:
            key = f"{dtype} {output} worst share of the elementwise bound"
            worst16[key] = max(worst16.get(key, 0.0), float(used))
    rec = {"float32": f32, "float32_worst_err_over_gate": max((float(l.split("err=")[1].split()[0]) / float(l.split("gate=")[1]) for l in f32),
                                                               default=None)}
    for key, val in worst16.items():
        rec[key] = val if not isinstance(val, list) else {
            "lines": len(val), "worst_err_over_gate": max(float(l.split("err=")[1].split()[0]) / float(l.split("gate=")[1]) for l in val)}
    return rec


def bench_shape(name, N, L, H, a):
    g = torch.Generator(device=dev).manual_seed(0)
    dt = torch.bfloat16
    x = torch.randn((N, L, H), generator=g, device=dev, dtype=dt).requires_grad_()
    lengths = torch.randint(L // 2, L + 1, (N,), generator=g, device=dev)
    mask = (torch.arange(L, device=dev)[None, :] < lengths[:, None]).to(torch.int64)
    go = torch.randn((N, H), generator=g, device=dev, dtype=dt)
    poolers = {mode: VodPooler(dict(CONFIG), H, mask_mode=mode).to(dev) for mode in ("reference", "masked")}
    log_scaler = poolers["reference"].log_scaler
    live = int(mask.sum())
    b = x.element_size()
    fwd_bytes = {"reference": N * L * H * b + N * H * b, "masked": live * H * b + N * H * b}
    bwd_bytes = N * L * H * b + 2 * N * H * 4
    sides = {
        "fused_reference": (lambda: poolers["reference"](x, attention_mask=mask), "reference"),
        "fused_masked": (lambda: poolers["masked"](x, attention_mask=mask), "masked"),
        "torch_reference": (lambda: reference_ops(x, mask, log_scaler), "reference"),
        "torch_masked": (lambda: reference_ops(x, mask, log_scaler, zero_pads=True), "masked"),
    }

    for lc in a.l_chunks:  # the same head with L cut into forced chunks (partial sums + a second launch): what the automatic choice is up against
        forced = VodPooler(dict(CONFIG), H, mask_mode="reference", l_chunk=lc).to(dev)
        sides[f"fused_reference_lchunk{lc}"] = (lambda forced=forced: forced(x, attention_mask=mask), "reference")

    def step(fwd):
        def run():
            x.grad = None
            y = fwd()
            y.backward(go.to(y.dtype))
        return run

    def forward_only(fwd):
        def run():
            with torch.no_grad():
                return fwd()
        return run

    times = {f"{k}_{w}": [] for k in sides for w in ("forward", "forward_backward")}
    peak = {}
    for side, (fwd, _) in sides.items():  # warm-up of every shape the timed window uses, then the peaks (one step each)
        for _ in range(a.warmup):
            forward_only(fwd)()
            step(fwd)()
        for what, fn in (("forward", forward_only(fwd)), ("forward_backward", step(fwd))):
            x.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak[f"{side}_{what}"] = torch.cuda.max_memory_allocated() - base
            del out
    for _ in range(a.reps):  # the sides alternate inside every repeat
        for side, (fwd, _) in sides.items():
            times[f"{side}_forward"].append(device_ms(forward_only(fwd), a.inner))
            times[f"{side}_forward_backward"].append(device_ms(step(fwd), a.inner))
    x.grad = None
    with torch.no_grad():  # faster and different is not faster: the outputs at the timed size, against the float32 torch sequence
        want = {False: reference_ops(x.float(), mask, log_scaler), True: reference_ops(x.float(), mask, log_scaler, zero_pads=True)}
        diff = {side: float((fwd().float() - want[mode == "masked"]).abs().max()) for side, (fwd, mode) in sides.items()}
    rec = {"shape": {"N": N, "L": L, "H": H}, "live_tokens": live, "padding_fraction": round(1 - live / (N * L), 4),
           "hidden_bytes": N * L * H * b, "algorithm_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
           "max_abs_diff_of_y_against_the_float32_torch_sequence": diff}
    for key, ts in times.items():
        side = key.rsplit("_forward", 1)[0]
        mode = sides[side][1]
        ms = statistics.median(ts)
        nbytes = fwd_bytes[mode] + (bwd_bytes if key.endswith("_backward") else 0)
        gbs = nbytes / (ms * 1e-3) / 1e9
        rec[key] = {"ms": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                    "spread": round((max(ts) - min(ts)) / ms, 4), "peak_bytes": peak[key],
                    "peak_over_hidden": round(peak[key] / (N * L * H * b), 3), "GBs": round(gbs, 1),
                    "fraction_of_stream_rate": round(gbs / (STREAM_TBS * 1e3), 4)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--poolerr", default=None, help="a pytest -s log of tests/test_pooler_gpu.py")
    ap.add_argument("--shapes", default="sections:2112,512,768;queries:64,64,768", help="name:N,L,H;...")
    ap.add_argument("--l-chunks", type=lambda v: [int(t) for t in v.split(",") if t], default=[], help="extra fused sides with a forced l_chunk")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "dtype": "bfloat16", "config": CONFIG,
           "timing": f"median of {a.reps} x {a.inner} steps between device events, {a.warmup} warm-up steps, sides alternating; "
                     "end-to-end eager step time (kernels + allocator, autograd and launch gaps), not kernel time",
           "stream_rate_TBs": STREAM_TBS}
    for item in a.shapes.split(";"):
        name, dims = item.split(":")
        N, L, H = (int(v) for v in dims.split(","))
        rec[name] = bench_shape(name, N, L, H, a)
    if a.poolerr:
        rec["poolerr"] = read_poolerr(a.poolerr)
    elif a.out and pathlib.Path(a.out).exists():  # the measured test errors live in the same file: a timing run must not drop them
        try:
            kept = json.loads(pathlib.Path(a.out).read_text()).get("poolerr")
        except (ValueError, AttributeError):
            kept = None
        if kept is not None:
            rec["poolerr"] = kept
    print(json.dumps({k: v for k, v in rec.items() if k != "poolerr"}, indent=1))
    if a.out:
        pathlib.Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
