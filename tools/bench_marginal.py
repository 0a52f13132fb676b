#!/usr/bin/env python3
"""What does the marginal-likelihood step cost?  B=8, D=8, L=256, V=32128, H=768, bf16, 3-D sections, 25 % trailing padding.

Times, in one process on one device, alternating the two sides (median device milliseconds between two events around `--inner`
back-to-back steps, after `--warmup` untimed steps of each).  These are END-TO-END STEP times of the eager path: the kernels plus the
allocator and launch gaps between them, not kernel times - the GB/s below is a step rate, a lower bound of the kernels' own rate:
  fused      `vod_amd.gradients.MarginalLikelihoodGradients`: forward, and forward + backward
  reference  a torch restatement of the reference's op sequence (marginal_likelihood.py:21-66: einsum, masked_fill, log_softmax, the
             shifted masked_fill / log_softmax / slice / gather / masked_fill of the logits, logsumexp) with torch's autograd backward
Per side: ms, the peak of `torch.cuda.max_memory_allocated` above what the inputs occupy, the achieved GB/s over the bytes the
ALGORITHM needs (forward: live positions * V * b read; backward: the same read again + N * L * V * b written - the reference side is
charged the same bytes, so its rate says how far its extra passes put it from the stream), and that rate over the 6.29 TB/s measured
streaming rate of the device.
An `errors` key already in the `--out` file (the measured test errors, profiles/README.md) is carried over.
usage: python tools/bench_marginal.py [--out profiles/marginal_likelihood.json]"""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd.gradients import MarginalLikelihoodGradients  # noqa: E402

STREAM_TBS = 6.29  # measured streaming rate of the MI355X
dev = torch.device("cuda", 0)


def reference_ops(batch, q, s, lm_logits):
    """The reference's op sequence, restated in torch (no reference code is imported)."""
    score, ids, mask = batch["section__score"], batch["lm__input_ids"], batch["lm__attention_mask"]
    pad = score.isinf() & (score < 0)
    r = torch.einsum("bh,bdh->bd", q, s) if s.dim() == 3 else torch.einsum("bh,dh->bd", q, s)
    r = r.masked_fill(pad, -torch.inf)
    lp_r = r.log_softmax(dim=-1)
    ids1, mask1 = ids[..., 1:], mask[..., 1:]
    x = lm_logits[..., :-1, :].masked_fill((mask1 == 0).unsqueeze(-1), -torch.inf)
    lp = torch.nn.functional.log_softmax(x, dim=-1)[..., :-1].gather(dim=-1, index=ids1.unsqueeze(-1)).squeeze(-1)
    lp_xz = lp.masked_fill(mask1 == 0, 0.0).sum(dim=-1) / mask1.sum(dim=-1)
    return -torch.logsumexp(lp_r + lp_xz, dim=-1).mean(), r


def device_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="8,8,256,32128,768", help="B,D,L,V,H")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    a = ap.parse_args()
    B, D, L, V, H = (int(v) for v in a.shape.split(","))
    g = torch.Generator(device=dev).manual_seed(0)
    dt = torch.bfloat16
    q = torch.randn((B, H), generator=g, device=dev).mul_(H ** -0.5).to(dt).requires_grad_()
    s = torch.randn((B, D, H), generator=g, device=dev).to(dt).requires_grad_()
    lm_logits = torch.randn((B, D, L, V), generator=g, device=dev, dtype=dt).mul_(3.0).requires_grad_()
    mask = torch.ones((B, D, L), dtype=torch.int64, device=dev)
    mask[..., L - L // 4:] = 0  # 25 % trailing padding
    batch = {"section__score": torch.zeros((B, D), device=dev), "lm__attention_mask": mask,
             "lm__input_ids": torch.randint(0, V - 1, (B, D, L), generator=g, device=dev)}
    fused = MarginalLikelihoodGradients()
    esize = lm_logits.element_size()
    live = int(mask[..., 1:].sum())
    fwd_bytes = live * V * esize
    bwd_bytes = fwd_bytes + B * D * L * V * esize

    def drop_grads():
        q.grad = s.grad = lm_logits.grad = None

    def fused_fwd():
        return fused(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lm_logits).loss

    def ref_fwd():
        return reference_ops(batch, q, s, lm_logits)[0]

    def step(fwd):
        def run():
            drop_grads()
            fwd().backward()
        return run

    sides = {"fused": fused_fwd, "reference": ref_fwd}
    times = {f"{k}_{w}": [] for k in sides for w in ("forward", "forward_backward")}
    peak = {}
    for name, fwd in sides.items():  # warm-up of every shape the timed window uses, then the peaks (one step each)
        for _ in range(a.warmup):
            fwd()
            step(fwd)()
        for what, fn in (("forward", fwd), ("forward_backward", step(fwd))):
            drop_grads()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            peak[f"{name}_{what}"] = torch.cuda.max_memory_allocated() - base
            del out
    for _ in range(a.reps):  # the two sides alternate inside every repeat
        for name, fwd in sides.items():
            times[f"{name}_forward"].append(device_ms(fwd, a.inner))
            times[f"{name}_forward_backward"].append(device_ms(step(fwd), a.inner))
    drop_grads()
    with torch.no_grad():
        l_f, l_r = float(fused_fwd()), float(ref_fwd())
    rec = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "D": D, "L": L, "V": V, "H": H}, "dtype": "bfloat16",
           "sections": "3-D", "padding": "25 % trailing", "live_positions": live, "logits_bytes": B * D * L * V * esize,
           "algorithm_bytes": {"forward": fwd_bytes, "forward_backward": fwd_bytes + bwd_bytes},
           "timing": f"median of {a.reps} x {a.inner} steps between device events, {a.warmup} warm-up steps, sides alternating; "
                     "end-to-end eager step time (kernels + allocator and launch gaps), not kernel time",
           "stream_rate_TBs": STREAM_TBS, "loss": {"fused": l_f, "reference_ops_bf16": l_r}}
    for key, ts in times.items():
        ms = statistics.median(ts)
        nbytes = fwd_bytes if key.endswith("_forward") else fwd_bytes + bwd_bytes
        gbs = nbytes / (ms * 1e-3) / 1e9
        rec[key] = {"ms": round(ms, 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "peak_bytes": peak[key],
                    "peak_over_logits": round(peak[key] / (B * D * L * V * esize), 3), "GBs": round(gbs, 1),
                    "fraction_of_stream_rate": round(gbs / (STREAM_TBS * 1e3), 4)}
    print(json.dumps(rec, indent=1))
    if a.out:
        out = pathlib.Path(a.out)
        if out.exists():  # the measured test errors live in the same file: a new timing run must not drop them
            try:
                kept = json.loads(out.read_text()).get("errors")
            except (ValueError, AttributeError):
                kept = None
            if kept is not None:
                rec["errors"] = kept
        out.write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
