#!/usr/bin/env python3
"""What does the VOD step cost?  B=8, D=8, L=256, V=32128, H=768, bf16, 3-D sections, 25 % trailing padding (the shape of
tools/bench_marginal.py), log-weights of a priority sample without replacement, alpha = 0.5.

Times, in one process on one device, the three sides alternating inside every repeat (median device milliseconds between two events
around `--inner` back-to-back steps, after `--warmup` untimed steps of each).  These are END-TO-END STEP times of the eager path: the
kernels plus the allocator and launch gaps between them, not kernel times:
  vod        `vod_amd.gradients.VodGradients`: forward, and forward + backward
  marginal   `vod_amd.gradients.MarginalLikelihoodGradients` on the same tensors: the step the VOD step differs from by a row kernel over
             B x D words only, hence the yardstick; `vod_over_marginal` is the ratio of the medians, `marginal_spread` the marginal
             side's own (max - min) / median over the repeats of this run
  torch_ops  the formulas of include/vodhip.h H5v as a plain-torch op sequence (log_softmax over V, gather, masked mean, the
             logsumexp / expm1 / log1p row arithmetic) with torch's autograd backward
Per side: ms, and the peak of `torch.cuda.max_memory_allocated` above what the inputs occupy.
An `errors` key already in the `--out` file (the measured test errors, profiles/README.md) is carried over.
usage: python tools/bench_vod.py [--out profiles/vod_gradients.json]"""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd.gradients import MarginalLikelihoodGradients, VodGradients  # noqa: E402

dev = torch.device("cuda", 0)


def torch_ops(batch, q, s, lm_logits, alpha, temperature):
    """The VOD objective (mean token reduction, every section live) as the op sequence a torch user would write."""
    score, logw = batch["section__score"], batch["section__log_weight"]
    ids, mask = batch["lm__input_ids"], batch["lm__attention_mask"]
    r = torch.einsum("bh,bdh->bd", q, s) if s.dim() == 3 else torch.einsum("bh,dh->bd", q, s)
    ids1, mask1 = ids[..., 1:], mask[..., 1:]
    x = lm_logits[..., :-1, :].masked_fill((mask1 == 0).unsqueeze(-1), -torch.inf)
    lp = torch.nn.functional.log_softmax(x, dim=-1)[..., :-1].gather(dim=-1, index=ids1.unsqueeze(-1)).squeeze(-1)
    l = lp.masked_fill(mask1 == 0, 0.0).sum(dim=-1) / mask1.sum(dim=-1)
    ls = logw.log_softmax(dim=-1)
    g = r.float() - temperature * score
    lw = l.float() + g - torch.logsumexp(ls + g, dim=-1, keepdim=True)
    eps = 1.0 - alpha
    if eps == 0:
        lhat = (ls.exp() * lw).sum(-1)
    else:
        m = lw.max(dim=-1, keepdim=True).values.detach()
        lhat = m.squeeze(-1) + torch.log1p((ls.exp() * torch.expm1(eps * (lw - m))).sum(-1)) / eps
    return -lhat.mean()


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
    ap.add_argument("--alpha", type=float, default=0.5)
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
    score = torch.randn((B, D), generator=g, device=dev)
    batch = {"section__score": score, "section__log_weight": torch.randn((B, D), generator=g, device=dev).log_softmax(-1),
             "lm__attention_mask": mask, "lm__input_ids": torch.randint(0, V - 1, (B, D, L), generator=g, device=dev)}
    vod, marginal = VodGradients(alpha=a.alpha), MarginalLikelihoodGradients()

    def drop_grads():
        q.grad = s.grad = lm_logits.grad = None

    def vod_fwd():
        return vod(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lm_logits).loss

    def marginal_fwd():
        return marginal(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lm_logits).loss

    def ops_fwd():
        return torch_ops(batch, q, s, lm_logits, a.alpha, 1.0)

    def step(fwd):
        def run():
            drop_grads()
            fwd().backward()
        return run

    sides = {"vod": vod_fwd, "marginal": marginal_fwd, "torch_ops": ops_fwd}
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
    for _ in range(a.reps):  # the sides alternate inside every repeat
        for name, fwd in sides.items():
            times[f"{name}_forward"].append(device_ms(fwd, a.inner))
            times[f"{name}_forward_backward"].append(device_ms(step(fwd), a.inner))
    drop_grads()
    with torch.no_grad():
        out = vod(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lm_logits)
        losses = {"vod": float(out.loss), "torch_ops_bf16": float(ops_fwd()), **{k: float(v) for k, v in out.diagnostics.items()}}
    logits_bytes = B * D * L * V * lm_logits.element_size()
    rec = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "D": D, "L": L, "V": V, "H": H}, "dtype": "bfloat16",
           "sections": "3-D", "padding": "25 % trailing", "alpha": a.alpha, "logits_bytes": logits_bytes,
           "timing": f"median of {a.reps} x {a.inner} steps between device events, {a.warmup} warm-up steps, sides alternating; "
                     "end-to-end eager step time (kernels + allocator and launch gaps), not kernel time",
           "loss": losses}
    for key, ts in times.items():
        rec[key] = {"ms": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                    "peak_bytes": peak[key], "peak_over_logits": round(peak[key] / logits_bytes, 3)}
    for what in ("forward", "forward_backward"):
        m = rec[f"marginal_{what}"]
        rec[f"vod_over_marginal_{what}"] = round(rec[f"vod_{what}"]["ms"] / m["ms"], 4)
        rec[f"marginal_spread_{what}"] = round((m["ms_max"] - m["ms_min"]) / m["ms"], 4)
    print(json.dumps(rec, indent=1))
    if a.out:
        out_path = pathlib.Path(a.out)
        if out_path.exists():  # the measured test errors live in the same file: a new timing run must not drop them
            try:
                kept = json.loads(out_path.read_text()).get("errors")
            except (ValueError, AttributeError):
                kept = None
            if kept is not None:
                rec["errors"] = kept
        out_path.write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
