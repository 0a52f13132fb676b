#!/usr/bin/env python3
"""What do exact samples from the posterior cost?  `HipFlatIndex.sample_posterior` over a 1 M x 768 fp16 store and over a 1 M x 64 one,
at nq 256 and 1024 and k 32 and 100, in one process on one device, alternating inside every repeat with three yardsticks:
  log_partition  the normaliser alone of the same batch (its three launches are the first part of sample_posterior);
  search         `search(q, k + 1)` of the same batch (a top-(k+1) WITHOUT noise: what the truncated proposal costs today);
  torch          THE YARDSTICK a user would write today, over chunks of the stored rows: `beta * q16 @ x_chunk.T - log(Exponential)`,
                 `topk(k + 1)`, and a running merge of the chunk lists - it materialises an nq x chunk score and noise block per chunk.
Timing as tools/bench_posterior_mean.py: every side warmed at every shape, a repeat is device milliseconds between two events around
`inner` back-to-back calls, medians with the minimum and maximum over the repeats.  CALL times on the current stream (sample_posterior
waits for its stream at the end of every call: that wait is inside its time).
Reported per shape: the times, the multiple of log_partition's time beside the cost model's (DESIGN.md 4 "Posterior sampling"), the
ratio to torch and the verdict with the spread it used; from one extra call with param "profile" = 1 the split per launch (HIP events);
the candidates per query (mean and max) and the share of emit-scan workgroups that skipped their K loop.  Then the measured key error
against float64 on two Gaussian shapes of tests/test_sample_posterior_gpu.py as a share of the derived bound
(tests/sample_posterior_ref.py::device_key_bound).
usage: python tools/bench_sample_posterior.py [--out profiles/sample_posterior.json] [--rows 1000000]"""
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
KS = (32, 100)
SEED = 20261019
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


def torch_sample(q16, x, beta, k, chunk):
    best_k, best_i = None, None
    for lo in range(0, x.shape[0], chunk):
        s = beta * (q16 @ x[lo : lo + chunk].T).float()
        key = s - torch.log(torch.empty_like(s).exponential_())
        kk, ii = torch.topk(key, min(k + 1, key.shape[1]), dim=1)
        ii = ii + lo
        if best_k is not None:
            kk, ii = torch.cat((best_k, kk), dim=1), torch.cat((best_i, ii), dim=1)
            kk, sel = torch.topk(kk, min(k + 1, kk.shape[1]), dim=1)
            ii = torch.gather(ii, 1, sel)
        best_k, best_i = kk, ii
    return best_k, best_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sample_posterior.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_posterior.py needs the GPU: there is no CPU path to time")

    g = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "store": "float16", "repeats": args.repeats, "window_s": args.window,
              "torch_chunk_rows": args.chunk, "shapes": {}}
    for dim in (768, 64):
        with HipFlatIndex(dim, args.rows, dtype=torch.float16, device=0) as ix:
            for lo in range(0, args.rows, 250_000):
                ix.add(torch.randn((min(250_000, args.rows - lo), dim), generator=g, device=dev).half())
            x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
            beta = float(torch.tensor(dim ** -0.5, dtype=torch.float32))
            for nq in BATCHES:
                q = torch.randn((nq, dim), generator=g, device=dev)
                q16 = q.half()
                out2 = tuple(torch.empty((nq,), dtype=torch.float32, device=dev) for _ in range(2))
                for k in KS:
                    f32 = dict(dtype=torch.float32, device=dev)
                    out7 = out2 + (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), **f32), torch.empty((nq, k), **f32),
                                   torch.empty((nq, k), **f32), torch.empty((nq, k + 1), **f32))
                    sides = {
                        "sample_posterior": lambda: ix.sample_posterior(q, k, temperature=1.0 / beta, seed=SEED, out=out7),
                        "log_partition": lambda: ix.log_partition(q, temperature=1.0 / beta, out=out2),
                        "search": lambda: ix.search(q, k + 1),
                        "torch": lambda: torch_sample(q16, x, beta, k, args.chunk),
                    }
                    inner = {}
                    for name, fn in sides.items():
                        for _ in range(args.warmup):
                            fn()
                        torch.cuda.synchronize()
                        inner[name] = max(1, int(args.window * 1e3 / max(device_ms(fn, 2), 1e-3)) + 1)
                    ms = {name: [] for name in sides}
                    for _ in range(args.repeats):
                        for name, fn in sides.items():  # alternating: every repeat times every side once
                            ms[name].append(device_ms(fn, inner[name]))
                    r = {name: summary(v) for name, v in ms.items()}
                    ix.set_param("profile", 1)
                    sides["sample_posterior"]()
                    ix.set_param("profile", 0)
                    split = {p: ix.get_stat("last_sample_ns_" + p) * 1e-6 for p in ("partition", "keymax", "threshold", "emit", "select")}
                    cand, cmax = ix.get_stat("last_sample_candidates"), ix.get_stat("last_sample_max_candidates")
                    groups, skipped = ix.get_stat("last_sample_emit_groups"), ix.get_stat("last_sample_emit_skipped")
                    sp, lp, th = r["sample_posterior"], r["log_partition"], r["torch"]
                    spread = max(sp["max_ms"] - sp["min_ms"], th["max_ms"] - th["min_ms"])
                    hit = 1.0 - skipped / max(groups, 1)
                    r.update({
                        "nq": nq, "dim": dim, "k": k, "beta": beta, "inner": inner, "launch_ms": split,
                        "launch_multiple_of_partition": {p: v / max(split["partition"], 1e-9) for p, v in split.items()},
                        "candidates_mean": cand / nq, "candidates_max": cmax, "emit_groups": groups, "emit_groups_skipped": skipped,
                        "emit_skip_share": skipped / max(groups, 1),
                        "multiple_of_log_partition": sp["median_ms"] / lp["median_ms"],
                        "cost_model": f"1 (partition) + keymax + {hit:.3f} (emit hit share) + threshold + select",
                        "multiple_of_search": sp["median_ms"] / r["search"]["median_ms"],
                        "speedup_vs_torch": th["median_ms"] / sp["median_ms"], "spread_ms": spread,
                        "overflow": ix.get_stat("last_sample_overflow"), "selfcheck": ix.get_stat("last_sample_selfcheck"),
                        "verdict": "faster than torch by more than the spread" if sp["median_ms"] + spread < th["median_ms"] else "NOT faster than torch",
                    })
                    result["shapes"][f"dim{dim}_nq{nq}_k{k}"] = r
                    print(f"dim {dim} nq {nq} k {k}: sample_posterior {sp['median_ms']:.3f} ms [{sp['min_ms']:.3f}, {sp['max_ms']:.3f}]  log_partition "
                          f"{lp['median_ms']:.3f} ms  x{r['multiple_of_log_partition']:.2f}  search {r['search']['median_ms']:.3f} ms  torch "
                          f"{th['median_ms']:.3f} ms [{th['min_ms']:.3f}, {th['max_ms']:.3f}]  {r['speedup_vs_torch']:.2f} x torch  launches "
                          + " ".join(f"{p} {v:.3f}" for p, v in split.items())
                          + f"  candidates mean {cand / nq:.1f} max {cmax}  emit skipped {skipped}/{groups}  {r['verdict']}", flush=True)
            del x

    # measured key error against float64 on two Gaussian shapes of tests/test_sample_posterior_gpu.py, as a share of the derived bound
    import partition_ref as P  # noqa: E402  (tests/)
    import sample_posterior_ref as R  # noqa: E402

    result["accuracy"] = {}
    for n, dim, nq, k in ((3000, 765, 300, 4), (20000, 64, 130, 32)):
        rng = np.random.default_rng(9000 + dim + n + nq)
        xa = rng.standard_normal((n, dim)).astype(np.float32)
        qa = rng.standard_normal((nq, dim)).astype(np.float32)
        b = float(np.float32(1.0 / np.sqrt(dim)))
        with HipFlatIndex(dim, n, dtype=torch.float16, device=0) as small:
            small.add(xa)
            got = small.sample_posterior(torch.from_numpy(qa).to(dev), k, temperature=1.0 / b, seed=SEED)
        ids, keys = got.ids.cpu().numpy(), got.keys.cpu().numpy()[:, :k].astype(np.float64)
        keymat = R.keys_from_scores(P.scores(qa, xa, "float16"), b, SEED)[0]
        bound = np.take_along_axis(R.key_bound(qa, xa, "float16", b, SEED, dot=True), ids, axis=1)
        err = np.abs(keys - np.take_along_axis(keymat, ids, axis=1))
        result["accuracy"][f"gauss_{n}x{dim}_k{k}_float16"] = {
            "beta": b, "max_abs_err_key": float(err.max()), "max_err_over_bound": float((err / bound).max())}
    print(json.dumps(result["accuracy"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
