#!/usr/bin/env python3
"""What do the exact entropy and score moments cost?  `HipFlatIndex.posterior_stats` over a 1 M x 768 fp16 store at nq 256 and 1024, in
one process on one device, alternating inside every repeat with three yardsticks:
  log_partition   the scan it extends (two more accumulators in the epilogue, 16-byte partials, a finish in double);
  mean_route      E_p[s] the way it was available before: `posterior_mean` (two scans, a second MFMA product) and `<q, mean>`;
  torch           what a user would write: chunks of the stored rows, `s = beta * (q16 @ x_chunk.T).float()`, a running maximum and the
                  max-rescaled sums of e, e s and e s^2 - it materialises an nq x chunk score block per chunk.
Every side is warmed at every shape; a repeat is device milliseconds between two events around `inner` back-to-back calls, with `inner`
sized from the warm-up so that a window lasts at least `--window` seconds; medians with the minimum and maximum over the repeats (the
run-to-run spread of this run).  CALL times on the current stream, not kernel times.
Reported per shape: the times, the ratio to `log_partition` (recorded, not gated), and the two verdicts: faster than the mean route and
faster than torch, each by more than the spread of the run, or not.  Then the same calls on a 1 M x 64 store, where the K loop is one
slice and the epilogue and the finish are nearly all of the call.  Then the measured share of the derived bound
(tests/stats_ref.py::device_bound) per word on the integer and the Gaussian shapes of tests/test_posterior_stats_gpu.py.
usage: python tools/bench_posterior_stats.py [--out profiles/posterior_stats.json] [--rows 1000000]"""
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

DIM = 768
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


def torch_moments(q16, x, beta, chunk):
    """(log_z, mean_score, var_score) from chunked score blocks with a running max-rescaled sum e, sum e s, sum e s^2 (s = beta * score)"""
    m = z = a = b = None
    for lo in range(0, x.shape[0], chunk):
        s = beta * (q16 @ x[lo : lo + chunk].T).float()
        cm = s.max(dim=1).values
        new_m = cm if m is None else torch.maximum(m, cm)
        d = s - new_m[:, None]
        e = torch.exp(d)
        ed = e * d
        zc, ac, bc = e.sum(dim=1), ed.sum(dim=1), (ed * d).sum(dim=1)
        if m is None:
            z, a, b = zc, ac, bc
        else:
            sh = m - new_m  # re-centre the running sums on the new maximum
            r = torch.exp(sh)
            z, a, b = r * z + zc, r * (a + sh * z) + ac, r * (b + 2 * sh * a + sh * sh * z) + bc
        m = new_m
    mean = a / z
    return m + torch.log(z), (m + mean) / beta, (b / z - mean * mean) / (beta * beta)


def timed_sides(sides, args, window):
    inner = {}
    for name, fn in sides.items():
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        inner[name] = max(1, int(window * 1e3 / max(device_ms(fn, 3), 1e-3)) + 1)
    ms = {name: [] for name in sides}
    for _ in range(args.repeats):
        for name, fn in sides.items():  # alternating: every repeat times every side once
            ms[name].append(device_ms(fn, inner[name]))
    r = {name: summary(v) for name, v in ms.items()}
    r["inner"] = inner
    return r


def bound_shares():
    """largest |device word - float64 word| / derived bound per word, over every query of a case family"""
    import partition_ref  # noqa: F401
    import stats_ref as S
    from test_l2_cpu import GAUSS_CASES, gauss_case

    names = ("max_score", "log_rel", "mean_rel", "var")
    tdt = {"float16": torch.float16, "bfloat16": torch.bfloat16}

    def shares(ix, q, ref, bounds, beta, into):
        st = ix.posterior_stats(torch.from_numpy(q).cuda(), temperature=1.0 / beta)
        got = (st.log_partition.max_score, st.log_partition.log_rel, st.mean_rel, st.var_score)
        for name, g, want, b in zip(names, got, ref, bounds):
            err = np.abs(g.cpu().numpy().astype(np.float64) - want)
            assert (err <= b).all(), (name, err.max())
            if (b > 0).any():
                into[name] = max(into.get(name, 0.0), float((err[b > 0] / b[b > 0]).max()))
            into["max_abs_err_" + name] = max(into.get("max_abs_err_" + name, 0.0), float(err.max()))

    out = {"integer": {}, "gaussian": {}}
    rng = np.random.default_rng(1)
    for d in (65, 768):
        x = rng.integers(-8, 9, size=(3000, d)).astype(np.float32)
        q = rng.integers(-8, 9, size=(129, d)).astype(np.float32)
        s = q.astype(np.float64) @ x.astype(np.float64).T
        for dt in tdt:
            with HipFlatIndex(d, 3000, dtype=tdt[dt], device=0) as ix:
                ix.add(x)
                for beta in (1.0 / 64.0, 1.0, 4.0):
                    ref = S.from_scores(s, beta)
                    shares(ix, q, ref, S.bounds(np.zeros((129, 1)), None, None, beta, 3000, ref, dot=False), beta, out["integer"])
    for dim, dt, seed in GAUSS_CASES:
        q, x = gauss_case(dim, seed)
        beta = float(np.float32(1.0 / np.sqrt(dim)))
        ref = S.posterior_stats(q, x, dt, beta)
        with HipFlatIndex(dim, 3000, dtype=tdt[dt], device=0) as ix:
            ix.add(x)
            shares(ix, q, ref, S.bounds(q, x, dt, beta, 3000, ref), beta, out["gaussian"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/posterior_stats.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_stats.py needs the GPU: there is no CPU path to time")

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
        f32 = dict(dtype=torch.float32, device=dev)
        out4 = tuple(torch.empty((nq,), **f32) for _ in range(4))
        out2 = tuple(torch.empty((nq,), **f32) for _ in range(2))
        out3 = (torch.empty((nq,), **f32), torch.empty((nq,), **f32), torch.empty((nq, DIM), **f32))

        def mean_route():
            return (q16.float() * ix.posterior_mean(q, temperature=1.0 / beta, out=out3).mean).sum(dim=1)

        sides = {
            "posterior_stats": lambda: ix.posterior_stats(q, temperature=1.0 / beta, out=out4),
            "log_partition": lambda: ix.log_partition(q, temperature=1.0 / beta, out=out2),
            "mean_route": mean_route,
            "torch": lambda: torch_moments(q16, x, beta, args.chunk),
        }
        st = sides["posterior_stats"]()
        tz, tmean, tvar = sides["torch"]()
        diffs = {"log_z_vs_torch": (st.log_partition.log_z.double() - tz.double()).abs().max().item(),
                 "mean_score_vs_torch": (st.mean_score.double() - tmean.double()).abs().max().item(),
                 "var_score_vs_torch": (st.var_score.double() - tvar.double()).abs().max().item(),
                 "mean_score_vs_mean_route": (st.mean_score.double() - mean_route().double()).abs().max().item()}
        r = timed_sides(sides, args, args.window)
        ps = r["posterior_stats"]
        spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in sides)
        r.update({
            "nq": nq, "ratio_to_log_partition": ps["median_ms"] / r["log_partition"]["median_ms"],
            "speedup_vs_mean_route": r["mean_route"]["median_ms"] / ps["median_ms"],
            "speedup_vs_torch": r["torch"]["median_ms"] / ps["median_ms"], "spread_ms": spread, "max_abs_diff": diffs,
            "verdict_mean_route": "faster than the mean route by more than the spread"
            if ps["median_ms"] + spread < r["mean_route"]["median_ms"] else "NOT faster than the mean route",
            "verdict_torch": "faster than torch by more than the spread" if ps["median_ms"] + spread < r["torch"]["median_ms"] else "NOT faster than torch",
        })
        result["shapes"][f"nq{nq}"] = r
        print(f"nq {nq}: posterior_stats {ps['median_ms']:.3f} ms [{ps['min_ms']:.3f}, {ps['max_ms']:.3f}]  log_partition "
              f"{r['log_partition']['median_ms']:.3f} ms (x{r['ratio_to_log_partition']:.3f})  mean route {r['mean_route']['median_ms']:.3f} ms  "
              f"torch {r['torch']['median_ms']:.3f} ms  spread {spread:.3f} ms  {r['verdict_mean_route']}; {r['verdict_torch']}  {json.dumps(diffs)}",
              flush=True)
    del x
    ix.close()
    # the one-slice store: K loop of one slice, so the epilogue, the partials and the finish are nearly all of the call
    with HipFlatIndex(64, args.rows, dtype=torch.float16, device=0) as thin:
        for lo in range(0, args.rows, 250_000):
            thin.add(torch.randn((min(250_000, args.rows - lo), 64), generator=g, device=dev).half())
        result["one_slice_dim64"] = {}
        for nq in BATCHES:
            q = torch.randn((nq, 64), generator=g, device=dev)
            sides = {"posterior_stats": lambda: thin.posterior_stats(q, temperature=8.0),
                     "log_partition": lambda: thin.log_partition(q, temperature=8.0)}
            r = timed_sides(sides, args, 0.3 * args.window)
            r["ratio_to_log_partition"] = r["posterior_stats"]["median_ms"] / r["log_partition"]["median_ms"]
            result["one_slice_dim64"][f"nq{nq}"] = r
        print("one-slice store (dim 64):", json.dumps(result["one_slice_dim64"]), flush=True)

    result["share_of_derived_bound"] = bound_shares()
    print(json.dumps(result["share_of_derived_bound"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
