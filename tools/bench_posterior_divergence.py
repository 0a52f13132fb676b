#!/usr/bin/env python3
"""What does the exact divergence between two query sets cost?  `HipFlatIndex.posterior_divergence` over a 1 M x 768 and a 1 M x 64 fp16
store at 256 and 1024 pairs, in one process on one device, alternating inside every repeat with three yardsticks:
  stats_2nq   `posterior_stats` of the 2 nq concatenated queries: the kernel this one extends doing the same MFMA work (the same K
              loop, the same number of exponentials per staged column) - the cost model says the divergence call is 1.0 - 1.15 x this;
  two_stats   two `posterior_stats` calls, one per side: what a user had before, and it still lacks the cross moments;
  torch       what a user would write for the exact KL: chunks of the stored rows, two score blocks per chunk, running maxima and the
              max-rescaled sums of e_a, e_a s_a, e_a s_b and their mirror - it materialises two nq x chunk score blocks per chunk.
Every side is warmed at every shape; a repeat is device milliseconds between two events around `inner` back-to-back calls, with `inner`
sized from the warm-up so that a window lasts at least `--window` seconds; medians with the minimum and maximum over the repeats (the
run-to-run spread of this run).  CALL times on the current stream, not kernel times.  No ratio is gated: the ratios and the spread are
recorded.  Then the measured share of the derived bounds (tests/divergence_ref.py) per word on the integer and the Gaussian shapes of
tests/test_posterior_divergence_gpu.py.
usage: python tools/bench_posterior_divergence.py [--out profiles/posterior_divergence.json] [--rows 1000000]"""
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

DIMS = (768, 64)
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


def torch_kl(qa16, qb16, x, beta_a, beta_b, chunk):
    """(kl_ab, kl_ba) from chunked score blocks: per side a running maximum and the max-rescaled sums of e, e d_own and e d_other
    (d = beta * score - running maximum of that side)"""
    st = None
    for lo in range(0, x.shape[0], chunk):
        xc = x[lo : lo + chunk].T
        s = (beta_a * (qa16 @ xc).float(), beta_b * (qb16 @ xc).float())
        cm = (s[0].max(dim=1).values, s[1].max(dim=1).values)
        new_m = cm if st is None else (torch.maximum(st[0][0], cm[0]), torch.maximum(st[0][1], cm[1]))
        d = (s[0] - new_m[0][:, None], s[1] - new_m[1][:, None])
        sums = []
        for k in (0, 1):
            e = torch.exp(d[k])
            sums.append((e.sum(dim=1), (e * d[k]).sum(dim=1), (e * d[1 - k]).sum(dim=1)))
        if st is not None:
            sh = (st[0][0] - new_m[0], st[0][1] - new_m[1])  # re-centre the running sums on the new maxima
            for k in (0, 1):
                r = torch.exp(sh[k])
                z, a, c = st[1][k]
                sums[k] = (r * z + sums[k][0], r * (a + sh[k] * z) + sums[k][1], r * (c + sh[1 - k] * z) + sums[k][2])
        st = (new_m, sums)
    (za, aa, cab), (zb, ab, cba) = st[1]
    la, lb = torch.log(za), torch.log(zb)
    return (lb - la) + (aa / za - cab / za), (la - lb) + (ab / zb - cba / zb)


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
    """largest |device word - float64 word| / derived bound per word, over every pair of a case family"""
    import divergence_ref as D
    from test_l2_cpu import GAUSS_CASES, gauss_case

    tdt = {"float16": torch.float16, "bfloat16": torch.bfloat16}

    def shares(ix, qa, qb, ref, b8, ba, bb, into):
        r = ix.posterior_divergence(torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), temperature_a=1.0 / ba, temperature_b=1.0 / bb)
        a, b = r.stats_a, r.stats_b
        got = (a.max_score, a.log_rel, a.mean_rel, r.cross_rel_ab, b.max_score, b.log_rel, b.mean_rel, r.cross_rel_ba,
               r.entropy_a, r.entropy_b, r.cross_entropy_ab, r.cross_entropy_ba, r.kl_ab, r.kl_ba)
        want = ref.words + D.derived(ref.words, ba, bb)
        bounds = tuple(b8) + D.derived_bounds(ba, bb, ref.words, b8)
        for name, g, w, bd in zip(D.WORDS + D.DERIVED, got, want, bounds):
            err = np.abs(g.cpu().numpy().astype(np.float64) - w)
            assert (err <= bd).all(), (name, err.max())
            if (bd > 0).any():
                into[name] = max(into.get(name, 0.0), float((err[bd > 0] / bd[bd > 0]).max()))
            into["max_abs_err_" + name] = max(into.get("max_abs_err_" + name, 0.0), float(err.max()))

    out = {"integer": {}, "gaussian": {}}
    rng = np.random.default_rng(1)
    for d in (65, 768):
        x = rng.integers(-8, 9, size=(3000, d)).astype(np.float32)
        qa = rng.integers(-8, 9, size=(129, d)).astype(np.float32)
        qb = np.roll(qa, 1, axis=0)
        sa = qa.astype(np.float64) @ x.astype(np.float64).T
        sb = np.roll(sa, 1, axis=0)
        for dt in tdt:
            with HipFlatIndex(d, 3000, dtype=tdt[dt], device=0) as ix:
                ix.add(x)
                for ba, bb in ((1.0 / 64.0, 1.0 / 64.0), (1.0, 1.0 / 64.0), (4.0, 1.0)):
                    ref = D.from_scores(sa, sb, ba, bb)
                    shares(ix, qa, qb, ref, D.bounds(None, None, None, None, ba, bb, ref, dot=False), ba, bb, out["integer"])
    for dim, dt, seed in GAUSS_CASES:
        qa, x = gauss_case(dim, seed)
        qb = np.roll(qa, 1, axis=0)
        ba, bb = float(np.float32(1.0 / np.sqrt(dim))), float(np.float32(0.5 / np.sqrt(dim)))
        ref = D.posterior_divergence(qa, qb, x, dt, ba, bb)
        with HipFlatIndex(dim, 3000, dtype=tdt[dt], device=0) as ix:
            ix.add(x)
            shares(ix, qa, qb, ref, D.bounds(qa, qb, x, dt, ba, bb, ref), ba, bb, out["gaussian"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/posterior_divergence.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.6, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_posterior_divergence.py needs the GPU: there is no CPU path to time")

    g = torch.Generator(device=dev).manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "store": "float16", "repeats": args.repeats, "window_s": args.window,
              "torch_chunk_rows": args.chunk, "cost_model_ratio_to_stats_2nq": [1.0, 1.15], "stores": {}}
    for dim in DIMS:
        ix = HipFlatIndex(dim, args.rows, dtype=torch.float16, device=0)
        for lo in range(0, args.rows, 250_000):
            ix.add(torch.randn((min(250_000, args.rows - lo), dim), generator=g, device=dev).half())
        x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
        beta_a = float(torch.tensor(dim ** -0.5, dtype=torch.float32))
        beta_b = float(torch.tensor(0.5 * dim ** -0.5, dtype=torch.float32))
        store = result["stores"][f"dim{dim}"] = {"dim": dim, "beta_a": beta_a, "beta_b": beta_b, "shapes": {}}
        for nq in BATCHES:
            qa = torch.randn((nq, dim), generator=g, device=dev)
            qb = qa + 0.5 * torch.randn((nq, dim), generator=g, device=dev)  # a student near its teacher
            qa16, qb16 = qa.half(), qb.half()
            qcat = torch.cat([qa, qb])
            f32 = dict(dtype=torch.float32, device=dev)
            out8 = tuple(torch.empty((nq,), **f32) for _ in range(8))
            out4 = tuple(torch.empty((2 * nq,), **f32) for _ in range(4))
            out4a = tuple(torch.empty((nq,), **f32) for _ in range(4))
            out4b = tuple(torch.empty((nq,), **f32) for _ in range(4))

            def two_stats():
                ix.posterior_stats(qa, temperature=1.0 / beta_a, out=out4a)
                return ix.posterior_stats(qb, temperature=1.0 / beta_b, out=out4b)

            sides = {
                "posterior_divergence": lambda: ix.posterior_divergence(qa, qb, temperature_a=1.0 / beta_a, temperature_b=1.0 / beta_b, out=out8),
                "stats_2nq": lambda: ix.posterior_stats(qcat, temperature=1.0 / beta_a, out=out4),
                "two_stats": two_stats,
                "torch": lambda: torch_kl(qa16, qb16, x, beta_a, beta_b, args.chunk),
            }
            dv = sides["posterior_divergence"]()
            t_ab, t_ba = sides["torch"]()
            diffs = {"kl_ab_vs_torch": (dv.kl_ab.double() - t_ab.double()).abs().max().item(),
                     "kl_ba_vs_torch": (dv.kl_ba.double() - t_ba.double()).abs().max().item(),
                     "kl_ab_max": dv.kl_ab.max().item(), "kl_ab_min": dv.kl_ab.min().item()}
            r = timed_sides(sides, args, args.window)
            pd = r["posterior_divergence"]
            spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in sides)
            ratio = pd["median_ms"] / r["stats_2nq"]["median_ms"]
            r.update({
                "nq": nq, "ratio_to_stats_2nq": ratio, "ratio_to_two_stats": pd["median_ms"] / r["two_stats"]["median_ms"],
                "speedup_vs_torch": r["torch"]["median_ms"] / pd["median_ms"], "spread_ms": spread, "max_abs_diff": diffs,
                "against_cost_model": "inside 1.0 - 1.15 x stats_2nq" if ratio <= 1.15 + spread / r["stats_2nq"]["median_ms"]
                else "ABOVE the cost model by more than the spread",
                "verdict_torch": "faster than torch by more than the spread" if pd["median_ms"] + spread < r["torch"]["median_ms"] else "NOT faster than torch",
            })
            store["shapes"][f"nq{nq}"] = r
            print(f"dim {dim} nq {nq}: posterior_divergence {pd['median_ms']:.3f} ms [{pd['min_ms']:.3f}, {pd['max_ms']:.3f}]  stats of 2 nq "
                  f"{r['stats_2nq']['median_ms']:.3f} ms (x{ratio:.3f})  two stats calls {r['two_stats']['median_ms']:.3f} ms "
                  f"(x{r['ratio_to_two_stats']:.3f})  torch {r['torch']['median_ms']:.3f} ms (x{r['speedup_vs_torch']:.2f})  spread {spread:.3f} ms  "
                  f"{r['against_cost_model']}; {r['verdict_torch']}  {json.dumps(diffs)}", flush=True)
        del x
        ix.close()

    result["share_of_derived_bound"] = bound_shares()
    print(json.dumps(result["share_of_derived_bound"]), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
