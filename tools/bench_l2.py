#!/usr/bin/env python3
"""What does the L2 metric cost beside inner product?  In one process on one device, on two stores of the SAME rows (1 M x dim fp16,
N(0, 1)): `HipFlatIndex(metric="l2")` against `HipFlatIndex()` - the yardstick is the inner-product time of the same run.

search   float32 queries, k = 100, at
           c2      1 M x 768, nq 256     (dim_pad 832 against 768: the L2 scan reads 13 K-tiles instead of 12 = 1.083)
           d765    1 M x 765, nq 256     (dim_pad 768 both: the bias columns live in the padding, the scan reads no more than before)
           nq1024  1 M x 768, nq 1024
         each timed two ways: `eager` = `search()` calls one after the other (enqueue, wait, check), `ahead` = the caller keeps one
         search in flight (`search_async` of batch i + 1 before `finish` of batch i).  Host clock around `--inner` searches that end in
         a device synchronise; the sides alternate inside every repeat; medians with minimum and maximum over the repeats.  Reported:
         the ratio L2 / inner product of the medians beside the run-to-run spread of the inner-product time, (max - min) / median, and
         the excess of the ratio over dim_pad_L2 / dim_pad_IP.
ingest   1 M x 768 float32 rows in pageable host memory -> HBM through `add` (reset first), GB/s of source bytes, alternating sides.
check    the L2 ids of four queries against a float32 torch evaluation of |q - x|^2 over the stored rows (rows whose float32
         distances tie within 1e-3 may swap).
usage: python tools/bench_l2.py [--out profiles/l2_search.json] [--rows 1000000]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd.index import HipFlatIndex  # noqa: E402

SHAPES = [("c2", 768, 256), ("nq1024", 768, 1024), ("d765", 765, 256)]  # (the two 768-wide shapes share their stores)
K = 100
dev = torch.device("cuda", 0)


def summary(ms):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med}


def eager_ms(ix, batches, outs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for q, o in zip(batches, outs):
        ix.search(q, K, out=o)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


def ahead_ms(ix, batches, outs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ix.search_async(batches[0], K, out=outs[0])
    for q, o in zip(batches[1:], outs[1:]):
        ix.search_async(q, K, out=o)
        ix.finish()
    ix.finish()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


def build(dim, rows, seed):
    ip = HipFlatIndex(dim, rows, dtype=torch.float16, device=0)
    l2 = HipFlatIndex(dim, rows, dtype=torch.float16, device=0, metric="l2")
    g = torch.Generator(device=dev).manual_seed(seed)
    for lo in range(0, rows, 250_000):
        part = torch.randn((min(250_000, rows - lo), dim), generator=g, device=dev).half()
        ip.add(part)
        l2.add(part)
    return ip, l2, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/l2_search.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ingest-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_l2.py needs the GPU: there is no CPU path to time")
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "store": "float16", "k": K, "repeats": args.repeats,
              "inner": args.inner, "search": {}, "ingest": {}}
    stores = {}
    for name, dim, nq in SHAPES:
        if dim not in stores:
            stores.clear()  # one pair of stores at a time
            stores[dim] = build(dim, args.rows, seed=dim)
        ip, l2, g = stores[dim]
        batches = [torch.randn((nq, dim), generator=g, device=dev) for _ in range(args.inner)]
        outs = [(torch.empty((nq, K), dtype=torch.float32, device=dev), torch.empty((nq, K), dtype=torch.int64, device=dev)) for _ in batches]
        sides = {"ip": ip, "l2": l2}
        ms = {(s, m): [] for s in sides for m in ("eager", "ahead")}
        for _ in range(args.warmup):
            for ix in sides.values():
                eager_ms(ix, batches, outs)
                ahead_ms(ix, batches, outs)
        for _ in range(args.repeats):
            for mode, fn in (("eager", eager_ms), ("ahead", ahead_ms)):
                for s, ix in sides.items():  # alternating: every repeat times every side once
                    ms[(s, mode)].append(fn(ix, batches, outs))
        pad_ratio = l2.get_stat("dim_pad") / ip.get_stat("dim_pad")
        r = {"dim": dim, "nq": nq, "dim_pad_ip": ip.get_stat("dim_pad"), "dim_pad_l2": l2.get_stat("dim_pad"), "dim_pad_ratio": pad_ratio}
        for mode in ("eager", "ahead"):
            a, b = summary(ms[("ip", mode)]), summary(ms[("l2", mode)])
            ratio = b["median_ms"] / a["median_ms"]
            r[mode] = {"ip": a, "l2": b, "l2_over_ip": ratio, "ip_spread": a["spread"], "excess_over_dim_pad_ratio": ratio - pad_ratio,
                       "within_twice_the_spread": ratio - pad_ratio <= 2 * a["spread"]}
        # check: four queries against a float32 evaluation over the stored rows
        x = l2.stored_rows().float()
        q16 = batches[0][:4].half().float()
        _, ids = l2.search(batches[0][:4], K)
        agree = 0
        for a in range(4):
            d = (x - q16[a]).pow_(2).sum(dim=1)
            kth = torch.topk(d, K, largest=False).values[-1]
            agree += int((d[ids[a]] <= kth + 1e-3).sum().item())
        del x
        r["ids_within_float32_topk"] = agree / (4 * K)
        # where the L2 side's extra time goes: HIP events around its two extra launches ("profile"; a pass of its own, not timed above)
        l2.set_param("profile", 1)
        prof = {"stage_us": [], "finish_us": [], "filter_us": []}
        for q, o in zip(batches, outs):
            l2.search(q, K, out=o)
            prof["stage_us"].append(l2.get_stat("last_l2_stage_ns") / 1e3)
            prof["finish_us"].append(l2.get_stat("last_l2_finish_ns") / 1e3)
            prof["filter_us"].append(l2.get_stat("last_filter_ns") / 1e3)
        l2.set_param("profile", 0)
        r["l2_profile_median_us"] = {key: statistics.median(v) for key, v in prof.items()}
        r["last_overflow"] = l2.get_stat("last_overflow")
        result["search"][name] = r
        print(f"{name}: " + "  ".join(
            f"{mode}: ip {r[mode]['ip']['median_ms']:.3f} ms (spread {100 * r[mode]['ip_spread']:.1f} %)  l2 {r[mode]['l2']['median_ms']:.3f} ms  "
            f"ratio {r[mode]['l2_over_ip']:.3f} (dim_pad ratio {pad_ratio:.3f})" for mode in ("eager", "ahead"))
            + f"  ids ok {r['ids_within_float32_topk']:.3f}  profile {r['l2_profile_median_us']}", flush=True)
    # ingest: 1 M x 768 float32, pageable host memory -> HBM
    stores.clear()
    del ip, l2
    dim = 768
    g = torch.Generator(device=dev).manual_seed(1)
    host = torch.cat([torch.randn((min(250_000, args.rows - lo), dim), generator=g, device=dev).cpu() for lo in range(0, args.rows, 250_000)]).numpy()
    sides = {"ip": HipFlatIndex(dim, args.rows, dtype=torch.float16, device=0),
             "l2": HipFlatIndex(dim, args.rows, dtype=torch.float16, device=0, metric="l2")}
    gbs = {s: [] for s in sides}
    for rep in range(args.ingest_repeats + 1):  # (the first repeat allocates the staging buffers: not kept)
        for s, ix in sides.items():
            ix.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.add(host)
            torch.cuda.synchronize()
            if rep:
                gbs[s].append(host.nbytes / (time.perf_counter() - t0) / 1e9)
    result["ingest"] = {"rows": args.rows, "dim": dim, "source": "float32, pageable host memory", "bytes": int(host.nbytes),
                        **{s: {"median_gbs": statistics.median(v), "min_gbs": min(v), "max_gbs": max(v)} for s, v in gbs.items()},
                        "l2_over_ip": statistics.median(gbs["l2"]) / statistics.median(gbs["ip"]),
                        "l2_saturated_rows": sides["l2"].get_stat("l2_saturated_rows")}
    print(f"ingest: ip {result['ingest']['ip']['median_gbs']:.2f} GB/s  l2 {result['ingest']['l2']['median_gbs']:.2f} GB/s", flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
