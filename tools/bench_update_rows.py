#!/usr/bin/env python3
"""What does changing stored rows in place cost?  `HipFlatIndex.update_rows` / `add_to_rows` on a 1 Mi x 768 fp16 store - plain, L2 and
`exact_f32` - from a float32 device source, in one process on one device, alternating inside every repeat:
  listed SET             1 Ki and 64 Ki uniformly random unique ids (the ids already on the device);
  dense SET / dense ADD  all rows;
  re-ingest              `reset(); add(all rows)`, the only route before; on the plain store also with `set_row_values` of a 64-column
                         table behind it, which `reset` drops and `read_out(..., keys=)` needs again;
  add, equal rows        `reset(); add(m rows)` into a second, empty index for m = 1 Ki, 64 Ki: the ingest rate at equal bytes.
The byte model: dense SET on a plain store moves the bytes of `add`; on an L2 store it saves the bias launch and its re-read of the
plane; a 64 Ki-row listed SET moves 1 / 16 of the re-ingest's bytes plus 64 Ki claim atomics.
Every call here ends in a wait for its stream (`add` and the update calls from a device source synchronise before they return, `reset`
waits for the device), so a repeat is HOST-clock milliseconds around `inner` back-to-back calls, behind a device synchronise: CALL
times.  Every side is warmed first; medians with the minimum and maximum over the repeats (the run-to-run spread).  GB/s are the
algorithmic bytes of the rows written (source read + every plane written + an ADD's read of the old row) over the call time.
NOT measured here: bf16 stores, 10 M rows, kernel-only times, the node index.
usage: python tools/bench_update_rows.py [--out profiles/update_rows.json] [--rows 1048576] [--kinds plain,l2,exact]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from vod_amd.index import HipFlatIndex  # noqa: E402

dev = torch.device("cuda", 0)
DIM = 768


def call_ms(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def row_bytes(kind, dim_pad, add):
    """algorithmic bytes per row written from a float32 source"""
    b = DIM * 4 + dim_pad * 2
    if kind == "exact":
        b += dim_pad * 4 + 8
    if add:
        b += dim_pad * (4 if kind == "exact" else 2)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/update_rows.json")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--kinds", default="plain,l2,exact")
    ap.add_argument("--listed", default="1024,65536")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_update_rows.py needs the GPU: there is no CPU path to time")
    n = args.rows
    listed = [min(int(m), n) for m in args.listed.split(",")]
    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randn((n, DIM), generator=gen, device=dev)
    table = torch.randn((n, 64), generator=gen, device=dev).half()
    ids = {m: torch.randperm(n, generator=gen, device=dev)[:m].contiguous() for m in listed}
    result = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": DIM, "store": "float16", "source": "float32, device", "repeats": args.repeats,
              "window_s": args.window, "timing": "host clock around back-to-back calls that each wait for their stream",
              "not_measured": ["bf16 stores", "10 M rows", "kernel-only times", "the node index"], "stores": {}}
    for kind in args.kinds.split(","):
        kw = {"exact_f32": kind == "exact", "metric": "l2" if kind == "l2" else "inner_product"}
        with HipFlatIndex(DIM, n, dtype=torch.float16, device=0, **kw) as ix, HipFlatIndex(DIM, n, dtype=torch.float16, device=0, **kw) as side:
            ix.add(src)
            dim_pad = ix.get_stat("dim_pad")

            def reingest():
                ix.reset()
                ix.add(src)

            def reingest_with_table():
                reingest()
                ix.set_row_values(table)

            def add_rows(m):
                def run():
                    side.reset()
                    side.add(src[:m])
                return run

            sides = {"reingest": reingest, "dense_set": lambda: ix.update_rows(src), "dense_add": lambda: ix.add_to_rows(src, alpha=-0.01)}
            if kind == "plain":
                sides["reingest_with_table"] = reingest_with_table
            for m in listed:
                sides[f"listed_set_{m}"] = (lambda m: lambda: ix.update_rows(src[:m], ids=ids[m]))(m)
                sides[f"add_{m}_rows"] = add_rows(m)
            inner = {}
            for name, fn in sides.items():
                for _ in range(args.warmup):
                    fn()
                inner[name] = max(1, int(args.window * 1e3 / max(call_ms(fn, 2), 1e-3)) + 1)
            ms = {name: [] for name in sides}
            for _ in range(args.repeats):
                for name, fn in sides.items():  # alternating: every repeat times every side once
                    ms[name].append(call_ms(fn, inner[name]))
            assert ix.ntotal == n  # (every side leaves the store full)
            r = {name: summary(v) for name, v in ms.items()}
            spread = lambda *names: max(r[k]["max_ms"] - r[k]["min_ms"] for k in names)  # noqa: E731
            gbs = lambda name, rows, add=False: rows * row_bytes(kind, dim_pad, add) / (r[name]["median_ms"] * 1e-3) / 1e9  # noqa: E731
            re = r["reingest"]["median_ms"]
            store = {"dim_pad": dim_pad, "inner": inner, "sides": r,
                     "bytes_per_row": {"set": row_bytes(kind, dim_pad, False), "add": row_bytes(kind, dim_pad, True)},
                     "gb_per_s": {"reingest": gbs("reingest", n), "dense_set": gbs("dense_set", n), "dense_add": gbs("dense_add", n, True)},
                     "dense_set_over_reingest": r["dense_set"]["median_ms"] / re, "dense_add_over_reingest": r["dense_add"]["median_ms"] / re,
                     "spread_dense_set_vs_reingest_ms": spread("dense_set", "reingest"),
                     "dense_set_no_slower_than_reingest": r["dense_set"]["median_ms"] <= re + spread("dense_set", "reingest"),
                     "dense_set_faster_than_reingest_by_more_than_the_spread": r["dense_set"]["median_ms"] + spread("dense_set", "reingest") < re,
                     "listed": {}}
            print(f"{kind}: re-ingest {re:.3f} ms [{r['reingest']['min_ms']:.3f}, {r['reingest']['max_ms']:.3f}] ({store['gb_per_s']['reingest']:.0f} GB/s)  "
                  f"dense SET {r['dense_set']['median_ms']:.3f} ms [{r['dense_set']['min_ms']:.3f}, {r['dense_set']['max_ms']:.3f}] x{store['dense_set_over_reingest']:.2f} "
                  f"({store['gb_per_s']['dense_set']:.0f} GB/s)  dense ADD {r['dense_add']['median_ms']:.3f} ms [{r['dense_add']['min_ms']:.3f}, "
                  f"{r['dense_add']['max_ms']:.3f}] x{store['dense_add_over_reingest']:.2f} ({store['gb_per_s']['dense_add']:.0f} GB/s)", flush=True)
            if kind == "plain":
                rt = r["reingest_with_table"]["median_ms"]
                store["dense_set_over_reingest_with_table"] = r["dense_set"]["median_ms"] / rt
                print(f"{kind}: re-ingest + set_row_values(64 columns) {rt:.3f} ms [{r['reingest_with_table']['min_ms']:.3f}, {r['reingest_with_table']['max_ms']:.3f}]  "
                      f"dense SET x{store['dense_set_over_reingest_with_table']:.2f} of it", flush=True)
            for m in listed:
                ls, ad = r[f"listed_set_{m}"], r[f"add_{m}_rows"]
                sp = spread(f"listed_set_{m}", "reingest")
                store["gb_per_s"][f"listed_set_{m}"] = gbs(f"listed_set_{m}", m)
                store["gb_per_s"][f"add_{m}_rows"] = gbs(f"add_{m}_rows", m)
                store["listed"][str(m)] = {"rows": m, "reingest_over_listed_set": re / ls["median_ms"], "listed_set_over_add_of_equal_rows": ls["median_ms"] / ad["median_ms"],
                                           "spread_vs_reingest_ms": sp, "faster_than_reingest_by_more_than_the_spread": ls["median_ms"] + sp < re}
                print(f"{kind}: listed SET {m}: {ls['median_ms']:.4f} ms [{ls['min_ms']:.4f}, {ls['max_ms']:.4f}] ({store['gb_per_s'][f'listed_set_{m}']:.0f} GB/s)  "
                      f"re-ingest / it = {re / ls['median_ms']:.1f} x (spread {sp:.3f} ms)  add of {m} rows {ad['median_ms']:.4f} ms [{ad['min_ms']:.4f}, {ad['max_ms']:.4f}]  "
                      f"{'faster than the re-ingest' if store['listed'][str(m)]['faster_than_reingest_by_more_than_the_spread'] else 'NOT faster than the re-ingest'}", flush=True)
            result["stores"][kind] = store
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
