#!/usr/bin/env python3
"""What does removing stored rows in place cost?  `HipFlatIndex.remove_rows` on a 1 Mi x 768 fp16 store - plain (with a 64-column
value table attached), L2 and `exact_f32` - in one process on one device.  Cases:
  random_1024      1 Ki uniformly random rows (the ids already on the device);
  random_1pct      1 % uniformly random rows;
  row_0            row 0 alone: everything shifts by one, every slab is bounced (its bytes move twice);
  last_10pct       the last 10 % by the range form: nothing moves;
  every_other      every other row: after the first slabs every slab is direct (its bytes move once).
Each case is timed against the only route there was before: `reset(); add(survivors)` from a float32 device tensor - plus
`set_row_values(survivors' table)` on the plain store, whose table `reset` drops.  A removal shrinks the store, so the store is
rebuilt (untimed) before every timed removal; a timed call is ONE call on the host clock between two device synchronisations.  The two
sides alternate inside every repeat; medians with the minimum and maximum over the repeats, and the spread (the larger max - min of the
two sides) beside every ratio.  No time here is a pass condition.
NOT measured here: bf16 stores, 10 M rows, kernel-only times, other slab sizes, the node index.
usage: python tools/bench_remove_rows.py [--out profiles/remove_rows.json] [--rows 1048576] [--kinds plain,l2,exact]"""
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


def once_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/remove_rows.json")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--kinds", default="plain,l2,exact")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_remove_rows.py needs the GPU: there is no CPU path to time")
    n = args.rows
    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randn((n, DIM), generator=gen, device=dev)
    table = torch.randn((n, 64), generator=gen, device=dev).half()
    perm = torch.randperm(n, generator=gen, device=dev)
    cases = {
        "random_1024": {"ids": perm[: min(1024, n)].contiguous()},
        "random_1pct": {"ids": perm[: max(1, n // 100)].contiguous()},
        "row_0": {"ids": torch.zeros(1, dtype=torch.int64, device=dev)},
        "last_10pct": {"begin": n - n // 10, "n": n // 10},
        "every_other": {"ids": torch.arange(0, n, 2, device=dev)},
    }
    result = {"device": torch.cuda.get_device_name(0), "rows": n, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "timing": "host clock around ONE call between two device synchronisations; the store is rebuilt, untimed, before every timed removal",
              "not_measured": ["bf16 stores", "10 M rows", "kernel-only times", "other slab sizes", "the node index"], "stores": {}}
    for kind in args.kinds.split(","):
        kw = {"exact_f32": kind == "exact", "metric": "l2" if kind == "l2" else "inner_product"}
        with HipFlatIndex(DIM, n, dtype=torch.float16, device=0, **kw) as ix, HipFlatIndex(DIM, n, dtype=torch.float16, device=0, **kw) as side:
            with_table = kind == "plain"

            def rebuild():
                ix.reset()
                ix.add(src)
                if with_table:
                    ix.set_row_values(table)

            store = {"slab_rows": None, "value_table_columns": 64 if with_table else 0, "cases": {}}
            rebuild()
            store["slab_rows"] = ix.get_stat("remove_slab_rows")
            for name, kwargs in cases.items():
                keep = torch.ones(n, dtype=torch.bool, device=dev)
                if "ids" in kwargs:
                    keep[kwargs["ids"]] = False
                else:
                    keep[kwargs["begin"]: kwargs["begin"] + kwargs["n"]] = False
                survivors, survivors_table = src[keep].contiguous(), table[keep].contiguous()
                removed = n - survivors.shape[0]

                def remove():
                    got = ix.remove_rows(**kwargs)
                    assert got == removed

                def reingest():
                    side.reset()
                    side.add(survivors)
                    if with_table:
                        side.set_row_values(survivors_table)

                for _ in range(args.warmup):
                    rebuild()
                    remove()
                    reingest()
                ms = {"remove_rows": [], "reingest": []}
                for _ in range(args.repeats):  # alternating: every repeat times both sides once
                    rebuild()
                    ms["remove_rows"].append(once_ms(remove))
                    ms["reingest"].append(once_ms(reingest))
                assert ix.ntotal == side.ntotal == n - removed
                r = {k: summary(v) for k, v in ms.items()}
                spread = max(r[k]["max_ms"] - r[k]["min_ms"] for k in r)
                rm, re = r["remove_rows"]["median_ms"], r["reingest"]["median_ms"]
                store["cases"][name] = {"removed": removed, "sides": r, "remove_over_reingest": rm / re, "spread_ms": spread,
                                        "faster_than_reingest_by_more_than_the_spread": rm + spread < re,
                                        "slower_than_reingest_by_more_than_the_spread": rm > re + spread}
                print(f"{kind} {name}: remove_rows {rm:.3f} ms [{r['remove_rows']['min_ms']:.3f}, {r['remove_rows']['max_ms']:.3f}]  "
                      f"re-ingest of the survivors {re:.3f} ms [{r['reingest']['min_ms']:.3f}, {r['reingest']['max_ms']:.3f}]  "
                      f"x{rm / re:.2f} (spread {spread:.3f} ms)", flush=True)
                del survivors, survivors_table
            result["stores"][kind] = store
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
