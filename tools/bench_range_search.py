#!/usr/bin/env python3
"""What does it cost to NAME the rows above a threshold?  `HipFlatIndex.range_search` over a 1 M x 768 fp16 store at nq 256 and 1024, in one
process on one device, with three kinds of per-query thresholds:
  hit10     the score of the search's hit 10: ten rows per query, almost every emit workgroup leaves before its K loop;
  hit1000   the score of the search's hit 1000;
  random    the score of a uniformly random row: about half the store per query - every tile holds hits, the emit scan skips nothing and
            the result is gigabytes.
Alternating inside every repeat, per kind:
  sizing        the native sizing call (count scan + prefix: lims alone, no outputs);
  full          `range_search(q, t, max_results=total)`: one native call, count scan + prefix + emit scan, outputs allocated per call;
  count_above   `count_above(q, t)` with one slot: the scan whose count the lists must match - the sizing call's yardstick (target: sizing
                within 1.15 x of it);
  torch         what a user would write today: chunks of the stored rows, `((q16 @ x_chunk.T) > t).nonzero()` and the gather of the scores -
                it materialises an nq x chunk score block per chunk, rounds the scores to fp16 and has no tie rule;
and `log_partition` of the same batch.  Every side is warmed at every shape; a repeat is device milliseconds between two events around
`inner` back-to-back calls, `inner` sized from the warm-up so that a window lasts at least `--window` seconds; medians with the minimum and
maximum over the repeats.  CALL times on the current stream, not kernel times (the full call waits for its stream to report overflow).
usage: python tools/bench_range_search.py [--out profiles/range_search.json] [--rows 1000000]"""
import argparse
import ctypes
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
from vod_amd import _native  # noqa: E402
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


def torch_range(q16, x, t16, chunk):
    """(queries, rows, scores) of every pair above the threshold, chunk by chunk"""
    qs, zs, ss = [], [], []
    for lo in range(0, x.shape[0], chunk):
        block = q16 @ x[lo : lo + chunk].T
        hit = (block > t16).nonzero()
        qs.append(hit[:, 0])
        zs.append(hit[:, 1] + lo)
        ss.append(block[hit[:, 0], hit[:, 1]])
    return torch.cat(qs), torch.cat(zs), torch.cat(ss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/range_search.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_range_search.py needs the GPU: there is no CPU path to time")

    lib = _native.load_library()
    ix = HipFlatIndex(DIM, args.rows, dtype=torch.float16, device=0)
    g = torch.Generator(device=dev).manual_seed(0)
    for lo in range(0, args.rows, 250_000):
        ix.add(torch.randn((min(250_000, args.rows - lo), DIM), generator=g, device=dev).half())
    x = ix.stored_rows()  # the yardstick reads the very rows the kernel reads
    beta = float(torch.tensor(DIM ** -0.5, dtype=torch.float32))
    result = {"device": torch.cuda.get_device_name(0), "rows": args.rows, "dim": DIM, "store": "float16", "repeats": args.repeats,
              "window_s": args.window, "torch_chunk_rows": args.chunk, "shapes": {}}
    for nq in BATCHES:
        q = torch.randn((nq, DIM), generator=g, device=dev)
        q16 = q.half()
        depth = min(1000, args.rows)
        top_s, _ = ix.search(q, depth)
        rand_i = torch.randint(0, args.rows, (nq, 1), generator=g, device=dev)
        thresholds = {"hit10": top_s[:, min(10, depth) - 1].contiguous(), "hit1000": top_s[:, depth - 1].contiguous(),
                      "random": ix.rank_ids(q, rand_i).score[:, 0].contiguous()}
        stream = _native.current_stream_ptr(0)
        sides, check, stats = {}, {}, {}
        for kind, t in thresholds.items():
            lims = torch.empty((nq + 1,), dtype=torch.int64, device=dev)
            sides[f"sizing_{kind}"] = lambda t=t, lims=lims: _native.check(lib.vodhip_index_range_search(
                ix._h, ctypes.c_void_p(q.data_ptr()), 2, nq, ctypes.c_void_p(t.data_ptr()), None, 0, None, 0, ctypes.c_void_p(lims.data_ptr()), None, None, 0,
                stream))
            res = ix.range_search(q, t)
            total = int(res.lims[-1])
            skipped, groups = ix.get_stat("last_range_emit_skipped"), ix.get_stat("last_range_emit_groups")
            counts = ix.count_above(q, t[:, None])[:, 0]
            check[f"{kind}_lengths_equal_count_above"] = bool(torch.equal(res.lims[1:] - res.lims[:-1], counts))
            check[f"{kind}_selfcheck"] = ix.get_stat("last_range_selfcheck")
            tq, tz, ts = torch_range(q16, x, t.half()[:, None], args.chunk)
            stats[kind] = {"total_rows": total, "rows_per_query": total / nq, "result_bytes": total * 12, "emit_groups": groups,
                           "emit_groups_skipped": skipped, "emit_skipped_share": skipped / max(groups, 1),
                           "torch_total_rows": int(tq.numel())}  # (fp16 scores against an fp16 threshold: near the kernel's count, not equal)
            del res, tq, tz, ts
            sides[f"full_{kind}"] = lambda t=t, total=total: ix.range_search(q, t, max_results=total)
            sides[f"count_above_{kind}"] = lambda t=t: ix.count_above(q, t[:, None])
            sides[f"torch_{kind}"] = lambda t=t: torch_range(q16, x, t.half()[:, None], args.chunk)
        sides["log_partition"] = lambda: ix.log_partition(q, temperature=1.0 / beta)
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
        res = {name: summary(v) for name, v in ms.items()}
        med = lambda name: res[name]["median_ms"]  # noqa: E731
        derived = {"nq": nq, "inner": inner, "check": check, "results": stats}
        for kind in thresholds:
            derived[f"sizing_over_count_above_{kind}"] = med(f"sizing_{kind}") / med(f"count_above_{kind}")
            derived[f"full_over_sizing_{kind}"] = med(f"full_{kind}") / med(f"sizing_{kind}")
            derived[f"torch_over_full_{kind}"] = med(f"torch_{kind}") / med(f"full_{kind}")
            derived[f"sizing_over_log_partition_{kind}"] = med(f"sizing_{kind}") / med("log_partition")
        res.update(derived)
        result["shapes"][f"nq{nq}"] = res
        print(f"nq {nq}: " + "  ".join(f"{name} {res[name]['median_ms']:.3f} [{res[name]['min_ms']:.3f}, {res[name]['max_ms']:.3f}]" for name in sides),
              flush=True)
        print(f"nq {nq}: " + json.dumps({k: v for k, v in derived.items() if k != "inner"}), flush=True)
    out_path = pathlib.Path(args.out)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
