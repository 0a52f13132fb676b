#!/usr/bin/env python3
"""What does an exact rank cost?  `HipFlatIndex.rank_ids` over a 1 M x 768 fp16 store at nq 256 and 1024 with 1, 8 and 64 listed rows per
query, in one process on one device.  Two kinds of targets:
  search   well ranked: the first m hits of `search(q, 64)` - most tiles count nothing above them;
  random   uniformly random rows: they sit near the median rank, so every tile holds a nonzero count for every slot - the worst case
           for the count traffic (one integer atomic per tile, query and slot).
Alternating inside every repeat with three yardsticks of the same batch:
  log_partition  the same scan with the exponential epilogue;
  search         `index.search(q, 100)`;
  torch          what a user would write today: chunks of the stored rows, `((q16 @ x_chunk.T).float() > s).sum()` per slot (m = 1) - it
                 materialises an nq x chunk score block per chunk and has no tie rule.
And the split of a call (m = 1, 8, 64, random targets): `pick` = stage + resolve + gather + the mini-store product
(`vodhip_index_scan_score_ids`), `count` = stage + prep + the scan + finish (`count_above` against the picked scores).
Every side is warmed at every shape; a repeat is device milliseconds between two events around `inner` back-to-back calls, `inner`
sized from the warm-up so that a window lasts at least `--window` seconds; medians with the minimum and maximum over the repeats.  CALL
times on the current stream, not kernel times.
usage: python tools/bench_rank_ids.py [--out profiles/rank_ids.json] [--rows 1000000]"""
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
SLOTS = (1, 8, 64)
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


def torch_count(q16, x, s, chunk):
    acc = torch.zeros_like(s, dtype=torch.int64)
    for lo in range(0, x.shape[0], chunk):
        acc += ((q16 @ x[lo : lo + chunk].T).float() > s).sum(dim=1, keepdim=True)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/rank_ids.json")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072, help="rows per chunk of the torch sequence")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rank_ids.py needs the GPU: there is no CPU path to time")

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
        top_s, top_i = ix.search(q, 64)
        rand_i = torch.randint(0, args.rows, (nq, 64), generator=g, device=dev)
        targets = {"search": top_i, "random": rand_i}
        sides, check = {}, {}
        for kind, ids in targets.items():
            for m in SLOTS:
                lst = ids[:, :m].contiguous()
                sides[f"rank_ids_{kind}_m{m}"] = lambda lst=lst: ix.rank_ids(q, lst)
        # the split of a call on random targets
        stream = _native.current_stream_ptr(0)
        for m in SLOTS:
            lst = rand_i[:, :m].contiguous()
            picked = ix.rank_ids(q, lst).score
            scratch = torch.empty_like(picked)
            sides[f"pick_random_m{m}"] = lambda lst=lst, scratch=scratch, m=m: _native.check(lib.vodhip_index_scan_score_ids(
                ix._h, ctypes.c_void_p(q.data_ptr()), 2, nq, ctypes.c_void_p(lst.data_ptr()), m, 0, None, 0, ctypes.c_void_p(scratch.data_ptr()), None,
                stream))
            sides[f"count_random_m{m}"] = lambda lst=lst, picked=picked: ix.count_above(q, picked, tie_ids=lst)
        one = rand_i[:, :1].contiguous()
        s_one = ix.rank_ids(q, one).score
        sides["log_partition"] = lambda: ix.log_partition(q, temperature=1.0 / beta)
        sides["search"] = lambda: ix.search(q, 100)
        sides["torch"] = lambda: torch_count(q16, x, s_one, args.chunk)
        # what is timed is what is right: the search's hits at their positions, count == rank, torch's strict count within the ties
        r = ix.rank_ids(q, top_i)
        check["search_hits_at_their_positions"] = bool(torch.equal(r.rank, torch.arange(64, device=dev).expand(nq, 64)))
        check["search_hits_same_score_bits"] = bool(torch.equal(r.score.view(torch.int32), top_s.view(torch.int32)))
        rr = ix.rank_ids(q, rand_i)
        check["count_above_equals_rank"] = bool(torch.equal(ix.count_above(q, rr.score, tie_ids=rand_i), rr.rank))
        check["random_median_rank"] = float(rr.rank.double().median())
        check["torch_strict_count_max_abs_diff"] = int((torch_count(q16, x, s_one, args.chunk) - ix.count_above(q, s_one)).abs().max())
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
        derived = {"nq": nq, "inner": inner, "check": check}
        for kind in targets:
            derived[f"slope_ms_per_slot_{kind}"] = (med(f"rank_ids_{kind}_m64") - med(f"rank_ids_{kind}_m1")) / 63.0
            derived[f"m1_{kind}_over_log_partition"] = med(f"rank_ids_{kind}_m1") / med("log_partition")
            derived[f"m1_{kind}_over_search"] = med(f"rank_ids_{kind}_m1") / med("search")
        for m in SLOTS:
            derived[f"random_over_search_targets_m{m}"] = med(f"rank_ids_random_m{m}") / med(f"rank_ids_search_m{m}")
        derived["torch_over_m1_random"] = med("torch") / med("rank_ids_random_m1")
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
