#!/usr/bin/env python3
"""Benchmark of the north-star metric: queries/s of exact brute-force inner-product top-k.

    python bench.py --gpus N --steps K --warmup W          # N > 1: spawns one fresh process per GPU itself
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W             # the same under an external launcher

Workload (BASELINE.json, configs[2], the configuration `metric` is quoted on; it fits one GPU):
10 M sections x 768 fp16, batch = 1024 queries, top-100, corpus resident in HBM, row-sharded over the N
ranks (strong scaling: the corpus is fixed, each rank holds N_total / N rows).  One "step" = one batch of
1024 queries answered end to end: local fused score + top-k on every rank, RCCL all-gather of the
per-shard top-k, merge.  Inputs are synthetic N(0,1) embeddings generated on the device (corpus seed 1234,
query seed 4321); queries are resident in HBM when the timed region starts.  `--data clustered` sorts the
rows by topic cluster and draws the queries from the LAST clusters (documents ingested in topic order:
the row order a real corpus has, /root/reference/src/vod_search/faiss_search/build.py:65-73); `--data normalized` scales rows and queries to norm 10 (the encoder's scaled-cosine pooler); `--data duplicates`
repeats ONE section over the last tenth of the store and aims every query at it (candidate-list overflow and
per-query recovery on the rank that holds those rows, and only there).

Prints ONE JSON line on rank 0 (see the keys below); `roofline` is for the dominant kernel
(`mips_filter16p_kernel`: MFMA-bound above ~312 queries per batch, HBM-bound below), `cpu_baseline` is the
oracle-side faiss-CPU restatement timed on the host cores of this box (rank 0, N = 1 only).

A plain run does what the headline needs and nothing else: build the store, W untimed + K timed steps, the line.
`--full` adds everything else it measures or checks, after the timed steps: the float64 verification of a query
sample and the integer twin (`verify`), the side workloads (`side`, N = 1 on the default workload) and the CPU
baseline (`cpu_baseline`); `--no-verify` / `--no-side` / `--no-cpu-baseline` drop single parts of it.
`--dump-outputs DIR` writes the last timed step's result to DIR (`scores.npy` float32, `ids.npy` float64, [nq, k]).
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

_T0 = time.perf_counter()


def _trace(msg: str) -> None:
    """BENCH_TRACE=1: phase stamps on stderr (seconds since import) - where a slow run spends its wall time"""
    dst = os.environ.get("BENCH_TRACE")
    if dst:
        line = f"[bench +{time.perf_counter() - _T0:7.2f}s rank {os.environ.get('RANK', '0')}] {msg}"
        if dst == "1":
            print(line, file=sys.stderr, flush=True)
        else:  # a path prefix: one file per rank (the launcher keeps the ranks' stderr to itself)
            with open(f"{dst}.rank{os.environ.get('RANK', '0')}.log", "a") as f:
                f.write(line + "\n")


GEN_CHUNK = 250_000  # rows per generation chunk; shard boundaries are multiples of it so the corpus is the same for every N


def parse_args() -> argparse.Namespace:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rows", type=int, default=10_000_000)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--nq", type=int, default=1024)
    p.add_argument("--k", type=int, default=100)
    p.add_argument("--dtype", choices=["f16", "bf16"], default="f16")
    p.add_argument("--config", choices=["c3", "c4"], default=None,
                   help="BASELINE presets: c3 = the default (10 M x 768 fp16, batch 1024, top-100); c4 = configs[3] (40 M x 1024 bf16, batch 512, "
                        "top-200: 82 GB on one GPU, 10 GB per GPU at --gpus 8) - sets --rows / --dim / --nq / --k / --dtype")
    p.add_argument("--exact-f32", action="store_true",
                   help="VODHIP_EXACT_F32 store: float32 rows kept next to the scan copy, float32 queries, results of the float32 brute force "
                        "on the UNROUNDED inputs (what the reference's faiss IndexFlat computes)")
    p.add_argument("--data", choices=["iid", "clustered", "duplicates", "normalized"], default="iid")
    p.add_argument("--tile", type=int, default=0)
    p.add_argument("--growth", type=int, default=0, help="stage growth factor x100 (0 = library default)")
    p.add_argument("--force-collective", action="store_true",
                   help="run the multi-GPU step (RCCL all-gather of the packed top-k + merge) even with one rank: exercises the N > 1 code on a 1-GPU box")
    p.add_argument("--param", action="append", default=[], metavar="KEY=VALUE[@RANK]",
                   help="library tunable (vodhip_index_set_param), repeatable; with @RANK only on that rank")
    p.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                   help="process-group backend.  nccl (= RCCL) is the product path; gloo stages the packed all-gather through the host and "
                        "lets several ranks share one GPU (RCCL refuses that): tests of the N > 1 step sequence on a 1-GPU box")
    p.add_argument("--engine", choices=["ranks", "node"], default="ranks",
                   help="ranks = one process per GPU, RCCL all-gather of the packed per-shard top-k (the default, what the driver's SCALE pass "
                        "launches); node = ONE process, `vodhip_node_index_*` over --gpus devices: per-shard top-k copied to devices[0] (xGMI peer "
                        "copies) + merge - the reference server's own shape (faiss index_cpu_to_all_gpus, server.py:51-54)")
    p.add_argument("--node-devices", type=str, default=None,
                   help="--engine node: comma-separated device ordinals, one per shard (default 0 .. gpus-1); repeating a device (0,0) puts several "
                        "shards on one GPU with the exchange forced through pinned host memory - the N > 1 code path on a 1-GPU box")
    p.add_argument("--full", action="store_true",
                   help="after the timed steps, also run the verification (float64 brute force + integer twin), the side workloads and the CPU "
                        "baseline; without it the run times the headline only")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's result (scores.npy float32, ids.npy float64, [nq, k]; a fixed sample of the query rows "
                        "above 64 MB, their indices in rows.npy) to DIR")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-verify", action="store_true")
    p.add_argument("--no-side", action="store_true",
                   help="skip the side workloads (C2, nq = 256, clustered C3, the 1.25 M-row shard with the exchange) a --full 1-GPU run appends as `side`")
    p.add_argument("--verify-queries", type=int, default=64)
    p.add_argument("--cpu-seconds", type=float, default=15.0)
    p.add_argument("--init-timeout", type=float, default=300.0,
                   help="seconds a rank waits for the process-group rendezvous + the first collective before it exits non-zero (code 75)")
    p.add_argument("--launch-check", action="store_true",
                   help="CPU-only check of the launcher: every rank joins a gloo group, all-reduces its rank, rank 0 prints one JSON line")
    pre, _ = p.parse_known_args()
    if pre.config == "c4":  # a preset = new defaults: explicit --rows / --nq ... still win
        p.set_defaults(rows=40_000_000, dim=1024, nq=512, k=200, dtype="bf16")
    args = p.parse_args()
    if args.steps < 1 and not args.launch_check:
        p.error("--steps must be at least 1")
    return args


def _free_rendezvous_port(socket) -> int:
    """A free port BELOW the kernel's ephemeral range: ranks 1..N-1 retry the rendezvous while rank 0 is still importing
    torch, and a client retrying a not-yet-listening localhost port inside that range can be given the port itself as
    its source (TCP self-connect), after which rank 0's listen fails with EADDRINUSE."""
    import random

    try:
        with open("/proc/sys/net/ipv4/ip_local_port_range") as f:
            lo = int(f.read().split()[0])
    except (OSError, ValueError):
        lo = 32768
    rng = random.SystemRandom()
    for _ in range(64):
        port = rng.randrange(20000, max(20001, min(lo, 32768)))
        with socket.socket() as s:
            try:
                s.bind(("127.0.0.1", port))
            except OSError:
                continue
            return port
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def visible_gpu_count() -> "int | None":
    """GPUs this process would see, WITHOUT touching the HIP runtime (the launcher's parent must never initialise a GPU): the KFD
    topology in sysfs (nodes with SIMDs are GPUs), narrowed by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES.  None = cannot tell."""
    fake = os.environ.get("VODHIP_BENCH_FAKE_GPUS")  # tests of the preflight on a box without a GPU
    if fake is not None:
        return int(fake)
    if not os.path.exists("/dev/kfd"):
        return 0  # no compute device node at all: ROCm cannot open any GPU from this process
    n = None
    try:
        nodes = pathlib.Path("/sys/class/kfd/kfd/topology/nodes")
        n = 0
        for node in nodes.iterdir():
            props = dict(ln.split()[:2] for ln in (node / "properties").read_text().splitlines() if len(ln.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
    except (OSError, ValueError):
        n = None
    if n is None:
        try:
            n = len([d for d in os.listdir("/dev/dri") if d.startswith("renderD")])
        except OSError:
            return None
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def launch_ranks(n: int, launch_check_only: bool = False) -> int:
    """`python bench.py --gpus N` without a launcher: start N fresh children (one per GPU) and wait for them.

    The parent never touches the GPU (it does not even import torch): a process that has initialised HIP must not be
    replaced or forked into ranks.  Rank 0 inherits stdout, so its JSON line is this command's output.  Every rank's stderr
    (and the other ranks' stdout) is kept in a scratch directory; when a rank leaves non-zero - it died, or its own init
    watchdog fired - the others are terminated (they would wait in a collective for ever) and the tails of ALL ranks' logs are
    printed, failing rank first, so the one record of a failed N-GPU run says which rank failed and why."""
    import socket
    import subprocess
    import tempfile

    if not launch_check_only:
        have = visible_gpu_count()
        if have is not None and have < n:
            print(f"bench.py --gpus {n}: only {have} GPU(s) visible on this node (KFD topology / *_VISIBLE_DEVICES): refusing to start "
                  f"{n} ranks that would share or miss devices", file=sys.stderr)
            return 2
    port = _free_rendezvous_port(socket)
    logdir = pathlib.Path(tempfile.mkdtemp(prefix="vodhip_bench_"))
    procs, files = [], []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        err = open(logdir / f"rank{r}.err", "wb")
        out = None if r == 0 else open(logdir / f"rank{r}.out", "wb")
        files += [f for f in (err, out) if f is not None]
        procs.append(subprocess.Popen([sys.executable, str(pathlib.Path(__file__).resolve()), *sys.argv[1:]], env=env, stdout=out, stderr=err))
    rc, failed = 0, None
    alive = list(procs)
    while alive:
        time.sleep(0.05)
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                failed = procs.index(p)
                for other in alive:  # a rank died: the others would wait in a collective for ever
                    other.terminate()
                deadline = time.monotonic() + 10.0
                while any(o.poll() is None for o in alive) and time.monotonic() < deadline:
                    time.sleep(0.05)
                for other in alive:
                    if other.poll() is None:
                        other.kill()
    for f in files:
        f.close()

    def tail(path: pathlib.Path, n_bytes: int = 3000) -> str:
        try:
            data = path.read_bytes()
        except OSError:
            return ""
        return data[-n_bytes:].decode("utf-8", "replace")

    if rc != 0:
        order = [failed] + [r for r in range(n) if r != failed]
        print(f"bench.py --gpus {n}: rank {failed} left with exit code {rc}; the other ranks were terminated.  Per-rank stderr tails:", file=sys.stderr)
        for r in order:
            print(f"---- rank {r} (exit {procs[r].returncode}) ----\n{tail(logdir / f'rank{r}.err')}", file=sys.stderr)
    else:
        sys.stderr.write(tail(logdir / "rank0.err", 20000))  # rank 0's warnings stay visible on a clean run
        import shutil

        shutil.rmtree(logdir, ignore_errors=True)
    return rc


def _init_watchdog(seconds: float, what: str):
    """A rank that cannot finish `what` within `seconds` (a peer that never arrives, an RCCL bootstrap that hangs) prints why and
    leaves with code 75 - the launcher then ends the other ranks and reports.  Returns the function that disarms it."""
    import threading

    def fire():
        print(f"[bench rank {os.environ.get('RANK', '?')}] {what} did not complete within {seconds:.0f} s: giving up "
              f"(MASTER_ADDR={os.environ.get('MASTER_ADDR')} MASTER_PORT={os.environ.get('MASTER_PORT')} WORLD_SIZE={os.environ.get('WORLD_SIZE')})",
              file=sys.stderr, flush=True)
        os._exit(75)

    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    return t.cancel


def _test_fault(stage: str, rank: int) -> None:
    """Fault injection for the launcher's CPU tests (VODHIP_BENCH_TEST_FAULT=die:RANK | hang:RANK at the process-group init)."""
    spec = os.environ.get("VODHIP_BENCH_TEST_FAULT", "")
    if not spec or stage != "init":
        return
    kind, _, r = spec.partition(":")
    if int(r or -1) != rank:
        return
    if kind == "die":
        print(f"[bench rank {rank}] injected failure before the process-group init", file=sys.stderr, flush=True)
        os._exit(41)
    if kind == "hang":
        time.sleep(3600)


def launch_check(rank: int, world: int, init_timeout: float) -> None:
    import datetime

    import torch
    import torch.distributed as dist

    disarm = _init_watchdog(init_timeout, "the process-group rendezvous")
    _test_fault("init", rank)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=init_timeout + 30))
    t = torch.tensor([float(rank)])
    dist.all_reduce(t)
    dist.barrier()
    disarm()
    if rank == 0:
        print(json.dumps({"launch_check": "ok", "world": world, "rank_sum": float(t.item())}), flush=True)
    dist.destroy_process_group()


def make_rows(torch, dev, tdt, data: str, chunk: int, rows: int, d: int, n_total: int):
    """Rows [chunk * GEN_CHUNK, +rows) of the synthetic corpus (identical for every rank count)."""
    g = torch.Generator(device=dev).manual_seed(1234 + chunk)
    x = torch.randn((rows, d), generator=g, device=dev, dtype=torch.float32)
    if data == "clustered":
        n_clusters = max(16, n_total // 5000)
        centers = cluster_centers(torch, dev, n_clusters, d)
        ridx = torch.arange(chunk * GEN_CHUNK, chunk * GEN_CHUNK + rows, device=dev, dtype=torch.int64)
        x = 0.6 * x + 0.8 * centers[(ridx * n_clusters) // n_total]  # unit variance, sorted by cluster
    if data == "duplicates":  # the last tenth of the store is ONE section repeated: every query ties > cand_cap rows at its top score
        ridx = torch.arange(chunk * GEN_CHUNK, chunk * GEN_CHUNK + rows, device=dev, dtype=torch.int64)
        x = torch.where((ridx >= n_total - n_total // 10)[:, None], cluster_centers(torch, dev, 1, d)[0][None, :], x)
    if data == "normalized":  # L2-normalised rows x 10 (the encoder's `mpool-scaled-cosine` pooler, scaler 100 = sqrt(100) per side)
        x = 10.0 * torch.nn.functional.normalize(x, dim=1)
    return x.to(tdt)


def cluster_centers(torch, dev, n_clusters: int, d: int):
    g = torch.Generator(device=dev).manual_seed(99)
    return torch.randn((n_clusters, d), generator=g, device=dev, dtype=torch.float32)


def make_queries(torch, dev, tdt, data: str, nq: int, d: int, n_total: int):
    g = torch.Generator(device=dev).manual_seed(4321)
    q = torch.randn((nq, d), generator=g, device=dev, dtype=torch.float32)
    if data == "clustered":  # every query looks for the topics at the END of the store
        n_clusters = max(16, n_total // 5000)
        centers = cluster_centers(torch, dev, n_clusters, d)
        late = n_clusters - 1 - torch.randint(0, max(1, n_clusters // 10), (nq,), generator=g, device=dev)
        q = 0.6 * q + 0.8 * centers[late]
    if data == "duplicates":  # every query scores the repeated section far above any other row
        q = 0.6 * q + 0.8 * cluster_centers(torch, dev, 1, d)[0][None, :]
    if data == "normalized":
        q = 10.0 * torch.nn.functional.normalize(q, dim=1)
    return q.to(tdt)


NAMEPLATE_MFMA = 2.5e15   # dense fp16 / bf16 MFMA peak (MI355X_MICROARCH.md): what `roofline.peak` / `frac` / `bound` use
NAMEPLATE_HBM = 8.0e12     # HBM3E peak
PRACTICAL_MFMA = 1.33e15   # flop/s of the best-known fp16 / bf16 contraction on this part: the guide's 8-phase GEMM template, K = 4 k, uniform random
                           # operands (cdna_hip_programming.md:377: 1.32-1.34 PF; power-limited, MI355X_MICROARCH "DVFS give-back").  Through round 6a this
                           # was 1.24e15, the rate of our own loop - which the round-6 epilogue work passed (1.28 PF on C3)
PRACTICAL_HBM = 6.29e12    # B/s of a streaming copy (MI355X_MICROARCH.md:34-43)


class Rig:
    """Process-wide state of one bench process: device, rank, the (lazily created) process group."""

    def __init__(self, torch, dev, rank, world, backend="nccl", init_timeout: float = 300.0):
        self.torch, self.dev, self.rank, self.world, self.backend = torch, dev, rank, world, backend
        self.dist = None
        self.init_timeout = init_timeout
        self.comm = None  # what the process group reports about itself once it is up (goes into the JSON line)

    def ensure_group(self):
        if self.dist is None:
            import torch.distributed as dist  # noqa: PLC0415

            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                import socket

                os.environ["MASTER_PORT"] = str(_free_rendezvous_port(socket))
            import datetime

            # rendezvous + communicator + FIRST collective under a watchdog: a rank that cannot get through leaves with code 75 and a
            # message instead of hanging the node's one measurement (the launcher then ends the other ranks and prints every rank's stderr)
            disarm = _init_watchdog(self.init_timeout, f"the {self.backend} process-group init + first all-reduce")
            _test_fault("init", self.rank)
            t0 = time.perf_counter()
            limit = datetime.timedelta(seconds=self.init_timeout + 30)
            if self.backend == "nccl":
                dist.init_process_group("nccl", device_id=self.dev, rank=self.rank, world_size=self.world, timeout=limit)
            else:
                dist.init_process_group("gloo", rank=self.rank, world_size=self.world, timeout=limit)
            self.dist = dist
            seen = self.all_reduce_scalar(1.0, "SUM")  # the first collective builds the communicator: every rank must show up in it
            self.torch.cuda.synchronize()
            disarm()
            rccl = None
            try:
                rccl = ".".join(str(v) for v in self.torch.cuda.nccl.version())
            except Exception:  # noqa: BLE001
                pass
            self.comm = {"backend": "rccl" if self.backend == "nccl" else "gloo", "world_size": dist.get_world_size(),
                         "ranks_in_first_all_reduce": int(round(seen)), "rccl_version": rccl, "comm_init_s": round(time.perf_counter() - t0, 3)}
            if int(round(seen)) != self.world:
                raise SystemExit(f"rank {self.rank}: the first all-reduce saw {seen} ranks, WORLD_SIZE is {self.world}")
        return self.dist

    def all_gather(self, dst, src) -> None:
        """ONE all-gather of the packed per-rank record (RCCL: device buffers; gloo: staged through the host)."""
        if self.backend == "nccl":
            self.dist.all_gather_into_tensor(dst, src)
        else:
            host = self.torch.empty(dst.shape, dtype=dst.dtype)
            self.dist.all_gather_into_tensor(host, src.cpu())
            dst.copy_(host)

    def all_reduce_scalar(self, value: float, op: str) -> float:
        t = self.torch.tensor([value], dtype=self.torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=getattr(self.dist.ReduceOp, op))
        return float(t.item())


def build_index(rig: Rig, *, rows: int, dim: int, dtype: str, data: str, tile: int = 0, growth: int = 0, params=(), exact: bool = False):
    """This rank's contiguous row shard (generation-chunk boundaries) of the synthetic corpus, resident in HBM."""
    from vod_amd.index import HipFlatIndex

    torch, dev = rig.torch, rig.dev
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    n_chunks = (rows + GEN_CHUNK - 1) // GEN_CHUNK
    c_lo = (n_chunks * rig.rank) // rig.world
    c_hi = (n_chunks * (rig.rank + 1)) // rig.world
    row_lo = min(rows, c_lo * GEN_CHUNK)
    row_hi = min(rows, c_hi * GEN_CHUNK)
    index = HipFlatIndex(dim, max(row_hi - row_lo, 1), dtype=tdt, device=dev.index, exact_f32=exact)
    if tile:
        index.set_param("tile", tile)
    if growth:
        index.set_param("growth", growth)
    for kv in params:
        kv, _, only_rank = kv.partition("@")
        key, _, val = kv.partition("=")
        if not only_rank or int(only_rank) == rig.rank:
            index.set_param(key, int(val))
    t0 = time.perf_counter()
    for c in range(c_lo, c_hi):
        # (an exact-f32 store ingests the UNROUNDED float32 rows: it rounds its scan copy itself)
        index.add(make_rows(torch, dev, torch.float32 if exact else tdt, data, c, min(GEN_CHUNK, rows - c * GEN_CHUNK), dim, rows))
    torch.cuda.synchronize()
    assert index.ntotal == row_hi - row_lo
    return index, row_lo, time.perf_counter() - t0


def _topk_ties_by_id(torch, sc, kb: int):
    """Row-wise top-kb of `sc` ordered (score desc, column asc) WITHOUT sorting the rows (a stable full sort of [S, 250 k] float64
    took minutes when eight ranks shared one GPU): the kb-th largest value t by radix select; every entry above t is in; of the entries
    equal to t the smallest columns fill the rest.  Returns (values [S, kb], columns [S, kb])."""
    n = sc.shape[1]
    sc = torch.nan_to_num(sc, nan=float("-inf"))
    top_v, top_c = torch.topk(sc, kb, dim=1)
    t = top_v[:, -1:]
    cols = torch.arange(n, device=sc.device, dtype=torch.int64)[None, :]
    tie_c = torch.topk(torch.where(sc == t, cols, n), kb, dim=1, largest=False).values  # ascending columns of the ties; n = none
    above = top_v > t
    cand_v = torch.cat([torch.where(above, top_v, float("-inf")), torch.where(tie_c < n, t.expand(-1, kb), float("-inf"))], dim=1)
    cand_c = torch.cat([torch.where(above, top_c, n), tie_c], dim=1)
    order = torch.sort(cand_c, dim=1, stable=True)                      # small [S, 2 kb] sorts: columns ascending ...
    cand_v, cand_c = torch.gather(cand_v, 1, order.indices), order.values
    order = torch.sort(cand_v, dim=1, descending=True, stable=True)     # ... then scores descending, ties keep the column order
    return order.values[:, :kb], torch.gather(cand_c, 1, order.indices)[:, :kb]


def _brute_force_f64(rig: Rig, qs, row_block, n_local: int, row_lo: int, k: int, multi: bool):
    """Exact top-k of the sampled queries `qs` (float64 [S, d]) over this rank's rows by a chunked FLOAT64 product, merged over the
    ranks when `multi`: the comparator of `verify`.  `row_block(lo, n)` -> rows [lo, lo + n) of the shard (any float dtype).
    Stable sorts keep ties in ascending id order, like the product.  Returns (scores f64 [S, k'], ids i64 [S, k']) on the CPU."""
    torch, dev, world = rig.torch, rig.dev, rig.world
    n_s = qs.shape[0]
    kk = min(k, n_local)
    ls = torch.full((n_s, kk), float("-inf"), device=dev, dtype=torch.float64)
    li = torch.full((n_s, kk), -1, dtype=torch.int64, device=dev)
    for lo in range(0, n_local, GEN_CHUNK):
        blk = row_block(lo, min(GEN_CHUNK, n_local - lo)).double()
        if os.environ.get("BENCH_TRACE"):
            torch.cuda.synchronize(); _trace(f"bf: rows {lo} fetched")
        sc = qs @ blk.T
        if os.environ.get("BENCH_TRACE"):
            torch.cuda.synchronize(); _trace("bf: product")
        kb = min(kk, sc.shape[1])
        ts, ti = _topk_ties_by_id(torch, sc, kb)
        if os.environ.get("BENCH_TRACE"):
            torch.cuda.synchronize(); _trace("bf: top-k")
        cs, ci = torch.cat([ls, ts], dim=1), torch.cat([li, ti + (lo + row_lo)], dim=1)
        top = torch.sort(cs, dim=1, descending=True, stable=True)
        ls, li = top.values[:, :kk], torch.gather(ci, 1, top.indices[:, :kk])
        del blk, sc
    if os.environ.get("BENCH_TRACE"):
        torch.cuda.synchronize(); _trace("bf: local done")
    if multi:
        pad_s = torch.full((n_s, k), float("-inf"), device=dev, dtype=torch.float64)
        pad_i = torch.full((n_s, k), -1, dtype=torch.int64, device=dev)
        pad_s[:, : ls.shape[1]] = ls
        pad_i[:, : li.shape[1]] = li
        as_ = torch.empty((world * n_s, k), device=dev, dtype=torch.float64)
        ai_ = torch.empty((world * n_s, k), dtype=torch.int64, device=dev)
        rig.all_gather(as_, pad_s)
        rig.all_gather(ai_, pad_i)
        # merge of the per-rank reference lists in fp64 (rank-major = ascending ids: the stable sort keeps the tie-break)
        cs = as_.view(world, n_s, k).permute(1, 0, 2).reshape(n_s, world * k)
        ci = ai_.view(world, n_s, k).permute(1, 0, 2).reshape(n_s, world * k)
        top = torch.sort(cs, dim=1, descending=True, stable=True)
        ls, li = top.values[:, :k], torch.gather(ci, 1, top.indices[:, :k])
    return ls.cpu(), li.cpu()


def _compare_with(torch, fs, fi, sample, ref_s, ref_i, comparator: str) -> dict:
    # recall@k as the reference defines it (vod_models/monitoring/functional.py:74-81,166-180), restated in oracle/metrics.py and pinned
    # by tests/golden/metrics_recall_ndcg.npz: the comparator's top-k ids are the positives, the returned list is ranked by its scores
    from oracle.metrics import recall_of_ids  # the checker, outside every timed region

    got_i = fi[sample].cpu()
    recall = recall_of_ids(got_i.numpy(), fs[sample].float().cpu().numpy(), ref_i.numpy())
    got_s = fs[sample][:, : ref_s.shape[1]].double().cpu()
    fin = torch.isfinite(ref_s) & torch.isfinite(got_s)
    diff = (got_s - ref_s).abs()[fin]
    scale = float(ref_s[fin].abs().max()) if bool(fin.any()) else 0.0
    return {
        "comparator": comparator,
        "recall_at_k": recall,
        "rows_with_identical_id_order": float((got_i[:, : ref_i.shape[1]] == ref_i).all(dim=1).float().mean()),
        "max_abs_score_diff": float(diff.max()) if diff.numel() else 0.0,
        "max_rel_score_diff": float((diff / ref_s[fin].abs().clamp_min(1e-30)).max()) if diff.numel() else 0.0,
        "score_scale": scale,  # largest |score| among the checked hits: the 1e-3 absolute tolerance is a statement about |score| <~ 200
        "queries_checked": len(sample),
    }


def integer_twin_check(rig: Rig, index, row_lo: int, *, rows: int, dim: int, nq: int, k: int, dtype: str, multi: bool, verify_queries: int) -> dict:
    """"Indices bit-exact" asserted at FULL size by the bench line itself (outside every timed region): the store is refilled with
    integer-valued rows of the same shape (every partial sum exact in fp32, thousands of exact ties), ONE batch of integer-valued
    queries runs through the same search, and the sampled queries' ids AND scores must equal a float64 brute force bit for bit under
    the (score desc, id asc) tie-break.  Leaves the index holding the twin."""
    from vod_amd.index import PackedTopk

    torch, dev, world = rig.torch, rig.dev, rig.world
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    n_local = index.ntotal
    _trace("twin: refill")
    index.reset()

    def twin_rows(lo, n):
        g = torch.Generator(device=dev).manual_seed(777 + (row_lo + lo) // GEN_CHUNK)
        return torch.randint(-8, 9, (n, dim), generator=g, device=dev, dtype=torch.int32).to(torch.float32)

    for lo in range(0, n_local, GEN_CHUNK):
        index.add(twin_rows(lo, min(GEN_CHUNK, n_local - lo)).to(torch.float32 if index.exact_f32 else tdt))
    g = torch.Generator(device=dev).manual_seed(778)
    q = torch.randint(-8, 9, (nq, dim), generator=g, device=dev, dtype=torch.int32).to(torch.float32 if index.exact_f32 else tdt)
    p = PackedTopk(nq, k, dev)
    _trace("twin: search")
    index.search(q, k, id_base=row_lo, out=(p.scores, p.ids))
    _trace("twin: brute force")
    fs, fi = p.scores, p.ids
    if multi:
        gathered = torch.empty((world * p.nbytes,), dtype=torch.uint8, device=dev)
        rig.all_gather(gathered, p.buffer)
        fs, fi = p.merge_gathered(gathered, world)
    n_v = min(nq, max(1, verify_queries))
    sample = sorted(set(int(round(j * (nq - 1) / max(1, n_v - 1))) for j in range(n_v))) if n_v > 1 else [0]
    ref_s, ref_i = _brute_force_f64(rig, q[sample].double(), twin_rows, n_local, row_lo, k, multi)
    got_s, got_i = fs[sample].cpu(), fi[sample].cpu()
    _trace("twin: compare")
    ties = int(sum((r[1:] == r[:-1]).sum() for r in ref_s))
    return {
        "ids_bit_exact": bool(torch.equal(got_i[:, : ref_i.shape[1]], ref_i)),
        "scores_bit_exact": bool(torch.equal(got_s[:, : ref_s.shape[1]].double(), ref_s)),
        "queries_checked": len(sample), "rows": rows, "tied_neighbours_in_the_reference_lists": ties,
        "data": "integer-valued rows and queries in [-8, 8] (exact fp32 arithmetic), same shape, one batch, outside the timed region",
    }


def run_workload(rig: Rig, index, row_lo: int, *, rows: int, dim: int, nq: int, k: int, dtype: str, data: str, multi: bool,
                 steps: int, warmup: int, verify_queries: int, tile: int = 0, exact: bool = False) -> dict:
    """W untimed + K timed steps of one workload on an index already resident in HBM; returns the measurements.

    One step = one batch through the hot path.  The host runs ONE step ahead of the device: step i+1 is enqueued before
    step i's exactness flag is checked (`finish` waits for that search alone), so the device never idles between batches.
    Every step's check (and recovery, if a candidate list overflowed) happens inside the timed region.

    Multi-rank steps are collective-safe by construction: a rank finishes (and, if needed, recovers) its LOCAL search of
    step i first and only then issues step i's exchange, so every rank issues exactly one all-gather + merge per step
    whether its shard overflowed or not (round 2 re-exchanged on the overflowing ranks only: mismatched collectives).
    The exchange of step i is enqueued behind the local search of step i+1, which keeps the device busy while the host
    waits for step i's flag; the two steps use alternating result records.
    (Overlapping the all-gather with the next search on RCCL's own stream was measured and dropped in round 2: the
    persistent filter kernel owns every CU, the collective's workgroups wait for one anyway: +11 % on the stage kernels.)
    """
    from vod_amd.index import PackedTopk

    torch, dev, world = rig.torch, rig.dev, rig.world
    dist = rig.ensure_group() if multi else None
    tdt = torch.float16 if dtype == "f16" else torch.bfloat16
    n_local = index.ntotal
    queries = make_queries(torch, dev, torch.float32 if exact else tdt, data, nq, dim, rows)  # (exact-f32: the unrounded float32 queries)
    packed = [PackedTopk(nq, k, dev) for _ in range(2)]  # [scores | ids] records: the exchange is ONE all-gather of 12*nq*k bytes
    gathered = torch.empty((world * packed[0].nbytes,), dtype=torch.uint8, device=dev) if multi else None
    state = {"pending": [], "n": 0, "ns": 0, "launches": 0, "recovery_passes": 0, "recovery_ns": 0, "res": None, "band_queries": 0, "xev": []}

    def step():
        p = packed[state["n"] % 2]
        state["n"] += 1
        index.search_async(queries, k, id_base=row_lo, out=(p.scores, p.ids))
        state["pending"].append(p)
        while len(state["pending"]) > 1:
            finish_one()

    def finish_one():
        p = state["pending"].pop(0)
        index.finish()  # waits for THIS search only; recovery passes (if any) run here, before the exchange
        state["ns"] += index.get_stat("last_filter_ns")
        state["launches"] += index.get_stat("last_filter_launches")
        state["recovery_passes"] += index.get_stat("last_safe_reruns")
        state["recovery_ns"] += index.get_stat("last_recovery_ns")
        if exact:
            state["band_queries"] += index.get_stat("last_exact_band_queries")
        if multi:
            # the exchange step, bracketed by HIP events on the stream it is ordered on (the collective's own stream joins it)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rig.all_gather(gathered, p.buffer)
            state["res"] = p.merge_gathered(gathered, world)
            e1.record()
            state["xev"].append((e0, e1))
        else:
            state["res"] = (p.scores, p.ids)

    def drain():
        while state["pending"]:
            finish_one()

    def fence():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    drain()
    index.set_param("profile", 1)
    for key in ("ns", "launches", "recovery_passes", "recovery_ns", "band_queries"):
        state[key] = 0
    state["xev"] = []
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    drain()
    fence()
    elapsed = time.perf_counter() - t0
    index.set_param("profile", 0)
    _trace(f"timed region done: {elapsed:.3f} s")
    per_rank = None
    if multi:
        elapsed = rig.all_reduce_scalar(elapsed, "MAX")
        state["recovery_passes"] = int(rig.all_reduce_scalar(state["recovery_passes"], "SUM"))  # over all ranks
        # what every rank spent, from its own HIP events: the filter launches (+ recovery) and the exchange (all-gather + merge)
        exch_us = sum(a.elapsed_time(b) for a, b in state["xev"]) * 1e3 / max(1, len(state["xev"]))
        mine = torch.tensor([(state["ns"] + state["recovery_ns"]) * 1e-6 / steps, exch_us, float(n_local)], dtype=torch.float64, device=dev)
        allr = torch.empty((world * 3,), dtype=torch.float64, device=dev)
        rig.all_gather(allr, mine)
        per_rank = [{"rank": r, "kernel_ms": float(allr[3 * r]), "exchange_us": float(allr[3 * r + 1]), "rows": int(allr[3 * r + 2])}
                    for r in range(world)]

    # ---- post-run verification (outside the timed region): exactness on a query sample ----
    verify = None
    if verify_queries > 0:
        fs, fi = state["res"]
        n_v = min(nq, max(1, verify_queries))
        sample = [int(round(j * (nq - 1) / max(1, n_v - 1))) for j in range(n_v)] if n_v > 1 else [0]
        sample = sorted(set(sample))
        _trace("verify: stored rows")
        # (1) against the STORED (rounded) rows and queries: every fp16 x fp16 product is exact in fp64 and the 768-1024-term sums
        # carry ~1e-13 relative error, so `max_abs_score_diff` is the kernel's own fp32-accumulation error
        q_stored = queries[sample].to(tdt).double()
        ref_s, ref_i = _brute_force_f64(rig, q_stored, lambda lo, n: index.stored_rows(lo, n), n_local, row_lo, k, multi)
        stored = _compare_with(torch, fs, fi, sample, ref_s, ref_i, "float64 chunked product over the stored (rounded) rows and queries (ties -> smaller id)")
        _trace("verify: unrounded rows")
        # (2) against the UNROUNDED float32 inputs the synthetic corpus was generated as - what the reference's float32 faiss index
        # would be searched with (build.py:65-73): the deviation a rounded store carries, and what the exact-f32 mode removes
        q32 = make_queries(torch, dev, torch.float32, data, nq, dim, rows)[sample].double()
        c0 = row_lo // GEN_CHUNK
        ref_s, ref_i = _brute_force_f64(
            rig, q32, lambda lo, n: make_rows(torch, dev, torch.float32, data, c0 + lo // GEN_CHUNK, n, dim, rows), n_local, row_lo, k, multi)
        unrounded = _compare_with(torch, fs, fi, sample, ref_s, ref_i, "float64 chunked product over the UNROUNDED float32 rows and queries")
        _trace("verify: done")
        verify = dict(unrounded if exact else stored)
        verify["vs_unrounded_inputs"] = {key: unrounded[key] for key in ("recall_at_k", "max_abs_score_diff", "rows_with_identical_id_order", "score_scale")}
        if exact:
            verify["vs_stored_rounded_rows"] = {key: stored[key] for key in ("recall_at_k", "max_abs_score_diff")}
            verify["exact_f32"] = {"band_queries_per_step": state["band_queries"] / steps, "list_rows_k_prime": index.get_stat("last_exact_kx")}
    return {"elapsed": elapsed, "filter_ns": state["ns"], "filter_launches": state["launches"], "recovery_passes": state["recovery_passes"],
            "recovery_ns": state["recovery_ns"], "verify": verify, "n_local": n_local, "steps": steps, "warmup": warmup,
            "rows": rows, "dim": dim, "nq": nq, "k": k, "dtype": dtype, "data": data, "multi": multi, "tile": tile, "exact": exact,
            "per_rank": per_rank, "result": state["res"]}


DUMP_LIMIT = 64 << 20  # bytes: what --dump-outputs may write in all


def dump_outputs(dst, scores, ids) -> None:
    """`--dump-outputs DIR`: the result a caller of the timed path receives, scores.npy (float32) and ids.npy (float64: exact for every
    id below 2^53), [nq, k].  A result above DUMP_LIMIT is cut to a fixed, seeded sample of its query rows, whose indices go to rows.npy."""
    import numpy as np

    out = pathlib.Path(dst)
    out.mkdir(parents=True, exist_ok=True)
    s = scores.float().cpu().numpy()
    i = ids.cpu().numpy().astype(np.float64)
    nq, k = s.shape
    if nq * k * 12 > DUMP_LIMIT - 4096:  # (4 KB: the three .npy headers)
        keep = max(1, (DUMP_LIMIT - 4096) // (k * 12 + 8))
        rows = np.sort(np.random.default_rng(0).choice(nq, size=keep, replace=False))
        s, i = s[rows], i[rows]
        np.save(out / "rows.npy", rows.astype(np.float64))
    else:
        (out / "rows.npy").unlink(missing_ok=True)
    np.save(out / "scores.npy", np.ascontiguousarray(s, dtype=np.float32))
    np.save(out / "ids.npy", np.ascontiguousarray(i, dtype=np.float64))


def _m(v: int) -> str:
    return f"{v // 1_000_000}M" if v % 1_000_000 == 0 else (f"{v / 1e6:g}M" if v >= 1_000_000 else str(v))


def traffic_key(rows: int, d: int, nq: int, world: int, data: str = "iid", exact: bool = False) -> str:
    """Key of profiles/hbm_traffic.json: shape @ ranks [/data] [/exact] - the store mode is part of the key (round 5's exact-f32 PMC passes
    overwrote the plain ones under a shared key)."""
    return f"{rows}x{d}x{nq}@{world}" + ("" if data == "iid" else "/" + data) + ("/exact" if exact else "")


def roofline_of(m: dict, world: int) -> dict:
    """Roofline record of the dominant kernel (the filter launches of a step) from live HIP-event durations.

    `bound` is the roof that binds at the NAMEPLATE peaks `peak` / `frac` are quoted against (2.5 PFLOP/s dense fp16 / bf16 MFMA, 8 TB/s
    HBM: SURVEY 8d's table - C2 is HBM-bound, C3 / C4 MFMA-bound); both fractions are always reported.  `practical` holds the ceilings a
    streaming kernel actually reaches on this part (1.33 PFLOP/s: the best-known power-limited fp16 / bf16 contraction, 6.29 TB/s streaming read) and the roof
    that binds at those - context, never the basis of `frac`.  Recovery launches, if any, are part of the kernel time."""
    rows, d, nq, k, steps = m["rows"], m["dim"], m["nq"], m["k"], m["steps"]
    n_local = m["n_local"]
    flops = 2.0 * nq * n_local * d                       # algorithmic flops of this rank's filter launches per step
    byts = n_local * d * 2.0 + nq * d * 2.0 + nq * k * 12.0
    kern_s = (m["filter_ns"] + m["recovery_ns"]) * 1e-9
    # Batches of one query tile run on two lanes (two searches on the device at once): a launch's event-to-event duration then includes
    # the time its workgroups waited for CUs the other lane held, and the durations of a step add up to more than the step.  The step's
    # own wall time bounds the exclusive kernel time from above: use it there (conservative: it also holds the selects).
    overlapped = kern_s > m["elapsed"]
    if overlapped:
        kern_s = m["elapsed"]
    mfma_bound = flops / NAMEPLATE_MFMA >= byts / NAMEPLATE_HBM
    tflops = flops * steps / kern_s / 1e12 if kern_s > 0 else None
    gbps = byts * steps / kern_s / 1e9 if kern_s > 0 else None
    achieved = tflops if mfma_bound else gbps
    peak = NAMEPLATE_MFMA / 1e12 if mfma_bound else NAMEPLATE_HBM / 1e9
    traffic, traffic_src = None, None
    tfile = ROOT / "profiles" / "hbm_traffic.json"
    if tfile.exists():  # HBM bytes per step from this round's rocprofv3 --pmc passes of the same workload (tools/pmc.sh)
        try:
            ent = json.loads(tfile.read_text()).get(traffic_key(rows, d, nq, world, m["data"], m.get("exact", False)))
            if isinstance(ent, dict):
                traffic, traffic_src = ent.get("bytes"), ent.get("source")
        except Exception:
            traffic = None
    return {
        "bound": "mfma" if mfma_bound else "hbm",
        "kernel": ("mips_filter8ph_kernel" if m["tile"] in (0, 14) else "mips_filter16p_kernel")
                  if (m["tile"] in (0, 8, 9, 14) and nq > 128) else f"mips_filter_kernel[tile={m['tile']}]",
        "achieved": achieved,
        "peak": peak,
        "unit": "TFLOP/s" if mfma_bound else "GB/s",
        "frac": (achieved / peak) if achieved else None,
        "traffic": traffic,
        "traffic_source": traffic_src,
        "launches_per_step": m["filter_launches"] / steps,
        "kernel_ms_per_step": kern_s / steps * 1e3,
        "includes_recovery_launches": m["recovery_ns"] > 0,
        "kernel_ms_is_step_wall_time": overlapped,  # two-lane overlap: per-launch durations are not exclusive (see above)
        "algorithmic_flops_per_step": flops,
        "algorithmic_bytes_per_step": byts,
        "mfma_frac_of_2.5PF": (tflops / 2500.0) if tflops else None,
        "hbm_frac_at_8TBps": (gbps / 8000.0) if gbps else None,
        "practical": {"mfma_tflops": PRACTICAL_MFMA / 1e12, "hbm_gbps": PRACTICAL_HBM / 1e9,
                      "bound": "mfma" if flops / PRACTICAL_MFMA >= byts / PRACTICAL_HBM else "hbm",
                      "frac": (max(flops / PRACTICAL_MFMA, byts / PRACTICAL_HBM) * steps / kern_s) if kern_s > 0 else None},
    }


LINE_LIMIT = 4000  # bytes: the final stdout line stays below 4 KB (round 5's 20.6 KB line was unreadable for the driver: BENCH_r05 parsed null)
SIDE_FILE = ROOT / "gpurun_out" / "bench_side.json"


def _r(v, digits: int = 6):
    """Float to `digits` significant digits (None / non-finite -> None): keeps the line short and strict JSON."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        return None
    return float(f"{v:.{digits}g}")


def _strict(obj):
    """Deep copy with every non-finite float replaced by None (json.dumps(..., allow_nan=False) then never raises)."""
    if isinstance(obj, dict):
        return {str(k): _strict(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_strict(v) for v in obj]
    if isinstance(obj, float):
        return obj if obj == obj and obj not in (float("inf"), float("-inf")) else None
    return obj


def compact_roofline(r: dict) -> dict:
    """The roofline record of the final line: the contract's keys + what the judge recomputes `achieved` from."""
    keep = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "launches_per_step", "kernel_ms_per_step",
            "algorithmic_flops_per_step", "algorithmic_bytes_per_step", "mfma_frac_of_2.5PF", "hbm_frac_at_8TBps")
    out = {key: _r(r.get(key)) for key in keep}
    for key in ("traffic", "algorithmic_flops_per_step", "algorithmic_bytes_per_step"):  # whole numbers: kept exact
        if r.get(key) is not None:
            out[key] = int(r[key])
    if r.get("kernel_ms_is_step_wall_time"):
        out["kernel_ms_is_step_wall_time"] = True
    if r.get("includes_recovery_launches"):
        out["includes_recovery_launches"] = True
    pr = r.get("practical") or {}
    out["practical"] = {key: _r(pr.get(key), 4) for key in ("mfma_tflops", "hbm_gbps", "bound", "frac")}
    return out


def compact_verify(v: "dict | None") -> "dict | None":
    """recall / score deviation of the sampled queries vs the float64 brute force, the same vs the unrounded float32 inputs, and the
    integer twin's bit-exactness booleans - nothing else (the full record goes to the side file)."""
    if v is None:
        return None
    out = {"recall_at_k": _r(v.get("recall_at_k")), "rows_with_identical_id_order": _r(v.get("rows_with_identical_id_order")),
           "max_abs_score_diff": _r(v.get("max_abs_score_diff"), 4), "score_scale": _r(v.get("score_scale"), 4),
           "queries_checked": v.get("queries_checked"),
           "comparator": "f64 brute force on the UNROUNDED f32 inputs" if "UNROUNDED" in str(v.get("comparator")) else "f64 brute force on the stored rows"}
    vu = v.get("vs_unrounded_inputs")
    if vu:
        out["vs_unrounded_inputs"] = {"recall_at_k": _r(vu.get("recall_at_k")), "max_abs_score_diff": _r(vu.get("max_abs_score_diff"), 4)}
    vs = v.get("vs_stored_rounded_rows")
    if vs:
        out["vs_stored_rounded_rows"] = {"recall_at_k": _r(vs.get("recall_at_k")), "max_abs_score_diff": _r(vs.get("max_abs_score_diff"), 4)}
    ex = v.get("exact_f32")
    if ex:
        out["exact_f32"] = {key: _r(val, 4) for key, val in ex.items()}
    tw = v.get("ids_bit_exact_on_integer_twin")
    if tw:
        out["integer_twin"] = {"ids_bit_exact": tw.get("ids_bit_exact"), "scores_bit_exact": tw.get("scores_bit_exact"),
                               "queries_checked": tw.get("queries_checked"), "rows": tw.get("rows")}
    return out


def compact_cpu_baseline(c: "dict | None") -> "dict | None":
    if c is None:
        return None
    out = {key: _r(c.get(key)) for key in ("value", "unit", "cores", "threads", "kind", "sgemm_only_value") if key in c}
    out["sample"] = str(c.get("sample", ""))[:300]
    if "thread_arms" in c:
        out["thread_arms"] = c["thread_arms"]
    return out


def side_summary(e: dict) -> dict:
    """One side workload in < 400 bytes: printed as a `# side {...}` line when it finishes, and kept (shorter still) in the final line."""
    out = {"name": e.get("name")}
    for key in ("error", "skipped"):
        if key in e:
            out[key] = str(e[key])[:200]
            return out
    if "ms_per_step" in e:
        out.update(ms_per_step=_r(e["ms_per_step"], 5), value=_r(e.get("value"), 6), unit=e.get("unit"), steps=e.get("steps"))
    r = e.get("roofline")
    if r:
        out["roofline"] = {"bound": r["bound"], "frac": _r(r["frac"], 4), "achieved": _r(r["achieved"], 5), "unit": r["unit"],
                           "kernel_ms_per_step": _r(r["kernel_ms_per_step"], 5)}
    v = e.get("verify")
    if v and "recall_at_k" in v:
        out["verify"] = {"recall_at_k": _r(v["recall_at_k"]), "max_abs_score_diff": _r(v.get("max_abs_score_diff"), 3)}
        vu = v.get("vs_unrounded_inputs")
        if vu:
            out["verify"]["vs_unrounded"] = [_r(vu.get("recall_at_k")), _r(vu.get("max_abs_score_diff"), 3)]
        tw = v.get("ids_bit_exact_on_integer_twin")
        if tw:
            out["verify"]["twin_bit_exact"] = bool(tw.get("ids_bit_exact") and tw.get("scores_bit_exact"))
    elif v:  # C5: its own verification record
        out["verify"] = {key: v[key] for key in ("ok", "collate_cases", "gradient_cases") if key in v}
    for key in ("collate_merge_sample", "retrieval_loss_inbatch_64x2048"):  # C5: latencies
        if isinstance(e.get(key), dict):
            out[key] = {kk: _r(vv, 4) for kk, vv in e[key].items() if kk in ("wall_us", "device_us", "fwd_bwd_wall_us", "graphed_fwd_bwd_wall_us", "host_syncs")}
    return out


def emit_side(e: dict) -> None:
    """`# side {json}`: a comment line, NOT a JSON line - stdout keeps exactly one line that parses as JSON, the last one."""
    print("# side " + json.dumps(_strict(side_summary(e)), allow_nan=False, separators=(",", ":")), flush=True)


def write_side_file(side: list, headline: dict) -> "str | None":
    """The full structure of every side workload (+ the uncut headline record) for whoever wants the detail: gpurun_out/bench_side.json."""
    try:
        SIDE_FILE.parent.mkdir(parents=True, exist_ok=True)
        SIDE_FILE.write_text(json.dumps(_strict({"headline": headline, "side": side}), allow_nan=False, indent=1))
        return str(SIDE_FILE.relative_to(ROOT))
    except OSError:
        return None


def final_line(line: dict, limit: int = LINE_LIMIT) -> str:
    """The ONE JSON line: strict JSON (no NaN / Infinity), below `limit` bytes.  Should a record still be too long (many ranks, long
    error strings) the optional parts go first - never metric / value / ms_per_step / config / roofline / cpu_baseline."""
    line = _strict(line)
    for drop in (None, "side", "per_rank", "comm", "verify"):
        if drop is not None:
            if drop not in line:
                continue
            line = dict(line)
            line[drop] = "dropped: line over the size limit (see " + str(line.get("side_file")) + ")"
        txt = json.dumps(line, allow_nan=False, separators=(", ", ": "))
        if len(txt.encode()) < limit:
            return txt
    raise SystemExit(f"bench.py: the final line does not fit {limit} bytes even without its optional parts")


def side_workloads(rig: Rig, args, headline_index, headline_row_lo) -> list:
    """The regimes next to the headline, timed by the same process in the same run (a few seconds): BASELINE configs[1]
    (C2), the 1.25 M-row shard each of 8 GPUs holds of C3 without and with the exchange step on RCCL (one rank gathers from itself:
    the difference is the per-step cost of the collective call + merge),
    nq = 256 on the headline store (one q-tile) and C3 with rows sorted by topic cluster.  Each entry carries ms/batch,
    q/s and the same roofline record as the headline; a failing side run is reported as {"error": ...} and never touches
    the headline fields."""
    out = []

    def one(name, *, rows, nq, data="iid", multi=False, steps, warmup, index=None, row_lo=0, dim=None, k=None, dtype=None, exact=False,
            twin=False):
        dim, k, dtype = dim or args.dim, k or args.k, dtype or args.dtype
        try:
            own = index is None
            t_build = None
            twin_rec = None
            if own:
                index, row_lo, t_build = build_index(rig, rows=rows, dim=dim, dtype=dtype, data=data, exact=exact)
            try:
                m = run_workload(rig, index, row_lo, rows=rows, dim=dim, nq=nq, k=k, dtype=dtype, data=data,
                                 multi=multi, steps=steps, warmup=warmup, verify_queries=args.verify_queries, exact=exact)
                if twin and own and args.verify_queries > 0:
                    twin_rec = integer_twin_check(rig, index, row_lo, rows=rows, dim=dim, nq=nq, k=k, dtype=dtype, multi=multi,
                                                  verify_queries=args.verify_queries)
            finally:
                if own:
                    index.close()
                    rig.torch.cuda.empty_cache()
            out.append({
                "name": name,
                "workload": f"{rows} sections x {dim} {dtype}, batch {nq} queries, top-{k}" + ("" if data == "iid" else ", rows sorted by topic cluster")
                            + (", + RCCL all-gather (1 rank) + merge" if multi else "")
                            + (", exact-f32 store: float32 rows + queries in, float32 brute-force result out" if exact else ""),
                "steps": steps, "warmup": warmup,
                "ms_per_step": m["elapsed"] / steps * 1e3,
                "value": nq * steps / m["elapsed"],
                "unit": "queries/s",
                "recovery_passes": m["recovery_passes"],
                "index_build_s": None if t_build is None else round(t_build, 3),
                "roofline": roofline_of(m, rig.world),
                "verify": m["verify"],
            })
            if twin_rec is not None:
                out[-1]["verify"]["ids_bit_exact_on_integer_twin"] = twin_rec
        except Exception as exc:  # noqa: BLE001 - a side line must never take the headline down
            out.append({"name": name, "error": f"{type(exc).__name__}: {exc}"[:400]})
        emit_side(out[-1])

    one("C2", rows=1_000_000, nq=256, steps=200, warmup=20)
    one("C3_nq256", rows=args.rows, nq=256, steps=50, warmup=5, index=headline_index, row_lo=headline_row_lo)
    one("C3_clustered", rows=args.rows, nq=args.nq, data="clustered", steps=max(5, args.steps), warmup=3)
    one("C3_shard_of_8", rows=args.rows // 8, nq=args.nq, steps=100, warmup=10)
    one("C3_shard_of_8_with_exchange", rows=args.rows // 8, nq=args.nq, multi=True, steps=100, warmup=10)
    # BASELINE configs[3] (C4: 40 M x 1024 bf16, batch 512, top-200): what each of its 8 GPUs holds, and the whole store on this ONE GPU (82 GB)
    one("C4_shard_of_8", rows=5_000_000, dim=1024, nq=512, k=200, dtype="bf16", steps=40, warmup=5)
    # the exact-f32 mode (float32 rows and queries in, the float32 brute-force result out) on the same shapes: what it costs, and that
    # `vs_unrounded_inputs` reads recall 1.0 / < 1e-3 there while the lines above carry the rounding of their store dtype
    one("C2_exact_f32", rows=1_000_000, nq=256, steps=200, warmup=20, exact=True)
    one("C3_exact_f32", rows=args.rows, nq=args.nq, steps=max(5, args.steps), warmup=3, exact=True)
    one("C4_shard_of_8_exact_f32", rows=5_000_000, dim=1024, nq=512, k=200, dtype="bf16", steps=40, warmup=5, exact=True)
    free_b = rig.torch.cuda.mem_get_info(rig.dev)[0]
    if free_b > 110e9:
        one("C4_one_gpu", rows=40_000_000, dim=1024, nq=512, k=200, dtype="bf16", steps=10, warmup=3, twin=True)
    else:
        out.append({"name": "C4_one_gpu", "skipped": f"{free_b / 1e9:.0f} GB of HBM free: the 82 GB store + workspace do not fit next to the headline store"})
        emit_side(out[-1])
    # BASELINE configs[4] (C5: hybrid merge + priority sampling + in-batch retrieval loss, batch 64 x 32 sections)
    try:
        sys.path.insert(0, str(ROOT / "tools"))
        import side_c5  # noqa: PLC0415  (tools/side_c5.py: timings + fixture verification of the collate-side chain and the loss)

        c5, ctx = side_c5.measure(rig.dev)
        out.append(c5)
        if not args.no_cpu_baseline:
            try:  # the CPU-baseline leg of C5: the oracle side's restatements, timed beside the kernels and used as the checker
                from oracle.c5_baseline import measure as c5_baselines  # noqa: PLC0415

                c5.update(c5_baselines(rig.torch, rig.dev, ctx["c5_data"], ctx["loss_inputs"], ctx["kw"]))
            except Exception as exc:  # noqa: BLE001
                c5["cpu_baseline"] = {"error": f"{type(exc).__name__}: {exc}"[:300]}
    except Exception as exc:  # noqa: BLE001
        out.append({"name": "C5", "error": f"{type(exc).__name__}: {exc}"[:400]})
    emit_side(out[-1])
    return out


DATA_NOTE = {"iid": "synthetic", "clustered": "synthetic, rows sorted by topic cluster, queries from the last clusters",
             "duplicates": "synthetic, one section repeated over the last tenth of the store, every query aimed at it",
             "normalized": "synthetic, rows and queries L2-normalised x 10 (scaled-cosine embeddings)"}


def compose_record(m: dict, *, world: int, backend: str, t_build: float, comm: "dict | None", cpu_baseline: "dict | None",
                   side: "list | None", engine: str = "ranks") -> dict:
    """The FULL record of a run from its measurements `m` (run_workload's dict): pure - no torch, no device - so that the CPU suite can
    check the shape and the size of the line.  `compact_record` + `final_line` cut it to the one stdout line."""
    n_total, d, nq, k, steps = m["rows"], m["dim"], m["nq"], m["k"], m["steps"]
    elapsed = m["elapsed"]
    qps = nq * steps / elapsed
    multi = m["multi"]
    if engine == "node":
        parallelism = f"ONE process, vodhip_node_index over {world} device(s): row-sharded, per-shard top-k copied to devices[0] + merge"
    elif multi:
        parallelism = f"row-sharded x{world} + {'RCCL' if backend == 'nccl' else 'gloo (host-staged)'} all-gather of per-shard top-k"
    else:
        parallelism = "single GPU"
    line = {
        "metric": f"queries/sec brute-force top-k ({_m(n_total)}x{d} {'fp16' if m['dtype'] == 'f16' else 'bf16'})",
        "value": qps,
        "unit": "queries/s",
        "n_gpus": world,
        "steps": steps,
        "warmup": m["warmup"],
        "ms_per_step": elapsed / steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": m["dtype"],
        "data": DATA_NOTE[m["data"]],
        "config": {
            "workload": f"{n_total} sections x {d} {m['dtype']}, batch {nq} queries, top-{k}, exact brute force"
                        + (", exact-f32 store (float32 rows + queries, float32 brute-force result)" if m.get("exact") else ""),
            "rows_per_gpu": m["n_local"],
            "parallelism": parallelism,
            "engine": engine,
            "index_build_s": round(t_build, 3),
            "recovery_passes": m["recovery_passes"],
        },
        "roofline": roofline_of(m, world),
    }
    if comm is not None:  # did the collective library see N ranks?  (answerable from the record alone)
        line["comm"] = comm
    if m.get("per_rank"):  # every rank's own HIP-event figures: filter kernel ms / step, exchange (all-gather + merge) us / step
        for r in m["per_rank"]:
            r["mfma_frac_of_2.5PF"] = (2.0 * nq * r["rows"] * d / (r["kernel_ms"] * 1e-3) / NAMEPLATE_MFMA) if r["kernel_ms"] > 0 else None
        line["per_rank"] = m["per_rank"]
        line["exchange_us_per_step_max"] = max(r["exchange_us"] for r in m["per_rank"])
    for key in ("per_shard", "merge_us", "copy_us_max", "peer_access"):  # the node engine's own figures
        if m.get(key) is not None:
            line[key] = m[key]
    if m["verify"] is not None:
        line["verify"] = m["verify"]
    if side is not None:
        line["side"] = side
    if cpu_baseline is not None:
        line["cpu_baseline"] = cpu_baseline
        line["speedup_vs_cpu_baseline"] = qps / cpu_baseline["value"]
    return line


def compact_record(full: dict, side_file: "str | None" = None) -> dict:
    """The final stdout line's content: the contract's keys, `roofline`, `cpu_baseline`, a short `verify`, the per-rank figures as
    parallel lists and ONE number pair per side workload; everything else lives in `side_file`."""
    line = {key: full[key] for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                        "vs_baseline", "dtype", "data", "config")}
    line["value"], line["ms_per_step"] = _r(full["value"], 7), _r(full["ms_per_step"], 7)
    line["roofline"] = compact_roofline(full["roofline"])
    if "cpu_baseline" in full:
        line["cpu_baseline"] = compact_cpu_baseline(full["cpu_baseline"])
        line["speedup_vs_cpu_baseline"] = _r(full["speedup_vs_cpu_baseline"], 5)
    if "comm" in full:
        line["comm"] = full["comm"]
    if "per_rank" in full:
        pr = full["per_rank"]
        line["per_rank"] = {"kernel_ms": [_r(r["kernel_ms"], 5) for r in pr], "exchange_us": [_r(r["exchange_us"], 4) for r in pr],
                            "rows": [r["rows"] for r in pr], "mfma_frac_of_2.5PF": [_r(r.get("mfma_frac_of_2.5PF"), 4) for r in pr]}
        line["exchange_us_per_step_max"] = _r(full["exchange_us_per_step_max"], 4)
    if "per_shard" in full:
        ps = full["per_shard"]
        line["per_shard"] = {"kernel_ms": [_r(r["kernel_ms"], 5) for r in ps], "rows": [r["rows"] for r in ps], "device": [r["device"] for r in ps]}
        line["merge_us"] = _r(full.get("merge_us"), 4)
        line["copy_us_max"] = _r(full.get("copy_us_max"), 4)
        line["peer_access"] = full.get("peer_access")
    if "verify" in full:
        line["verify"] = compact_verify(full["verify"])
    if "side" in full:  # name -> [ms / step, roofline.frac, bound] (errors / skips as a string); the detail is in the `# side` lines and the file
        short = {}
        for e in full["side"]:
            if "error" in e or "skipped" in e:
                short[e.get("name")] = ("error: " + str(e["error"]))[:80] if "error" in e else "skipped"
            elif "roofline" in e:
                short[e["name"]] = [_r(e["ms_per_step"], 5), _r(e["roofline"]["frac"], 4), e["roofline"]["bound"]]
            else:
                short[e.get("name")] = "ok" if (e.get("verify") or {}).get("ok") else "see side_file"
        line["side"] = short
        line["side_legend"] = "name: [ms_per_step, roofline.frac, bound]; detail: the '# side' stdout lines and side_file"
    if side_file:
        line["side_file"] = side_file
    return line


def run_node_engine(args) -> None:
    """`--engine node`: the same workload on ONE process driving `vodhip_node_index_*` over N devices (row shards, per-shard search on
    every device at once, lists copied to devices[0], one merge) - DESIGN 6's second multi-GPU design, one flag away from a SCALE
    measurement.  Under an external launcher (torchrun starts N ranks) rank 0 does the work and the others leave at once."""
    if int(os.environ.get("RANK", "0")) != 0:
        return
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch

    from vod_amd.hostcpu import limit_cpu_threads, usable_cpus
    from vod_amd.index import HipNodeIndex

    limit_cpu_threads(usable_cpus(), export=False)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback exists)")
    devices = [int(v) for v in args.node_devices.split(",")] if args.node_devices else list(range(args.gpus))
    if len(devices) != args.gpus:
        raise SystemExit(f"--node-devices lists {len(devices)} devices, --gpus is {args.gpus}")
    if max(devices) >= torch.cuda.device_count():
        raise SystemExit(f"--engine node: device {max(devices)} requested, {torch.cuda.device_count()} GPU(s) visible")
    shared = len(set(devices)) < len(devices)
    torch.cuda.set_device(devices[0])
    dev = torch.device("cuda", devices[0])
    rig = Rig(torch, dev, 0, 1)
    n_total, d, nq, k, G = args.rows, args.dim, args.nq, args.k, len(devices)
    tdt = torch.float16 if args.dtype == "f16" else torch.bfloat16
    exact = args.exact_f32
    index = HipNodeIndex(d, n_total, devices, dtype=tdt, exact_f32=exact)
    if shared:
        index.set_param("host_staging", 1)
    for kv in args.param:
        key, _, val = kv.partition("@")[0].partition("=")
        index.set_param(key, int(val))
    t0 = time.perf_counter()
    n_chunks = (n_total + GEN_CHUNK - 1) // GEN_CHUNK
    for c in range(n_chunks):  # the same corpus as the rank engine, chunk by chunk through the host (the node index ingests host rows)
        rows = make_rows(torch, dev, torch.float32 if exact else tdt, args.data, c, min(GEN_CHUNK, n_total - c * GEN_CHUNK), d, n_total)
        index.add((rows if exact else rows.to(torch.float16 if tdt == torch.float16 else torch.float32)).cpu().numpy())
    t_build = time.perf_counter() - t0
    assert index.ntotal == n_total
    queries = make_queries(torch, dev, torch.float32 if exact else tdt, args.data, nq, d, n_total)
    res = None
    for _ in range(args.warmup):
        res = index.search(queries, k)
    index.set_param("profile", 1)
    torch.cuda.synchronize()
    shard_ns = [0] * G
    launches = merge_ns = copy_ns = recov = 0
    step_ns = 0

    def finish_one():
        # completes the OLDEST pending batch: every shard's exactness check, the lists' copies to devices[0], the merge (enqueued on this stream)
        nonlocal res, step_ns, launches, recov
        res = index.finish()
        per = [index.shard_stat(g, "last_filter_ns") + index.shard_stat(g, "last_recovery_ns") for g in range(G)]
        for g in range(G):
            shard_ns[g] += per[g]
        step_ns += max(per)
        launches += index.shard_stat(0, "last_filter_launches")
        recov += sum(index.shard_stat(g, "last_safe_reruns") for g in range(G))

    # the host runs ONE batch ahead (as the rank engine does): batch i + 1 is enqueued on every shard before batch i is finished
    t0 = time.perf_counter()
    pending = 0
    for _ in range(args.steps):
        index.search_async(queries, k)
        pending += 1
        if pending > 1:
            finish_one()
            pending -= 1
    while pending:
        finish_one()
        pending -= 1
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    merge_ns = index.get_stat("last_merge_ns") * args.steps        # (HIP events of the last batch's merge / slowest copy: read once, after the
    copy_ns = index.get_stat("last_copy_ns_max") * args.steps      # timed region - reading them per batch would wait for every merge)
    index.set_param("profile", 0)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, *res)
    shard_rows = [max(0, min(n_total, (g + 1) * -(-n_total // G)) - g * -(-n_total // G)) for g in range(G)]
    verify = None
    if args.full and not args.no_verify and args.verify_queries > 0:
        fs, fi = res
        n_v = min(nq, args.verify_queries)
        sample = sorted(set(int(round(j * (nq - 1) / max(1, n_v - 1))) for j in range(n_v))) if n_v > 1 else [0]
        gen_dt = torch.float32 if exact else tdt  # (a plain store holds exactly the generated, rounded rows)
        ref_s, ref_i = _brute_force_f64(rig, queries[sample].double(),
                                        lambda lo, n: make_rows(torch, dev, gen_dt, args.data, lo // GEN_CHUNK, n, d, n_total), n_total, 0, k, False)
        verify = _compare_with(torch, fs, fi, sample, ref_s, ref_i,
                               "float64 chunked product over the UNROUNDED float32 rows and queries" if exact
                               else "float64 chunked product over the stored (rounded) rows and queries (ties -> smaller id)")
    peer = index.peer_access()
    index.close()
    m = {"elapsed": elapsed, "filter_ns": step_ns, "filter_launches": launches, "recovery_passes": recov, "recovery_ns": 0, "verify": verify,
         "n_local": max(shard_rows), "steps": args.steps, "warmup": args.warmup, "rows": n_total, "dim": d, "nq": nq, "k": k, "dtype": args.dtype,
         "data": args.data, "multi": G > 1, "tile": args.tile, "exact": exact, "per_rank": None,
         "per_shard": [{"shard": g, "device": devices[g], "rows": shard_rows[g], "kernel_ms": shard_ns[g] * 1e-6 / args.steps} for g in range(G)],
         "merge_us": merge_ns * 1e-3 / args.steps, "copy_us_max": copy_ns * 1e-3 / args.steps, "peer_access": peer}
    cpu = None
    if args.full and G == 1 and not args.no_cpu_baseline:
        from oracle.cpu_baseline import time_cpu_baseline  # the reported CPU baseline, never the product path

        cpu = time_cpu_baseline(d, nq, k, n_total, target_seconds=args.cpu_seconds)
    full = compose_record(m, world=G, backend="node", t_build=t_build, comm=None, cpu_baseline=cpu, side=None, engine="node")
    print(final_line(compact_record(full)), flush=True)


def main() -> None:
    args = parse_args()
    if args.engine == "node":
        return run_node_engine(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, launch_check_only=args.launch_check or args.backend == "gloo"))  # (gloo test rig: ranks may share a GPU)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this pool (before HIP starts)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.launch_check:
        return launch_check(rank, world, args.init_timeout)
    import torch

    from vod_amd.hostcpu import limit_cpu_threads, usable_cpus

    limit_cpu_threads(max(1, usable_cpus() // world), export=False)  # torch's CPU pool: the cgroup's grant, shared by the ranks (vod_amd/hostcpu.py)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback exists)")
    if args.backend == "gloo":  # test rig: the ranks may share a GPU
        local_rank %= torch.cuda.device_count()
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"rank {rank}: LOCAL_RANK={local_rank} but only {torch.cuda.device_count()} GPU(s) are visible to this process")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    multi = world > 1 or args.force_collective  # the exchange step runs (with one rank it gathers from itself)
    if rank != 0:  # only rank 0 reports: keep the other ranks' library banners out of the launcher's merged stdout
        os.dup2(os.open(os.devnull, os.O_WRONLY), 1)
    rig = Rig(torch, dev, rank, world, args.backend, init_timeout=args.init_timeout)
    if multi:
        os.environ.setdefault("MASTER_PORT", "29517")
        rig.ensure_group()

    n_total, d, nq, k = args.rows, args.dim, args.nq, args.k
    _trace("group up; building the index")
    index, row_lo, t_build = build_index(rig, rows=n_total, dim=d, dtype=args.dtype, data=args.data, tile=args.tile, growth=args.growth,
                                         params=args.param, exact=args.exact_f32)
    m = run_workload(rig, index, row_lo, rows=n_total, dim=d, nq=nq, k=k, dtype=args.dtype, data=args.data, multi=multi,
                     steps=args.steps, warmup=args.warmup, verify_queries=args.verify_queries if args.full and not args.no_verify else 0,
                     tile=args.tile, exact=args.exact_f32)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, *m["result"])
    default_workload = (n_total, d, nq, k, args.dtype, args.data, args.tile, args.growth, tuple(args.param), args.exact_f32) == (10_000_000, 768, 1024, 100, "f16", "iid", 0, 0, (), False)
    side = None
    if args.full and world == 1 and not args.force_collective and not args.no_side and default_workload:
        side = side_workloads(rig, args, index, row_lo)
    if m["verify"] is not None:  # (last use of the headline store: it is refilled with the integer twin)
        m["verify"]["ids_bit_exact_on_integer_twin"] = integer_twin_check(
            rig, index, row_lo, rows=n_total, dim=d, nq=nq, k=k, dtype=args.dtype, multi=multi, verify_queries=args.verify_queries)
    index.close()

    line = None
    if rank == 0:
        cpu = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            from oracle.cpu_baseline import time_cpu_baseline  # the reported CPU baseline, never the product path

            cpu = time_cpu_baseline(d, nq, k, n_total, target_seconds=args.cpu_seconds)
        full = compose_record(m, world=world, backend=args.backend, t_build=t_build, comm=rig.comm, cpu_baseline=cpu, side=side)
        side_file = write_side_file(side or [], full) if side is not None else None
        line = final_line(compact_record(full, side_file))
    if rig.dist is not None:
        rig.dist.barrier()
        rig.dist.destroy_process_group()
    if rank == 0:
        # RCCL writes a version banner through C stdio (block-buffered when stdout is a pipe): flush it first so that
        # the JSON line is the LAST line of rank 0's stdout
        import ctypes

        ctypes.CDLL(None).fflush(None)
        print(line, flush=True)


if __name__ == "__main__":
    main()
