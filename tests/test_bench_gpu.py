"""bench.py contract on the GPU box: ONE JSON line, last on stdout, with the fields the driver reads - for the plain
single-GPU step and for the multi-GPU step (RCCL all-gather of the packed per-shard top-k + merge), which
`--force-collective` runs with a single rank so that the N > 1 code is exercised on a 1-GPU machine."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"}


def _strict_loads(txt):
    def refuse(const):
        raise AssertionError(f"non-strict JSON constant {const} in the bench line")

    return json.loads(txt, parse_constant=refuse)


def _run(*extra):
    """A `--full` run (verify, CPU baseline) of a small store."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--rows", "300000", "--nq", "1024", "--steps", "3", "--warmup", "1", *extra],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines[-1].encode()) < 4096, len(lines[-1])
    line = _strict_loads(lines[-1])  # the JSON line is the last line of stdout, whatever the libraries printed before
    assert REQUIRED <= set(line), REQUIRED - set(line)
    assert sum(ln.lstrip().startswith("{") for ln in lines) == 1
    return line


def test_single_gpu_line_with_roofline_and_cpu_baseline():
    line = _run("--cpu-seconds", "2")
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["value"] > 0 and line["vs_baseline"] is None
    assert set(line["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    assert set(line["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    assert line["verify"]["recall_at_k"] == 1.0


def test_multi_gpu_step_runs_with_one_rank():
    line = _run("--force-collective", "--no-cpu-baseline")
    assert "all-gather" in line["config"]["parallelism"]
    assert line["verify"]["recall_at_k"] == 1.0


def test_plain_run_times_the_headline_only_and_dumps_its_result(tmp_path):
    """Without `--full` the line carries the headline alone (no verify / side / CPU baseline), and `--dump-outputs` writes the last timed
    step's result: the top-k of the synthetic store, checked here against a float64 product over the same generated rows and queries."""
    import importlib.util

    import numpy as np
    import torch

    n, d, nq, k = 300_000, 128, 64, 10
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29535")
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--rows", str(n), "--dim", str(d), "--nq", str(nq), "--k", str(k), "--steps", "4",
                          "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    line = _strict_loads(lines[-1])
    assert REQUIRED <= set(line) and line["steps"] == 4 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"verify", "side", "cpu_baseline", "side_file"} & set(line), set(line)
    s = np.load(tmp_path / "dump" / "scores.npy")
    i = np.load(tmp_path / "dump" / "ids.npy")
    assert s.dtype == np.float32 and i.dtype == np.float64 and s.shape == i.shape == (nq, k)
    assert not (tmp_path / "dump" / "rows.npy").exists()
    assert np.all(np.diff(s, axis=1) <= 0) and np.all((i >= 0) & (i < n) & (i == np.round(i)))

    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    dev = torch.device("cuda", 0)
    x = torch.cat([bench.make_rows(torch, dev, torch.float16, "iid", c, min(bench.GEN_CHUNK, n - c * bench.GEN_CHUNK), d, n)
                   for c in range(-(-n // bench.GEN_CHUNK))]).double()
    q = bench.make_queries(torch, dev, torch.float16, "iid", nq, d, n).double()
    sc = q @ x.T
    kth = torch.topk(sc, k, dim=1).values[:, -1].cpu().numpy()
    at_ids = sc.gather(1, torch.from_numpy(i.astype(np.int64)).to(dev)).cpu().numpy()
    assert np.abs(at_ids - s).max() < 1e-3           # every returned score is its row's score ...
    assert np.all(s[:, -1] >= kth - 1e-3)            # ... and the rows are the top k


def test_sharded_index_exchange_on_rccl_with_one_rank(tmp_path):
    """`ShardedFlatIndex`'s native path (HIP search -> ONE packed RCCL all-gather -> HIP merge) on a real RCCL
    communicator; a single rank gathers from itself, so the result must equal the plain search."""
    script = tmp_path / "one_rank.py"
    script.write_text(f"""
import sys
import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, {str(ROOT)!r})
from vod_amd.distributed import ShardedFlatIndex
from vod_amd.index import HipFlatIndex

torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
rng = np.random.default_rng(0)
x = rng.integers(-8, 9, size=(50000, 96)).astype(np.float16)
q = rng.integers(-8, 9, size=(300, 96)).astype(np.float16)
ix = HipFlatIndex(96, 50000)
ix.add(x)
tq = torch.from_numpy(q).cuda()
s0, i0 = ix.search(tq, 50, id_base=7000)
sh = ShardedFlatIndex(ix, row_offset=7000, always_exchange=True)
for _ in range(3):
    s1, i1 = sh.search(tq, 50)
assert torch.equal(s0, s1) and torch.equal(i0, i1)
dist.destroy_process_group()
print("sharded exchange ok")
""")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "sharded exchange ok" in out.stdout


def test_sharded_index_two_ranks_on_one_gpu(tmp_path):
    """world_size 2 on real kernels: two processes share the box's GPU, each holds one row shard in its own HIP context and
    runs `ShardedFlatIndex`'s native path (fused HIP search with the shard's id offset -> ONE packed all-gather -> HIP
    merge).  RCCL refuses two ranks on one device, so the group is gloo and the exchange is staged through the host
    (`ShardedFlatIndex._all_gather`); everything else is the multi-GPU code.  Both ranks must hold the oracle's answer
    for the WHOLE store, ties across the shard boundary included (integer-valued rows)."""
    script = tmp_path / "two_ranks.py"
    script.write_text(f"""
import os
import sys
import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, {str(ROOT)!r})
from oracle.flat_ip import flat_ip_topk
from vod_amd.distributed import ShardedFlatIndex, shard_bounds
from vod_amd.index import HipFlatIndex

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
rng = np.random.default_rng(3)
n, d, nq = 90001, 160, 260
x = rng.integers(-5, 6, size=(n, d)).astype(np.float16)
q = rng.integers(-5, 6, size=(nq, d)).astype(np.float16)
bounds = shard_bounds(n, world, align=256)
lo, hi = bounds[rank], bounds[rank + 1]
ix = HipFlatIndex(d, hi - lo)
ix.add(x[lo:hi])
sh = ShardedFlatIndex(ix, row_offset=lo)
tq = torch.from_numpy(q).cuda()
for k in (100, 7, 300):
    s, i = sh.search(tq, k)
    rs, ri = flat_ip_topk(q.astype(np.float32), x.astype(np.float32), k)
    assert np.array_equal(i.cpu().numpy(), ri), (rank, k)
    assert np.array_equal(s.cpu().numpy(), rs), (rank, k)
    assert (ri >= hi if rank == 0 else ri < lo).any(), "the answer must draw on the OTHER rank's shard"
dist.barrier()
dist.destroy_process_group()
print(f"rank {{rank}} ok", flush=True)
""")
    port = "29547"
    procs = [subprocess.Popen([sys.executable, str(script)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(r), WORLD_SIZE="2"))
             for r in range(2)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err[-2000:]
        assert f"rank {r} ok" in out


def _run_bench(*args, timeout=900):
    """`bench.py --full <args>`: the record with `verify` (and, on the default workload, `side` and `cpu_baseline`)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=str(ROOT))
    assert out.returncode == 0, (out.stderr[-3000:], out.stdout[-1000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.lstrip().startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]   # exactly ONE line of stdout parses as JSON ...
    assert out.stdout.rstrip().splitlines()[-1] == lines[0] and len(lines[0].encode()) < 4096, len(lines[0])  # ... the last one, below 4 KB
    rec = _strict_loads(lines[0])
    rec["_side_lines"] = [_strict_loads(ln[len("# side "):]) for ln in out.stdout.splitlines() if ln.startswith("# side ")]
    return rec


def test_bench_two_ranks_only_one_shard_overflows_stays_collective_safe():
    """Round-2 advisor / verdict finding: a rank whose candidate lists overflowed issued one more all-gather than its peers.
    `--data duplicates` puts > cand_cap tied rows at the top of every query on the LAST rank's shard only; both ranks must
    still issue one exchange per step (no hang), the recovered result must be the exact answer under the tie-break
    (smaller id first among 50 k equal scores), and the recovery launches must be part of the reported kernel time."""
    rec = _run_bench("--gpus", "2", "--backend", "gloo", "--rows", "500000", "--dim", "128", "--nq", "300", "--k", "50", "--steps", "4",
                     "--warmup", "1", "--data", "duplicates", "--no-cpu-baseline", "--verify-queries", "64")
    assert rec["n_gpus"] == 2 and rec["config"]["recovery_passes"] >= 4   # every step recovered on rank 1
    assert rec["verify"]["recall_at_k"] == 1.0
    assert rec["verify"]["rows_with_identical_id_order"] == 1.0
    assert rec["verify"]["max_abs_score_diff"] < 1e-3


def test_bench_eight_ranks_sharing_the_gpu_headline_shape():
    """The driver's widest launch, `python bench.py --gpus 8`, end to end on real kernels: eight fresh ranks (gloo, sharing the box's one
    GPU - RCCL refuses that), the headline's generation-chunk sharding (2 M rows = 8 chunks of 250 k), one packed all-gather + 8-way merge
    per step, the fp64 verification merged over the ranks, and the `comm` record of the line."""
    rec = _run_bench("--gpus", "8", "--backend", "gloo", "--rows", "2000000", "--dim", "128", "--nq", "512", "--k", "100", "--steps", "3",
                     "--warmup", "1", "--no-cpu-baseline", "--verify-queries", "32", timeout=1200)
    assert rec["n_gpus"] == 8 and rec["config"]["rows_per_gpu"] == 250_000 and rec["scaling"] == "strong"
    assert rec["comm"]["world_size"] == 8 and rec["comm"]["ranks_in_first_all_reduce"] == 8 and rec["comm"]["backend"] == "gloo"
    assert rec["verify"]["recall_at_k"] == 1.0 and rec["verify"]["max_abs_score_diff"] < 1e-3
    assert "all-gather" in rec["config"]["parallelism"]
    # round 5: one SCALE pass yields, per rank, the filter-kernel time, its roofline fraction and the exchange cost (HIP events)
    pr = rec["per_rank"]  # (parallel lists, rank order: the line stays below 4 KB)
    assert pr["rows"] == [250_000] * 8 and len(pr["kernel_ms"]) == len(pr["exchange_us"]) == 8
    assert all(v > 0 for v in pr["kernel_ms"] + pr["exchange_us"]) and all(0 < v < 1 for v in pr["mfma_frac_of_2.5PF"])
    assert abs(rec["exchange_us_per_step_max"] - max(pr["exchange_us"])) <= 1e-3 * max(pr["exchange_us"])
    twin = rec["verify"]["integer_twin"]  # merged over the eight ranks
    assert twin["ids_bit_exact"] is True and twin["scores_bit_exact"] is True


def test_bench_c4_preset_and_exact_mode_across_two_ranks():
    """`--config c4` selects BASELINE configs[3]'s shape (bf16, dim 1024, batch 512, top-200; fewer rows here), and `--exact-f32` makes
    every rank keep float32 rows: the merged result must match the UNROUNDED float32 inputs (per-shard exact lists merge exactly)."""
    rec = _run_bench("--gpus", "2", "--backend", "gloo", "--config", "c4", "--rows", "500000", "--exact-f32", "--steps", "3", "--warmup", "1",
                     "--no-cpu-baseline", "--verify-queries", "32")
    assert "x 1024 bf16, batch 512 queries, top-200" in rec["config"]["workload"] and "exact-f32" in rec["config"]["workload"]
    assert rec["verify"]["recall_at_k"] == 1.0 and rec["verify"]["max_abs_score_diff"] < 1e-3 and "UNROUNDED" in rec["verify"]["comparator"]
    assert rec["verify"]["vs_stored_rounded_rows"]["max_abs_score_diff"] > 1e-3  # (the bf16 scan alone would be this far off)
    assert len(rec["per_rank"]["kernel_ms"]) == 2


def test_bench_default_line_carries_the_side_workloads():
    """The default 1-GPU run times C2, nq = 256, clustered C3, the 1.25 M-row shard with the exchange, C4 and C5 next to the headline.
    Round 6: the final line stays below 4 KB (name -> [ms, frac, bound] per side workload); every side workload prints one `# side` comment
    line when it finishes and the full records go to gpurun_out/bench_side.json."""
    rec = _run_bench("--steps", "3", "--warmup", "1", "--cpu-seconds", "1")
    assert rec["config"]["workload"].startswith("10000000 sections x 768")
    names = ["C2", "C3_nq256", "C3_clustered", "C3_shard_of_8", "C3_shard_of_8_with_exchange", "C4_shard_of_8",
             "C2_exact_f32", "C3_exact_f32", "C4_shard_of_8_exact_f32", "C4_one_gpu", "C5"]
    assert list(rec["side"]) == names and [s_["name"] for s_ in rec["_side_lines"]] == names
    for name in names[:10]:
        ms, frac, bound = rec["side"][name]
        assert ms > 0 and frac > 0.05 and bound in ("mfma", "hbm")
    assert rec["side"]["C2"][2] == "hbm" and rec["side"]["C3_exact_f32"][2] == "mfma"  # SURVEY 8d's table: the nameplate roofs
    assert rec["side"]["C5"] == "ok"
    for s_ in rec["_side_lines"][:10]:
        assert s_["verify"]["recall_at_k"] == 1.0 and s_["verify"]["max_abs_score_diff"] < 1e-3 and s_["roofline"]["frac"] > 0.05
    full = json.loads((ROOT / rec["side_file"]).read_text())
    assert [s_["name"] for s_ in full["side"]] == names and full["headline"]["value"] > 0
    for s_ in full["side"][:10]:
        assert "error" not in s_ and "skipped" not in s_, s_
        assert s_["verify"]["recall_at_k"] == 1.0 and s_["roofline"]["frac"] > 0.05
        assert s_["verify"]["comparator"].startswith("float64") and s_["verify"]["max_abs_score_diff"] < 1e-3
        # round 5: every line also says how its result compares with the UNROUNDED float32 inputs (the reference's input type) ...
        vu = s_["verify"]["vs_unrounded_inputs"]
        assert 0.9 < vu["recall_at_k"] <= 1.0 and vu["max_abs_score_diff"] >= 0
        if "exact_f32" in s_["name"]:  # ... and the exact-f32 lines match them: float32 brute-force results
            assert "UNROUNDED" in s_["verify"]["comparator"] and vu["recall_at_k"] == 1.0 and vu["max_abs_score_diff"] < 1e-3
            assert s_["verify"]["exact_f32"]["list_rows_k_prime"] > 100
        else:  # a rounded store carries its rounding (fp16: ~1e-2, bf16: ~0.2): on the record, not hidden
            assert vu["max_abs_score_diff"] > 1e-3
    twin = full["side"][9]["verify"]["ids_bit_exact_on_integer_twin"]  # C4 at full size
    assert twin["ids_bit_exact"] is True and twin["scores_bit_exact"] is True and twin["rows"] == 40_000_000
    twin = rec["verify"]["integer_twin"]              # the headline at full size
    assert twin["ids_bit_exact"] is True and twin["scores_bit_exact"] is True and twin["rows"] == 10_000_000 and twin["queries_checked"] >= 32
    assert rec["verify"]["vs_unrounded_inputs"]["max_abs_score_diff"] > 1e-3
    c5 = full["side"][10]
    assert "error" not in c5, c5
    assert c5["verify"]["ok"] is True and c5["verify"]["collate_cases"] >= 4 and c5["verify"]["gradient_cases"] == 5
    assert c5["collate_merge_sample"]["host_syncs"] == 0 and c5["collate_merge_sample_flatten"]["host_syncs"] == 0
    assert 0 < c5["collate_merge_sample"]["wall_us"] < 2000 and 0 < c5["collate_merge_sample"]["device_us"] < 1.5 * c5["collate_merge_sample"]["wall_us"]  # (two separate medians)
    assert c5["retrieval_loss_inbatch_64x2048"]["fwd_bwd_wall_us"] > 0
    for shape in ("retrieval_loss_3d_64x32", "retrieval_loss_inbatch_64x2048"):  # the same step as one captured hipGraph
        assert c5[shape]["graphed_equals_eager"] is True and 0 < c5[shape]["graphed_fwd_bwd_wall_us"] < 400  # (the eager step varies 110-220 us with the box)
    # the tier's "CPU path timed beside it", for C5: the reference's numba loops restated in C on the host cores (and used as the checker of
    # the device chain on the same inputs), and the reference's H5 op sequence restated in eager torch on the same GPU
    assert c5["cpu_baseline"]["value"] > 0 and c5["cpu_baseline"]["kind"] == "port" and c5["cpu_baseline"]["device_chain_equals_cpu_restatement"] is True
    for shape in ("retrieval_loss_3d_64x32", "retrieval_loss_inbatch_64x2048"):
        assert c5["reference_op_sequence"][shape]["fwd_bwd_wall_us"] > 0 and c5["reference_op_sequence"][shape]["fused_equals_op_sequence"] is True
    assert rec["comm"]["world_size"] == 1 and rec["comm"]["ranks_in_first_all_reduce"] == 1  # (the exchange side line brought RCCL up)
    assert {"bound", "mfma_frac_of_2.5PF", "hbm_frac_at_8TBps", "frac", "achieved", "peak", "traffic", "practical"} <= set(rec["roofline"])
    assert rec["roofline"]["traffic_source"] and "exact" not in rec["roofline"]["traffic_source"]  # (round 5: the exact-mode PMC run had taken the plain key)
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["threads"] >= 1 and rec["cpu_baseline"]["cores"] >= 1
    assert len(rec["cpu_baseline"]["thread_arms"]) >= 1 and abs(rec["cpu_baseline"]["value"] - max(rec["cpu_baseline"]["thread_arms"].values())) < 0.01


def test_bench_node_engine_two_shards_on_one_gpu():
    """`bench.py --gpus N --engine node`: ONE process, `vodhip_node_index_*` over N devices - the second multi-GPU design is one flag away
    from a SCALE measurement.  Here two shards share the box's GPU (the exchange is forced through pinned host memory: the N > 1 step
    sequence - replicate the queries, search every shard, copy the lists to devices[0], merge - on real kernels)."""
    rec = _run_bench("--gpus", "2", "--engine", "node", "--node-devices", "0,0", "--rows", "500000", "--dim", "128", "--nq", "512", "--k", "50",
                     "--steps", "4", "--warmup", "2", "--verify-queries", "32")
    assert rec["n_gpus"] == 2 and rec["config"]["engine"] == "node" and "vodhip_node_index" in rec["config"]["parallelism"]
    assert rec["config"]["rows_per_gpu"] == 250_000 and rec["value"] > 0 and rec["roofline"]["frac"] > 0
    ps = rec["per_shard"]
    assert ps["rows"] == [250_000, 250_000] and ps["device"] == [0, 0] and all(v > 0 for v in ps["kernel_ms"])
    assert rec["merge_us"] > 0 and rec["copy_us_max"] > 0 and rec["peer_access"] == [2, 0]   # shard 1: staged through the host
    assert rec["verify"]["recall_at_k"] == 1.0 and rec["verify"]["rows_with_identical_id_order"] == 1.0 and rec["verify"]["max_abs_score_diff"] < 1e-3
    # the exact-f32 store behind the same engine: the merged result is the float32 brute force of the unrounded inputs
    rec = _run_bench("--gpus", "2", "--engine", "node", "--node-devices", "0,0", "--rows", "500000", "--dim", "128", "--nq", "512", "--k", "50",
                     "--steps", "2", "--warmup", "1", "--verify-queries", "32", "--exact-f32")
    assert rec["verify"]["recall_at_k"] == 1.0 and rec["verify"]["max_abs_score_diff"] < 1e-3 and "UNROUNDED" in rec["verify"]["comparator"]
