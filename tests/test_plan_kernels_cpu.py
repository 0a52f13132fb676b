"""Which filter kernel the search planner (vod_amd/csrc/search_plan.cpp, host code only) picks for every stage, checked on CPU.

The planner is compiled here with the host compiler, next to a small driver that prints a plan: per pass of queries, the kernel id
(the public "tile" ids) of every stage, plus the corpus-`nt` flag and the stage order.  The rules:
  * auto tile: nq > 128 -> 8, nq > 64 -> 46, else 42; nq_pad is a multiple of the kernel's query width;
  * FILTER stages of auto batches above 128 queries without a subset filter run the 8-phase kernel (14);
  * under auto with a persistent kernel, FILTER stages of fewer 256x256 tiles than small_chunk_tiles (x the pass's query tiles) run 1;
  * DENSE stages on a persistent kernel run 1; the bootstrap of an explicit 14 runs 8;
  * subset searches (not safe, not recovering) run the geometric schedule: a DENSE head, then FILTER stages;
  * corpus-nt: a persistent kernel and nq_pad == 256; the stage permutation: no DENSE stage, tile_order 0, >= 8 super-tiles.
"""
import pathlib
import shutil
import subprocess

import pytest

CSRC = pathlib.Path(__file__).resolve().parent.parent / "vod_amd" / "csrc"
FILTER, DENSE, GMAX = 0, 1, 2

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include "search_plan.h"
int main(int argc, char** argv) {
    using namespace vodhip;
    auto a = [&](int i) { return (int64_t)atoll(argv[i]); };
    PlanTunables t;
    t.cand_cap = a(4); t.small_chunk_tiles = a(5); t.tile = a(6); t.tile_order = a(7);
    const SearchPlan p = plan_search(a(1), (int)a(2), a(3), t, a(8) != 0, a(9) != 0, (int)a(10));
    printf("%lld %d %lld %lld\n", (long long)p.bn, (int)p.corpus_nt, (long long)p.perm_mul, (long long)p.perm_mod);
    for (int64_t q0 = 0; q0 < a(3); q0 += MAX_NQ_PER_PASS) {
        const int64_t nq_pad = round_up(std::min(MAX_NQ_PER_PASS, a(3) - q0), p.bn);
        printf("%lld", (long long)nq_pad);
        for (const Stage& sg : p.stages) printf(" %d:%d:%lld", sg.kind, (int)p.kernel(sg, nq_pad), (long long)(sg.e - sg.b));
        printf("\n");
    }
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the Makefile builds search_plan.cpp with one)")
    d = tmp_path_factory.mktemp("plan")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "plan"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(CSRC), str(d / "driver.cpp"), str(CSRC / "search_plan.cpp"), "-o", str(exe)],
                   check=True)

    def run(n, k, nq, cap=16384, small=256, tile=0, order=0, subset=False, safe=False, recovery=0):
        out = subprocess.run([str(exe), *map(str, (n, k, nq, cap, small, tile, order, int(subset), int(safe), recovery))],
                             check=True, capture_output=True, text=True).stdout.split("\n")
        bn, nt, pm, pd = map(int, out[0].split())
        passes = []
        for line in filter(None, out[1:]):
            nq_pad, *st = line.split()
            passes.append((int(nq_pad), [tuple(map(int, s.split(":"))) for s in st]))
        return dict(bn=bn, nt=bool(nt), perm=(pm, pd), passes=passes)

    return run


def kernels(p, kind, pass_=0):
    return {kern for kd, kern, _ in p["passes"][pass_][1] if kd == kind}


@pytest.mark.parametrize("nq,bn,nq_pad", [(1, 64, 64), (64, 64, 64), (65, 128, 128), (128, 128, 128), (129, 256, 256), (1024, 256, 1024)])
def test_auto_kernel_and_query_padding(plan, nq, bn, nq_pad):
    p = plan(10_000_000, 100, nq)
    assert p["bn"] == bn and p["passes"][0][0] == nq_pad
    base = {64: 42, 128: 46, 256: 8}[bn]
    assert kernels(p, GMAX) == {base}
    assert kernels(p, FILTER) <= ({14, 1} if bn == 256 else {base})


def test_auto_large_batches_filter_on_the_8phase_kernel_short_stages_on_128x128(plan):
    p = plan(10_000_000, 100, 1024)
    for kd, kern, rows in p["passes"][0][1]:
        if kd == FILTER:
            assert kern == (1 if (rows + 255) // 256 * 4 < 256 else 14)
    assert 14 in kernels(p, FILTER)
    # a stage that fills the CUs on 4 query tiles is short on a smaller last pass of one query tile
    p = plan(1_000_000, 100, 2048 + 256, small=1024)
    for (nq_pad, st0), (_, st1) in zip(p["passes"], p["passes"][1:]):
        assert nq_pad == 2048
        for (kd, k0, rows), (_, k1, _) in zip(st0, st1):
            if kd == FILTER:
                assert k0 == (1 if (rows + 255) // 256 * 8 < 1024 else 14)
                assert k1 == (1 if (rows + 255) // 256 * 1 < 1024 else 14)


@pytest.mark.parametrize("tile", [8, 9, 14])
def test_explicit_persistent_kernels_keep_short_stages(plan, tile):
    p = plan(10_000_000, 100, 1024, tile=tile, small=1 << 30)
    assert kernels(p, FILTER) == {tile}
    assert kernels(p, GMAX) == {8 if tile == 14 else tile}


@pytest.mark.parametrize("tile", [0, 8, 9, 14])
def test_dense_stages_of_persistent_kernels_run_128x128(plan, tile):
    p = plan(1_000_000, 100, 1024, tile=tile, safe=True)
    assert {kd for kd, _, _ in p["passes"][0][1]} == {DENSE}
    assert kernels(p, DENSE) == {1}


@pytest.mark.parametrize("tile,filter_kernels", [(0, {8, 1}), (14, {14})])
def test_subset_searches_run_the_geometric_schedule(plan, tile, filter_kernels):
    p = plan(10_000_000, 100, 1024, tile=tile, subset=True)
    st = p["passes"][0][1]
    assert st[0][0] == DENSE and all(kd == FILTER for kd, _, _ in st[1:])
    assert kernels(p, FILTER) <= filter_kernels and kernels(p, DENSE) == {1}
    assert p["perm"] == (0, 0)  # a DENSE stage: row order


@pytest.mark.parametrize("tile,nq,nt", [(0, 256, True), (0, 200, True), (0, 1024, False), (8, 100, True), (0, 100, False), (46, 256, False)])
def test_corpus_nt_flag(plan, tile, nq, nt):
    assert plan(10_000_000, 100, nq, tile=tile)["nt"] is nt


def test_stage_order(plan):
    mul, mod = plan(10_000_000, 100, 1024)["perm"]
    assert mod == (10_000_000 + 255) // 256 and mul > 1
    assert plan(10_000_000, 100, 1024, order=1)["perm"] == (0, 0)
    assert plan(7 * 256, 10, 1024, cap=256)["perm"] == (0, 0)  # fewer than 8 super-tiles
    p = plan(1_000_000, 100, 1024, recovery=2)
    assert {kd for kd, _, _ in p["passes"][0][1]} == {FILTER} and p["perm"][0] > 1
