"""How the search planner (vod_amd/csrc/search_plan.cpp, host code only) sizes the survivor rings of the 8-phase FILTER kernel, checked on CPU.

Rule (search_plan.h, survivor_ring_records): a FILTER stage against a threshold calibrated on C rows passes ~1.4 k * rows / C rows
per query (C = the bootstrap's sampled rows for the first stage, the rows before the stage later, the whole store in a recovery pass).
The waves that see a query are the two wave rows of every workgroup of its query tile (8 * floor(n_cu / (8 * query tiles)) workgroups,
at least 8).  Records per wave = 2 x (the largest stage's survivors per query x 64 queries / those waves) + 64, in steps of 64, at most
1024 (277 MB of workspace per lane on 256 CUs, whatever k and the batch); "survivor_ring" = n forces n; no ring (0) when no FILTER stage
runs the 8-phase kernel.
"""
import math
import pathlib
import shutil
import subprocess

import pytest

CSRC = pathlib.Path(__file__).resolve().parent.parent / "vod_amd" / "csrc"

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "search_plan.h"
int main(int argc, char** argv) {
    using namespace vodhip;
    auto a = [&](int i) { return (int64_t)atoll(argv[i]); };
    PlanTunables t;
    t.tile = a(4); t.survivor_ring = a(5); t.n_cu = (int)a(6);
    const SearchPlan p = plan_search(a(1), (int)a(2), a(3), t, a(7) != 0, a(8) != 0, (int)a(9));
    printf("%lld\n", (long long)p.ring);
    for (const Stage& sg : p.stages)
        printf("%d %d %lld %lld %lld\n", sg.kind, (int)sg.kernel, (long long)sg.b, (long long)sg.e, (long long)sg.n_tiles);
}
"""
FILTER, DENSE, GMAX = 0, 1, 2
AUTO_CAP = 1024  # records per wave


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the Makefile builds search_plan.cpp with one)")
    d = tmp_path_factory.mktemp("ring")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "plan"
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", str(CSRC), str(d / "driver.cpp"), str(CSRC / "search_plan.cpp"), "-o", str(exe)],
                   check=True)

    def run(n, k, nq, tile=0, ring=0, n_cu=256, subset=False, safe=False, recovery=0):
        out = subprocess.run([str(exe), *map(str, (n, k, nq, tile, ring, n_cu, int(subset), int(safe), recovery))],
                             check=True, capture_output=True, text=True).stdout.split("\n")
        return int(out[0]), [tuple(map(int, line.split())) for line in out[1:] if line]

    return run


def expected(n, k, nq, stages, n_cu=256):
    per_query, calibrated = 0.0, n
    for kind, kern, b, e, n_tiles in stages:
        if kind == GMAX:
            calibrated = n_tiles * 256
        if kind == FILTER and kern == 14:
            per_query = max(per_query, 1.4 * k * (e - b) / calibrated)
        if kind != GMAX:
            calibrated = e
    if per_query == 0.0:
        return 0
    n_qt = -(-min(nq, 2048) // 256)
    unit = 8 * n_qt
    grid = max(unit, n_cu // unit * unit)
    per_wave = per_query * 64 / (2 * grid // n_qt)
    return min(AUTO_CAP, math.ceil((int(2 * per_wave) + 64) / 64) * 64)


@pytest.mark.parametrize("n,k,nq,n_cu", [(10_000_000, 100, 1024, 256), (10_000_000, 100, 256, 256), (1_250_000, 100, 1024, 256),
                                         (1_000_000, 100, 256, 256), (5_000_000, 200, 512, 256), (40_000_000, 200, 512, 304),
                                         (10_000_000, 100, 2300, 256), (10_000_000, 100, 1024, 80), (200_000, 10, 300, 256)])
def test_ring_follows_the_largest_stage(plan, n, k, nq, n_cu):
    ring, stages = plan(n, k, nq, n_cu=n_cu)
    assert any(kind == FILTER and kern == 14 for kind, kern, *_ in stages)
    assert ring == expected(n, k, nq, stages, n_cu) and ring % 64 == 0 and 64 < ring <= AUTO_CAP


def test_headline_ring(plan):
    # 10 M x 768, nq 1024, top-100: growth 3 behind a N / 192 bootstrap, 128 waves per query column -> a few hundred records
    ring, _ = plan(10_000_000, 100, 1024)
    assert 256 <= ring <= 1024


def test_more_waves_per_query_column_fewer_records(plan):
    r4, _ = plan(10_000_000, 100, 1024, tile=14)
    r1, _ = plan(10_000_000, 100, 256, tile=14)
    assert plan(10_000_000, 100, 1024, tile=14, n_cu=128)[0] > r4
    assert r1 < r4 * 2  # one query tile: 4x the waves per column, ~the survivors of the same stage sizes


@pytest.mark.parametrize("ring", [1, 4, 777, 8192])
def test_forced_ring(plan, ring):
    assert plan(10_000_000, 100, 1024, ring=ring)[0] == ring


@pytest.mark.parametrize("kw", [dict(nq=128), dict(nq=1024, subset=True), dict(nq=1024, safe=True), dict(nq=1024, tile=8),
                                dict(nq=1024, ring=5, tile=8)])
def test_no_ring_without_the_8phase_kernel(plan, kw):
    nq = kw.pop("nq")
    ring, stages = plan(10_000_000, 100, nq, **kw)
    assert ring == 0 and not any(kern == 14 and kind == FILTER for kind, kern, *_ in stages)


def test_recovery_pass_calibrated_on_the_whole_store(plan):
    ring, stages = plan(1_000_000, 100, 1024, tile=14, recovery=2)
    assert [kind for kind, *_ in stages] == [FILTER, FILTER]
    assert ring == expected(1_000_000, 100, 1024, stages)


@pytest.mark.parametrize("n,k,nq", [(10_000_000, 2048, 2048), (10_000_000, 1000, 2048), (10_000_000, 2048, 256), (40_000_000, 1000, 1024)])
def test_auto_ring_is_capped(plan, n, k, nq):
    # large k and many query tiles would ask for thousands of records per wave (17 k at k 2048, nq 2048: 4.7 GB per lane); the
    # planner stops at 1024 and the blocks that do not fit take the in-loop path
    ring, stages = plan(n, k, nq)
    assert ring == AUTO_CAP
    assert 8 * 256 * ring * 132 <= 280 * 2**20  # bytes of rings per lane on 256 CUs
