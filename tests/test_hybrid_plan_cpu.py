"""The LDS plan of the hybrid merge kernel (vod_amd/csrc/hybrid_plan.h, host code only), checked on the CPU for EVERY row width.

`launch_merge_hybrid` sizes the kernel's open-addressing table with `hybrid_plan(W)`.  Its contract: a power-of-two table of at
least 64 slots, load factor <= 1/4 (T >= 4 W) wherever that table fits the plan's own cap, never above 1/2 (T >= 2 W), inside the
LDS of one gfx950 workgroup (160 KiB).  Results do not depend on T - a table at load factor 0.9998 still merges correctly, with probe
chains thousands of LDS reads long - so no parity test can see a wrong size: this one restates the arithmetic.
"""
import pathlib
import shutil
import subprocess

import pytest

CSRC = pathlib.Path(__file__).resolve().parent.parent / "vod_amd" / "csrc"
MAX_W = 4096         # the width the C ABI admits
LDS_LIMIT = 163840   # bytes of LDS one workgroup can have on gfx950

DRIVER = r"""
#include <cstdio>
#include "hybrid_plan.h"
int main() {
    using namespace vodhip;
    printf("%d %d %zu %zu\n", HY_THREADS, HY_WAVES, (size_t)HY_LDS_CAP, (size_t)HY_LDS_SLACK);
    for (int W = 0; W <= HY_MAX_WIDTH; ++W) {
        const HybridPlan p = hybrid_plan(W);
        printf("%d %d %zu\n", W, p.T, p.lds);
    }
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the Makefile builds the host-only sources with one)")
    d = tmp_path_factory.mktemp("hybrid_plan")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "hybrid_plan"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(CSRC), str(d / "driver.cpp"), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    threads, waves, cap, slack = map(int, lines[0].split())
    rows = [tuple(map(int, ln.split())) for ln in lines[1:] if ln]
    assert [w for w, _, _ in rows] == list(range(MAX_W + 1))
    return dict(threads=threads, waves=waves, cap=cap, slack=slack, rows=rows)


def carve_up(W, T, waves, slack):
    """The kernel's LDS carve-up (kernels_hybrid.hip, `// LDS carve-up`), element sizes written out."""
    ids = 8 * W              # int64 [W]
    table = 8 * T            # uint64 [T]
    wsc = 4 * W              # float [W]
    nsc = 4 * W              # float [W]
    pre = 4 * (W + 1)        # int [W + 1]
    s_min = 4 * waves * 4    # float [waves][4]
    s_misc = 4 * (waves + 1)  # int [waves + 1]
    multi = 1 * T            # unsigned char [T]
    return ids + table + wsc + nsc + pre + s_min + s_misc + multi + slack


def test_constants(plans):
    assert plans["threads"] == 512 and plans["waves"] == plans["threads"] // 64
    assert plans["cap"] <= LDS_LIMIT and 0 <= plans["slack"] <= 16


def test_table_is_a_power_of_two_of_at_least_64_slots_and_at_most_half_full(plans):
    bad = [(W, T) for W, T, _ in plans["rows"] if T & (T - 1) or T < 64 or T < 2 * W]
    assert not bad, f"{len(bad)} widths, first {bad[:5]}"


def test_table_is_at_most_a_quarter_full_wherever_that_table_fits_the_cap(plans):
    bad = []
    for W, T, _ in plans["rows"]:
        t4 = 64
        while t4 < 4 * W:
            t4 *= 2
        if carve_up(W, t4, plans["waves"], plans["slack"]) <= plans["cap"] and T < 4 * W:
            bad.append((W, T))
    assert not bad, f"{len(bad)} widths, first {bad[:5]}"


def test_footprint_is_the_kernels_carve_up_and_fits_one_workgroup(plans):
    for W, T, lds in plans["rows"]:
        assert lds == carve_up(W, T, plans["waves"], plans["slack"]), (W, T, lds)
        assert lds <= LDS_LIMIT, (W, T, lds)
    assert max(lds for _, _, lds in plans["rows"]) == plans["rows"][MAX_W][2] == 155832  # W = 4096, T = 8192


def test_table_never_shrinks_as_the_row_grows(plans):
    ts = [T for _, T, _ in plans["rows"]]
    bad = [(W, ts[W - 1], ts[W]) for W in range(1, len(ts)) if ts[W] < ts[W - 1]]
    assert not bad, bad[:5]
