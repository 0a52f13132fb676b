"""How the whole-store scans cut a query batch into slices (vod_amd/csrc/scan_slices.h, host code only), checked on CPU.

The header is compiled here with the host compiler, next to a small driver that prints `scan_slice_queries(budget, per_query)` for
every pair it is given.  The rule: the slice is 64 or a multiple of 128, at most 1024, and the largest such value
whose temporaries (`slice * per_query` bytes) fit the budget - unless 64 queries alone need more, in which case it is 64 and the
temporaries exceed the budget.  With the default budget (`VODHIP_POSTERIOR_TEMP_BYTES`) the slices DESIGN.md states for a
10 M x 768 store come out of the same function.
"""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "vod_amd" / "csrc"
ALLOWED = [64] + list(range(128, 1025, 128))

DRIVER = r"""
#include <cstdio>
#include "scan_slices.h"
int main() {
    long long budget, per_query;
    while (scanf("%lld %lld", &budget, &per_query) == 2)
        printf("%lld\n", (long long)vodhip::scan_slice_queries((int64_t)budget, (size_t)per_query));
}
"""


def default_budget():
    """VODHIP_POSTERIOR_TEMP_BYTES as include/vodhip.h defines it"""
    m = re.search(r"#define VODHIP_POSTERIOR_TEMP_BYTES \((\d+)ll << (\d+)\)", (ROOT / "include" / "vodhip.h").read_text())
    assert m, "VODHIP_POSTERIOR_TEMP_BYTES is no longer `(<n>ll << <shift>)`"
    return int(m.group(1)) << int(m.group(2))


@pytest.fixture(scope="module")
def slices(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the Makefile builds the host-only sources with one)")
    d = tmp_path_factory.mktemp("scan_slices")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "scan_slices"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(CSRC), str(d / "driver.cpp"), "-o", str(exe)], check=True)

    def run(pairs):
        text = "".join(f"{b} {p}\n" for b, p in pairs)
        out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.split()
        assert len(out) == len(pairs)
        return [int(v) for v in out]

    return run


def expected(budget, per_query):
    """the largest allowed slice whose temporaries fit the budget; 64 when none does"""
    fit = [s for s in ALLOWED if s > 64 and s * per_query <= budget]
    return max(fit) if fit else 64


def grid():
    budgets = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 4096, 65536, 65537, 10 ** 6, (1 << 20) - 1, 1 << 20, 1 << 28, (1 << 28) + 1, 1 << 40]
    per_query = [1, 2, 3, 7, 16, 100, 272, 1024, 1025, 4096, 39063 * 16, 2 ** 21, 7_501_824, 1 << 28, (1 << 28) + 1, 1 << 33]
    pairs = [(b, p) for b in budgets for p in per_query]
    # every edge of every allowed slice: the budget that just fits it, one byte less, one byte more
    for p in (1, 3, 272, 1025, 625_008):
        for s in ALLOWED:
            pairs += [(s * p - 1, p), (s * p, p), (s * p + 1, p)]
    return [(b, p) for b, p in pairs if b >= 1]


def test_slice_is_the_largest_allowed_value_that_fits_the_budget(slices):
    pairs = grid()
    assert any(p > b for b, p in pairs) and any(b >= p and 64 * p > b for b, p in pairs) and any(p == 1 for _, p in pairs)
    got = slices(pairs)
    seen = set()
    for (budget, per_query), s in zip(pairs, got):
        what = f"budget {budget} per_query {per_query} -> {s}"
        assert s == 64 or s % 128 == 0, what
        assert 64 <= s <= 1024, what
        if s > 64:
            assert s * per_query <= budget, what
        bigger = [t for t in ALLOWED if t > s]
        assert all(t * per_query > budget for t in bigger), what  # no larger allowed slice fits
        assert s == expected(budget, per_query), what
        seen.add(s)
    assert seen == set(ALLOWED)  # the grid reaches every slice there is


def test_budget_of_per_query_times_slice_gives_that_slice(slices):
    """what the GPU tests rely on: budget = per_query * wanted selects `wanted`; budget 1 selects 64 through the clamp"""
    per_query = [1, 48, 272, 280, 1296, 1576, 7_501_824]
    pairs = [(p * s, p) for p in per_query for s in ALLOWED if s > 64]
    assert slices(pairs) == [s for _ in per_query for s in ALLOWED if s > 64]
    assert slices([(1, p) for p in per_query if p > 1]) == [64] * (len(per_query) - 1)


def test_the_slices_design_md_states_for_ten_million_rows(slices):
    """10 M rows x dim 768 with the default budget: the table of DESIGN.md 4 (derived, not measured)"""
    budget = default_budget()
    assert budget == 256 << 20
    n, dim_pad = 10_000_000, 768
    tiles = (n + 255) // 256
    mean_groups = (n + 16383) // 16384   # VODHIP_POSTERIOR_GROUP_ROWS
    read_groups = (n + 4095) // 4096     # VODHIP_READOUT_GROUP_ROWS
    assert (tiles, mean_groups, read_groups) == (39063, 611, 2442)
    per_query = {
        "posterior_stats": tiles * 16,
        "posterior_divergence": tiles * 32,
        "posterior_mean": mean_groups * dim_pad * 4,
        "posterior_expectation": read_groups * 64 * 4 + tiles * 8,
        "posterior_expectation_backward": read_groups * dim_pad * 4,
    }
    assert per_query["posterior_expectation_backward"] == 7_501_824  # 7.5 MB: 64 queries alone exceed the budget
    got = dict(zip(per_query, slices([(budget, p) for p in per_query.values()])))
    assert got == {"posterior_stats": 384, "posterior_divergence": 128, "posterior_mean": 128, "posterior_expectation": 256,
                   "posterior_expectation_backward": 64}
    assert 64 * per_query["posterior_expectation_backward"] > budget
