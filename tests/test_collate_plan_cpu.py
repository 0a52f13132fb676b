"""The LDS plan of the collate-side kernels (vod_amd/csrc/collate_plan.h, host code only), checked on the CPU for EVERY shape the
C ABI admits.

`launch_sample_args` and `launch_flatten_inbatch` (kernels_sample.hip) take the dynamic LDS of `priority_sample_kernel` and
`flatten_inbatch_kernel` from this header, and `vodhip_flatten_inbatch` / `vodhip_collate` take the admitted shapes of the one-launch
flattening from it.  A footprint that is too small lets a kernel write past its LDS; one above the 163,840 bytes of a gfx950 workgroup
cannot be launched.  No parity test at a handful of shapes can see either, so this one restates the kernels' pointer arithmetic in
Python, element sizes written out, and compares it with the header for

  * the sampler: every (sort capacity P in 256 ... 4096, k_total in 1 ... 4096, proposal in {0, 1}),
  * the flattening: every (n_rows, n_keys) with n_rows * n_keys <= 8192 and n_keys <= 1024.

Before this header existed the entry points admitted that whole rectangle, and `test_every_admitted_flattening_fits_one_workgroup`
fails on such a rule for exactly the 12 shapes 8 x 1013 ... 8 x 1024 (163,880 ... 164,944 bytes; 8 x 1012 takes 163,780).
`flatten_admits` now excludes exactly those: `flatten_samples` gathers them with `vodhip_gather_by_id`.
"""
import pathlib
import shutil
import subprocess

import pytest

CSRC = pathlib.Path(__file__).resolve().parent.parent / "vod_amd" / "csrc"
LDS_LIMIT = 163840   # bytes of LDS one workgroup can have on gfx950
MAX_WIDTH = 4096     # candidates per row the sampler's entry points admit
MAX_K_TOTAL = 4096   # samples per row they admit
MAX_IDS = 8192       # ids in a batch the flattening's entry points admit ...
MAX_KEYS = 1024      # ... and ids per row
TOO_LARGE = [(8, n) for n in range(1013, 1025)]

DRIVER = r"""
#include <cstdio>
#include "collate_plan.h"
int main() {
    using namespace vodhip;
    printf("K %d %d %zu %zu %d %d %d %d %d\n", SM_THREADS, FL_THREADS, (size_t)CL_LDS_LIMIT, (size_t)CL_LDS_SLACK, SM_MAX_WIDTH, SM_MAX_K_TOTAL,
           FL_MAX_IDS, FL_MAX_KEYS, FL_MAX_VALUES);
    for (int w = 0; w <= SM_MAX_WIDTH; ++w) printf("C %d %d\n", w, sample_sort_capacity(w));
    for (int P = 256; P <= 4096; P <<= 1)
        for (int k = 1; k <= SM_MAX_K_TOTAL; ++k)
            for (int p = 0; p < 2; ++p) printf("S %d %d %d %zu\n", P, k, p, sample_lds_bytes(P, k, p != 0));
    // the rectangle of the two size bounds, and one step past each of them
    for (int n_keys = 0; n_keys <= FL_MAX_KEYS + 1; ++n_keys)
        for (int n_rows = 0; n_rows <= (n_keys ? FL_MAX_IDS / n_keys : 2) + 1; ++n_rows) {
            const bool in_bounds = n_keys <= FL_MAX_KEYS && (long long)n_rows * n_keys <= FL_MAX_IDS;
            const FlattenPlan p = in_bounds ? flatten_plan(n_rows, n_keys) : FlattenPlan{0, 0, 0};
            printf("F %d %d %d %d %zu %d\n", n_rows, n_keys, p.U, p.P, p.lds, (int)flatten_admits(n_rows, n_keys));
        }
}
"""


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (the Makefile builds the host-only sources with one)")
    d = tmp_path_factory.mktemp("collate_plan")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "collate_plan"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", str(CSRC), str(d / "driver.cpp"), "-o", str(exe)], check=True)
    out = {"K": [], "C": [], "S": [], "F": []}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if ln:
            out[ln[0]].append(tuple(map(int, ln.split()[1:])))
    names = ("sm_threads", "fl_threads", "limit", "slack", "max_width", "max_k_total", "max_ids", "max_keys", "max_values")
    out.update(dict(zip(names, out["K"][0])))
    return out


def sampler_carve_up(P, k_total, proposal, waves):
    """`priority_sample_kernel`'s LDS, array by array in the order of its pointer arithmetic: the offset one past the last array."""
    end = 0
    end += 8 * P              # keys     u64   [P_cap]
    end += 4 * P              # lp       float [P_cap]
    end += 4 * k_total        # wsel     float [k_total]
    end += 4 * k_total        # isel     int   [k_total]
    end += 4 * k_total        # sel_all  int   [k_total]
    end += 4 * P              # order    int   [P_cap]
    end += 4 * waves          # red      float [one per wavefront]
    end += 4 * 16             # red_i    int   [16]: four engines' maxima per wavefront
    if proposal:
        end += 4 * 2          # mass_s   float [2]
        end += 4 * k_total    # wall     float [k_total]
    return end


def flatten_carve_up(U, P, n_keys, max_values, waves):
    """`flatten_inbatch_kernel`'s LDS in the order of its pointer arithmetic: (offset of s_w, offset one past it)."""
    end = 0
    end += 8 * P                      # srt   int64 [P]
    end += 8 * U                      # uq    int64 [U]
    end += 4 * max_values * n_keys    # vals  float [8][n_keys], whatever n_values is
    end += (n_keys + 3) // 4 * 4      # lab   uint8 [n_keys], rounded up so that s_w is 4-byte aligned
    s_w = end
    end += 4 * waves                  # s_w   int   [one per wavefront]
    return s_w, end


def test_constants_are_the_limits_of_the_c_abi(plans):
    assert plans["sm_threads"] == 256 and plans["fl_threads"] == 1024  # the kernels' launch bounds; red_i [16] holds 4 waves x 4 engines
    assert plans["limit"] == LDS_LIMIT and 0 <= plans["slack"] <= 16
    assert (plans["max_width"], plans["max_k_total"], plans["max_ids"], plans["max_keys"], plans["max_values"]) == (MAX_WIDTH, MAX_K_TOTAL, MAX_IDS, MAX_KEYS, 8)


def test_sampler_sort_capacity_is_a_size_the_sort_network_has(plans):
    """`wg_sort_lds_256` sorts 256, 512, ..., 4096 keys and does NOTHING for any other count."""
    assert [w for w, _ in plans["C"]] == list(range(MAX_WIDTH + 1))
    bad = [(w, P) for w, P in plans["C"] if P not in (256, 512, 1024, 2048, 4096) or P < w or (P > 256 and P // 2 >= w)]
    assert not bad, bad[:5]


def test_sampler_footprint_is_the_kernels_carve_up_and_fits_one_workgroup(plans):
    assert len(plans["S"]) == 5 * MAX_K_TOTAL * 2
    waves = plans["sm_threads"] // 64
    bad = [(P, k, p, lds) for P, k, p, lds in plans["S"] if lds != sampler_carve_up(P, k, p, waves) + plans["slack"] or lds > LDS_LIMIT]
    assert not bad, f"{len(bad)} shapes, first {bad[:5]}"
    # the largest: the widest row, the most samples, with the proposal; the old entry points stay 16,392 bytes below it
    assert max(lds for *_, lds in plans["S"]) == sampler_carve_up(4096, 4096, 1, waves) + plans["slack"] == 131176
    assert sampler_carve_up(4096, 4096, 0, waves) + plans["slack"] == 114784


def _rectangle(plans):
    return [r for r in plans["F"] if r[1] <= MAX_KEYS and r[0] * r[1] <= MAX_IDS]


def test_flattening_rows_cover_the_rectangle_of_the_size_bounds(plans):
    got = {(r, n) for r, n, *_ in _rectangle(plans)}
    want = {(r, n) for n in range(1, MAX_KEYS + 1) for r in range(1, MAX_IDS // n + 1)}
    assert want <= got and all(r == 0 or n == 0 for r, n in got - want)


def test_flattening_sort_size_is_one_the_sort_network_has(plans):
    """`wg_sort_lds_1024` sorts 1024, 2048, 4096 or 8192 keys and does NOTHING for any other count; after the sort the first n_keys
    slots of the sort buffer hold the row's own ids."""
    bad = [(r, n, U, P) for r, n, U, P, _, _ in _rectangle(plans)
           if U != r * n or P not in (1024, 2048, 4096, 8192) or P < U or (P > 1024 and P // 2 >= U) or n > P]
    assert not bad, bad[:5]


def test_flattening_footprint_is_the_kernels_carve_up(plans):
    waves = plans["fl_threads"] // 64
    bad = []
    for r, n, U, P, lds, _ in _rectangle(plans):
        s_w, end = flatten_carve_up(U, P, n, plans["max_values"], waves)
        if lds != end + plans["slack"] or s_w % 4:
            bad.append((r, n, lds, end))
    assert not bad, f"{len(bad)} shapes, first {bad[:5]}"


def test_every_admitted_flattening_fits_one_workgroup(plans):
    too_large = [(r, n, lds) for r, n, _, _, lds, admits in plans["F"] if admits and lds > LDS_LIMIT]
    assert not too_large, f"{len(too_large)} admitted shapes above {LDS_LIMIT} bytes: {too_large}"


def test_the_flattening_refuses_what_is_out_of_bounds_and_exactly_the_twelve_shapes_that_do_not_fit(plans):
    rect = _rectangle(plans)
    assert sorted((r, n) for r, n, _, _, lds, _ in rect if lds > LDS_LIMIT) == TOO_LARGE
    assert sorted((r, n) for r, n, *_, admits in rect if not admits) == TOO_LARGE
    outside = [row for row in plans["F"] if not (row[1] <= MAX_KEYS and row[0] * row[1] <= MAX_IDS)]
    assert {(1, 1025), (9, 1024), (8193, 1), (17, 512)} <= {(r, n) for r, n, *_ in outside}  # one step past either bound
    assert not any(admits for *_, admits in outside)
    by_shape = {(r, n): lds for r, n, _, _, lds, _ in rect}
    assert (by_shape[8, 1012], by_shape[8, 1013], by_shape[8, 1024], by_shape[8, 1000], by_shape[7, 1024]) == (163780, 163880, 164944, 162616, 156752)


def test_the_library_answers_with_the_plan(plans):
    """`vodhip_flatten_inbatch_admits` - what `flatten_samples` and `collate_on_device` choose their path by - is `flatten_admits`."""
    from vod_amd import _native

    lib = _native.load_library()
    bad = [(r, n) for r, n, *_, admits in plans["F"] if lib.vodhip_flatten_inbatch_admits(r, n) != admits]
    assert not bad, bad[:5]
    assert lib.vodhip_flatten_inbatch_admits(-1, 4) == 0 and lib.vodhip_flatten_inbatch_admits(4, -1) == 0
    assert lib.vodhip_flatten_inbatch_admits(1 << 62, 1024) == 0 and lib.vodhip_flatten_inbatch_admits(1 << 62, 0) == 1
