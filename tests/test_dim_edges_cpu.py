"""The width table of tests/test_dim_edges_gpu.py, and CPU proof that its shapes run what they claim.

The fused inner-product top-k is tested in depth along every axis but the embedding width: `nk = dim_pad / 64` took the values 1, 2,
4, 6, 12 and 16 only, so every corpus tile of a persistent workgroup started on operand-buffer parity 0, no scan kernel ever ran more
than 16 K-tiles, and exact-f32 mode never left `exact_dot_preload`.  The tables below name the widths that close this, each with the
reason it is there; the GPU module imports them.  This module checks on the CPU, with the host planner (the `plan` fixture and driver of
tests/test_plan_kernels_cpu.py, imported, not copied):

  * every (n, k, nq, tile) of the GPU module plans a FILTER stage on the kernel the case forces (auto tile: on the planner's own mix);
  * for the persistent kernels (8, 9, 14) that stage has more 256-row tiles than `xt_step`, and at least a quarter of the workgroup
    columns walk two or more corpus tiles - otherwise no workgroup crosses a corpus-tile boundary and an odd `nk` proves nothing;
  * the integer fixtures are exact in fp32 at every width used.

`xt_step` restates `launch_8phase` / the persistent launch of kernels_mips.hip for 256 CUs:

    n_qtiles = nq_pad / 256;  unit = 8 * n_qtiles;  total = ceil(n_xtiles / 8) * unit
    grid     = clamp((256 / unit) * unit, unit, total)        # rounded DOWN to a multiple of 8 * n_qtiles
    xt_step  = grid / n_qtiles

Workgroup column xt0 (0 <= xt0 < xt_step) walks the tiles xt0, xt0 + xt_step, ...: it crosses a boundary iff xt0 + xt_step < n_xtiles,
so min(xt_step, n_xtiles - xt_step) columns do.
"""
import pytest

from test_plan_kernels_cpu import DRIVER, FILTER, GMAX, kernels, plan  # noqa: F401  (`plan` is the fixture, DRIVER what it compiles)

N_CU = 256
PERSISTENT = (8, 9, 14)

# ---- scan kernels: (dim, nk, why the width is there) -------------------------------------------------------------------------------
SCAN_WIDTHS = [
    (1, 1, "one live column, 63 padded: the smallest store there is"),
    (7, 1, "below the 8-element ingest group: scalar convert path, nk = 1 flips the parity on every corpus tile"),
    (65, 2, "one column into the second K-tile: 63 padded columns are multiplied as data would be"),
    (192, 3, "the smallest odd nk > 1: corpus tiles start on alternating operand-buffer parity"),
    (320, 5, "odd nk, 4 k + 1: the two-slot ring ends a tile on slot 0"),
    (448, 7, "odd nk = the 8-phase lead of 7 half-tiles: the prologue's last stage meets the tile's end"),
    (832, 13, "odd nk above the widths of every earlier test but 1024"),
    (1088, 17, "the first nk above 16, and odd: one K-tile more than any scan kernel has run"),
    (1536, 24, "a common encoder width (nk even, 1.5 x the largest tested)"),
    (2048, 32, "a common encoder width"),
    (4096, 64, "a common encoder width: 4 x the K loop length of any earlier test"),
]
BF16_WIDTHS = (192, 448, 1088, 4096)   # the per-tile bit-exact tests were fp16 only
AUTO_WIDTHS = (192, 1088, 4096)        # the planner's own kernel mix at an odd nk, the first nk > 16, the longest K loop
MARKER_WIDTHS = (192, 1088)
TOP_DIM = 16384                        # nk = 256: the limit vodhip_index_create states for exact-f32 stores; the plain store states none
SMALL_NQ = {1: 100, 42: 50, 46: 100}   # the batch sizes of test_mips_gpu.test_subset_filtered_search
SMALL_N = 20_001                       # 79 row tiles, the last one holds a single row
KS = (10, 100)


def persistent_shape(dim):
    """(n, nq) of the persistent-kernel cases: four query tiles (xt_step 64), and a store that plans as ONE FILTER stage of 157 row
    tiles (all 64 workgroup columns walk two or three) or of 80 (16 columns walk two); the smaller store from dim 1536 on keeps
    nq * n * dim of the float64 oracle below 1e11.  Not any n does: 24,000 rows at k = 10 plan as stages of 64 and 30 tiles - one round
    of the grid and a tail, no workgroup walks a second tile - which the check below refuses."""
    return (40_000 if dim < 1536 else 20_470), 1024


def _why(dim):
    return next(w for d, _nk, w in SCAN_WIDTHS if d == dim)


# (family, tile, dim, dtype, n, nq, ks, why) - sorted by dim: the cases of one width share one data set and one oracle run
WIDE_CASES = sorted(
    [("persistent", t, d, "float16", *persistent_shape(d), KS, w) for d, _nk, w in SCAN_WIDTHS for t in PERSISTENT]
    + [("persistent", t, d, "bfloat16", *persistent_shape(d), KS, "bf16 MFMA: " + _why(d)) for d in BF16_WIDTHS for t in PERSISTENT]
    + [("auto", 0, d, "float16", persistent_shape(d)[0], nq, KS, "auto tile, the planner's own kernels: " + _why(d))
       for d in AUTO_WIDTHS for nq in (300, 1024)],
    key=lambda c: c[2])
SMALL_CASES = [("small", t, d, "float16", SMALL_N, SMALL_NQ[t], KS, w) for d, _nk, w in SCAN_WIDTHS for t in (1, 42, 46)]
# rows and queries zero except in column dim - 1: one case per kernel family and width
MARKER_CASES = [("marker", t, d, "float16", (persistent_shape(d)[0] if t in PERSISTENT else SMALL_N), (1024 if t in PERSISTENT else SMALL_NQ[t]), (10,),
                 "only column dim - 1 is live: a dropped or doubled last K-tile, or a padded column read as data, changes every score")
                for d in MARKER_WIDTHS for t in (1, 8, 9, 14, 42, 46)]
SUBSET_CASES = [("subset", t, 320, "float16", 40_000, 1024, (50,), "the SUBSET instantiation at an odd nk") for t in (8, 14)]
# The top of the range: 5,000 rows are 20 row tiles, fewer than any persistent grid has columns, so no workgroup of tile 14 walks two
# tiles here (a store that does would cost the oracle 3e11 multiply-adds): these two cases prove the K loop of 256 K-tiles and the
# 32 KB row pitch, the boundary crossing is proved at 4096 and below.
TOP_CASES = [("top", 1, TOP_DIM, "float16", 5_000, 100, (10,), "nk = 256 on the 128x128 kernel"),
             ("top", 14, TOP_DIM, "float16", 5_000, 300, (10,), "nk = 256 on the 8-phase kernel: 1,024 phases per corpus tile")]
SCAN_CASES = WIDE_CASES + SMALL_CASES + MARKER_CASES + SUBSET_CASES + TOP_CASES

# ---- exact-f32 mode: (dim, why) --------------------------------------------------------------------------------------------------
EXACT_WIDTHS = [
    (64, "exact_dot_preload<NI = 1>, a quarter of its 256 columns"),
    (256, "NI = 1, full"),
    (257, "NI = 2 by one column (dim_pad 320)"),
    (512, "NI = 2, full"),
    (513, "NI = 3 by one column"),
    (768, "NI = 3, full"),
    (769, "NI = 4 by one column"),
    (1024, "NI = 4, full: the last width of the preload path"),
    (1025, "the first width of the generic exact_dot (dim_pad 1088, five blocks, the last a quarter full); scalar ingest"),
    (1536, "generic exact_dot, six full blocks; ingest loops three times"),
    (4096, "generic exact_dot, 16 blocks; 16 KB of query in LDS; ingest loops eight times"),
]
EXACT_BF16_WIDTHS = (1025, 4096)
EXACT_INT_WIDTHS = (1025, 1536, 4096)
EXACT_PATH_WIDTHS = (1088, 4096)
EXACT_ROW_WIDTHS = (1025, 1027, 4096)  # 1027: not a multiple of 8 - the scalar ingest path over more than 512 columns
EXACT_MAX_DIM = 16384                  # "VODHIP_EXACT_F32 stores take dim <= 16384" (vodhip_index_create)


def nk_of(dim):
    return -(-dim // 64)


def xt_step(nq_pad, n_xtiles, n_cu=N_CU):
    n_qtiles = nq_pad // 256
    unit = 8 * n_qtiles
    total = -(-n_xtiles // 8) * unit
    grid = min(max(n_cu // unit * unit, unit), total)
    return grid // n_qtiles


def crossing_columns(n_xtiles, step):
    """workgroup columns that walk two or more corpus tiles"""
    return max(0, min(step, n_xtiles - step))


def _plan_keys(cases):
    """the distinct (n, k, nq, tile, subset) the planner sees"""
    return sorted({(n, k, nq, tile, fam == "subset") for fam, tile, _d, _dt, n, nq, ks, _w in cases for k in ks})


def _filter_stages(p, kernel):
    nq_pad, stages = p["passes"][0]
    return nq_pad, [-(-rows // 256) for kd, kern, rows in stages if kd == FILTER and kern == kernel]


def test_the_tables_hold_every_width_with_its_reason():
    assert [d for d, _, _ in SCAN_WIDTHS] == [1, 7, 65, 192, 320, 448, 832, 1088, 1536, 2048, 4096]
    assert all(nk == nk_of(d) for d, nk, _ in SCAN_WIDTHS)
    assert {nk for _, nk, _ in SCAN_WIDTHS} >= {3, 5, 7, 13, 17, 24, 32, 64} and nk_of(TOP_DIM) == 256
    assert [d for d, _ in EXACT_WIDTHS] == [64, 256, 257, 512, 513, 768, 769, 1024, 1025, 1536, 4096]
    # exact_rescore_kernel: ni = ceil(dim_pad / 256) picks exact_dot_preload<NCR, 1..4>, anything above the generic exact_dot
    ni = {d: -(-nk_of(d) * 64 // 256) for d, _ in EXACT_WIDTHS}
    assert {ni[d] for d in (64, 256)} == {1} and {ni[d] for d in (257, 512)} == {2} and {ni[d] for d in (513, 768)} == {3}
    assert {ni[d] for d in (769, 1024)} == {4} and all(ni[d] > 4 for d in (1025, 1536, 4096))
    assert all(ni > 4 for ni in (-(-nk_of(d) * 64 // 256) for d in EXACT_INT_WIDTHS + EXACT_PATH_WIDTHS + EXACT_ROW_WIDTHS))
    assert all(len(c[-1]) > 10 for c in SCAN_CASES) and all(len(w) > 5 for _, w in EXACT_WIDTHS)  # every row carries its reason
    for fam, tile, d, dt, n, nq, ks, _ in SCAN_CASES:  # the float64 oracle stays within a few seconds
        assert nq * n * d <= 1.01e11, (fam, tile, d)
    dims = lambda fam, tile, dt="float16": sorted({c[2] for c in SCAN_CASES if c[0] == fam and c[1] == tile and c[3] == dt})
    every = [d for d, _, _ in SCAN_WIDTHS]
    assert all(dims("persistent", t) == every and dims("persistent", t, "bfloat16") == sorted(BF16_WIDTHS) for t in PERSISTENT)
    assert all(dims("small", t) == every for t in (1, 42, 46)) and dims("auto", 0) == sorted(AUTO_WIDTHS)
    assert all(dims("marker", t) == sorted(MARKER_WIDTHS) for t in (1, 8, 9, 14, 42, 46))


def test_integer_fixtures_are_exact_in_fp32_at_every_width():
    """Inputs lie in -8 .. 8: a dot product of `dim` terms is below 64 * dim in magnitude, and so is every partial sum in any order;
    integers below 2^24 are exact in fp32.  The marker rows hold one live column: a single product, below 2048 * 1024 = 2^21."""
    widths = {c[2] for c in SCAN_CASES} | {d for d, _ in EXACT_WIDTHS} | set(EXACT_INT_WIDTHS) | {TOP_DIM, EXACT_MAX_DIM}
    assert max(widths) == 16384
    for d in widths:
        assert 64 * d < 2 ** 24, d


def test_the_xt_step_restatement_on_the_shapes_checked_by_hand(plan):
    p = plan(24_000, 10, 2048, tile=14)
    assert p["passes"][0][0] == 2048 and xt_step(2048, 94) == 32
    p = plan(40_000, 10, 1024, tile=14)
    assert _filter_stages(p, 14) == (1024, [157]) and xt_step(1024, 157) == 64 and crossing_columns(157, 64) == 64
    assert kernels(p, GMAX) == {8} and p["perm"][0] > 1          # one bootstrap on kernel 8, one permuted whole-store FILTER stage on 14
    assert max(_filter_stages(plan(70_001, 64, 1024, tile=14), 14)[1]) > 64
    # shapes that do NOT qualify: a store of fewer tiles than the grid has columns (the grid shrinks to it); one query tile on 300 tiles
    assert xt_step(1024, 20) == 24 and crossing_columns(20, 24) == 0
    assert xt_step(256, 150) == 152 and xt_step(256, 300) == 256 and crossing_columns(300, 256) == 44
    assert crossing_columns(70, 64) == 6  # 6 of 64 columns: below a quarter
    assert _filter_stages(plan(24_000, 10, 1024, tile=14), 14) == (1024, [64, 30])  # one round of the grid and a tail: nothing crosses


@pytest.mark.parametrize("n,k,nq,tile,subset", _plan_keys(SCAN_CASES))
def test_every_gpu_shape_filters_on_its_kernel_and_crosses_tile_boundaries(plan, n, k, nq, tile, subset):
    p = plan(n, k, nq, tile=tile, subset=subset)
    if tile == 0:  # auto: a GMAX bootstrap on kernel 8, FILTER stages on the 8-phase kernel and / or the 128x128 one
        assert p["bn"] == 256 and kernels(p, GMAX) == {8} and kernels(p, FILTER) and kernels(p, FILTER) <= {1, 14}
        if nq == 1024:
            assert 14 in kernels(p, FILTER)
        return
    nq_pad, tiles = _filter_stages(p, tile)
    assert tiles, f"no FILTER stage on kernel {tile}: {p}"
    assert kernels(p, FILTER) == {tile}
    if tile in PERSISTENT and n > 5_000:  # (TOP_CASES: see the table)
        n_x = max(tiles)
        step = xt_step(nq_pad, n_x)
        assert n_x > step, (n_x, step)
        assert 4 * crossing_columns(n_x, step) >= step, (n_x, step)


def test_the_auto_cases_see_both_filter_kernels(plan):
    seen = set()
    for n, k, nq, tile, subset in _plan_keys([c for c in SCAN_CASES if c[0] == "auto"]):
        seen |= kernels(plan(n, k, nq, tile=tile), FILTER)
    assert seen == {1, 14}


def test_only_the_top_cases_are_exempt_from_the_crossing_check():
    assert [c[:2] for c in SCAN_CASES if c[1] in PERSISTENT and c[4] <= 5_000] == [("top", 14)]
