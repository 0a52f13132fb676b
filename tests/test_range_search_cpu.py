"""`range_search`, the parts that need no GPU:

* the NumPy restatement (tests/range_ref.py) against a plain loop, on random and on heavily tied data (7 distinct values) with NaN rows,
  both zeros, infinities, a subset, `id_base`, NaN / -inf / +inf thresholds, tie ids below, inside and past the store, and `inclusive`;
  its list lengths equal `rank_ref.count` in every case;
* the nibble interleave of the kernel: a pure-Python model of `scan_lane_row` shows that the 64-bit mask built from the two lane
  halves' masks is in row order for all 64 rows of a wave;
* the `order="score"` re-sort on a hand-made segment with ties and `-0.0`;
* the host fold of a node index (vod_amd/csrc/range_fold.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
  program (tests/sanitize/range_fold_check.cpp); nothing is loaded into Python under a sanitizer;
* both symbols are declared in include/vodhip.h, listed in `_native.SIGNATURES` with as many arguments, and exported;
* the Python refusals that need no index.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import range_ref as G
import rank_ref as R
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
INF = np.float32(np.inf)


def _plain_loop(s, t, tie, elig, id_base, inclusive):
    """R(q) by the definition, one (query, row) pair at a time, on Python floats (no `key`)"""
    lims, scores, ids = [0], [], []
    for q in range(s.shape[0]):
        for z in range(s.shape[1]):
            v, th = float(s[q, z]), float(t[q])
            if v != v or th != th or (elig is not None and not elig[q, z]):
                continue
            take = v > th  # (Python floats: -0.0 == 0.0, as the keys)
            if v == th:
                take = inclusive or (tie is not None and id_base + z < int(tie[q]))
            if take:
                scores.append(s[q, z])
                ids.append(id_base + z)
        lims.append(len(ids))
    return np.array(lims, dtype=np.int64), np.array(scores, dtype=np.float32), np.array(ids, dtype=np.int64)


def _data(seed, nq, n, tied):
    rng = np.random.default_rng(seed)
    s = rng.integers(-3, 4, size=(nq, n)).astype(np.float32) if tied else rng.standard_normal((nq, n)).astype(np.float32)
    special = [np.nan, 0.0, -0.0, INF, -INF, np.nan, -0.0, 0.0]
    for q in range(nq):  # NaN rows, both zeros, both infinities at random places of every query
        at = rng.choice(n, size=min(n, len(special)), replace=False)
        s[q, at] = np.array(special[: len(at)], dtype=np.float32)
    return rng, s


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    np.testing.assert_array_equal(a[2], b[2])


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("n", [1, 9, 257, 700])
def test_restatement_matches_a_plain_loop_and_the_rank_counts(n, tied):
    nq = 12
    rng, s = _data(100 + n, nq, n, tied)
    elig = rng.random((nq, n)) < 0.7
    # thresholds: scores that occur (ties), values between scores, NaN, -inf, +inf, both zeros
    thr = s[np.arange(nq), rng.integers(0, n, size=nq)].copy()
    thr[np.isnan(thr)] = 0.5
    thr[0], thr[1], thr[2], thr[3], thr[4], thr[5] = np.nan, -INF, INF, -0.0, 0.0, 0.5
    for id_base in (0, 1000):
        # tie ids below the store, inside it, on its last row and past it
        tie = id_base + rng.integers(0, n, size=nq).astype(np.int64)
        tie[6], tie[7], tie[8], tie[9] = id_base - 5, id_base, id_base + n - 1, id_base + n + 7
        for subset in (None, elig):
            for ties, inclusive in ((None, False), (tie, False), (None, True)):
                got = G.range_search(s, thr, ties, subset, id_base, inclusive)
                _same(got, _plain_loop(s, thr, ties, subset, id_base, inclusive))
                count_ties = np.full((nq,), G.TIE_PAST_EVERY_ROW) if inclusive else ties
                cnt = R.count(s, thr[:, None], None if count_ties is None else count_ties[:, None], subset, id_base)[:, 0]
                np.testing.assert_array_equal(np.diff(got[0]), np.where(cnt < 0, 0, cnt))
                for q in range(nq):  # ascending ids within a query
                    assert (np.diff(got[2][got[0][q]:got[0][q + 1]]) > 0).all()
    # the thresholds that select nothing / everything above -inf
    lims = G.range_search(s, thr)[0]
    assert lims[1] - lims[0] == 0 and lims[3] - lims[2] == 0
    assert lims[2] - lims[1] == (~np.isnan(s[1]) & (s[1] > -INF)).sum()


def scan_lane_row(rlane, bit):
    """store_scan.h"""
    return rlane + (bit >> 4) * 32 + (bit & 3) + 8 * ((bit & 15) >> 2)


def spread_nibbles(x):
    x = (x | (x << 8)) & 0x00FF00FF
    return (x | (x << 4)) & 0x0F0F0F0F


def row_order(h0, h1):
    """range_row_order of kernels_range.hip"""
    lo = spread_nibbles(h0 & 0xFFFF) | (spread_nibbles(h1 & 0xFFFF) << 4)
    hi = spread_nibbles(h0 >> 16) | (spread_nibbles(h1 >> 16) << 4)
    return lo | (hi << 32)


def test_nibble_interleave_puts_the_two_lane_masks_in_row_order():
    # one row at a time: bit `b` of lane half `h` is row scan_lane_row(4 h, b) of the wave's 64, and lands on that bit of the 64-bit mask
    seen = set()
    for h in (0, 1):
        for b in range(32):
            row = scan_lane_row(4 * h, b)
            assert 0 <= row < 64
            masks = [0, 0]
            masks[h] = 1 << b
            assert row_order(masks[0], masks[1]) == 1 << row
            # the position the emit pass computes for the bit: 32 i + 8 (r >> 2) + 4 h + (r & 3)
            i, r = b >> 4, b & 15
            assert 32 * i + 8 * (r >> 2) + 4 * h + (r & 3) == row
            seen.add(row)
    assert seen == set(range(64))
    # and random pairs of masks: the union of their rows, nothing else
    rng = np.random.default_rng(5)
    for _ in range(200):
        h0, h1 = (int(v) for v in rng.integers(0, 1 << 32, size=2, dtype=np.uint64))
        want = 0
        for h, m in ((0, h0), (1, h1)):
            for b in range(32):
                if (m >> b) & 1:
                    want |= 1 << scan_lane_row(4 * h, b)
        assert row_order(h0, h1) == want


def test_order_score_resorts_every_segment_with_ties_and_negative_zero():
    torch = pytest.importorskip("torch")
    from vod_amd.index import RangeResult, sort_range_by_score

    lims = np.array([0, 7, 7, 10], dtype=np.int64)
    scores = np.array([0.0, 2.0, -0.0, 2.0, -1.0, 0.0, -np.inf, 5.0, 1.0, 5.0], dtype=np.float32)
    ids = np.array([3, 4, 8, 9, 11, 12, 40, 2, 6, 7], dtype=np.int64)
    want_ids = [4, 9, 3, 8, 12, 11, 40, 2, 7, 6]
    want_scores = np.array([2.0, 2.0, 0.0, -0.0, 0.0, -1.0, -np.inf, 5.0, 5.0, 1.0], dtype=np.float32)
    got = sort_range_by_score(RangeResult(lims, scores, ids))  # NumPy in, NumPy out
    assert isinstance(got.ids, np.ndarray)
    np.testing.assert_array_equal(got.ids, want_ids)
    np.testing.assert_array_equal(got.scores.view(np.uint32), want_scores.view(np.uint32))  # the -0.0 keeps its sign and its id
    got_t = sort_range_by_score(RangeResult(torch.from_numpy(lims), torch.from_numpy(scores), torch.from_numpy(ids)))
    np.testing.assert_array_equal(got_t.ids.numpy(), want_ids)
    ref_s, ref_i = G.sort_by_score(lims, scores, ids)
    np.testing.assert_array_equal(ref_i, want_ids)
    np.testing.assert_array_equal(ref_s.view(np.uint32), want_scores.view(np.uint32))
    empty = sort_range_by_score(RangeResult(np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)))
    assert empty.ids.shape == (0,)


def test_shard_fold_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "range_fold_check"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "sanitize" / "range_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if built.returncode != 0 and "sanitizer" in built.stderr.lower() and "unsupported" in built.stderr.lower():
        pytest.skip("-fsanitize=address,undefined is not supported by this toolchain")
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


DECLARED = {
    "vodhip_index_range_search": ["index", "queries", "q_dtype", "nq", "thresholds_dev", "tie_ids_dev", "id_base", "q_labels_dev", "n_per_query",
                                  "lims_dev", "out_scores_dev", "out_ids_dev", "capacity", "stream"],
    "vodhip_node_index_range_search": ["index", "queries", "q_dtype", "nq", "thresholds", "tie_ids", "q_labels", "n_per_query", "lims",
                                       "out_scores", "out_ids", "capacity"],
}


@pytest.mark.parametrize("name", sorted(DECLARED))
def test_symbols_are_declared_listed_and_exported(name):
    from vod_amd import _native

    header = (ROOT / "include" / "vodhip.h").read_text()
    found = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert found, name
    params = [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", found.group(1), flags=re.S).split(",")]
    assert params == DECLARED[name]
    restype, argtypes = _native.SIGNATURES[name]
    assert len(argtypes) == len(params)
    assert hasattr(_native.load_library(), name)


def test_python_refusals_that_need_no_index():
    pytest.importorskip("torch")
    from vod_amd.index import HipFlatIndex, HipNodeIndex, check_range_args

    check_range_args(5, (5,), None, False, None, "id")
    check_range_args(5, (5,), (5,), False, 0, "score")
    check_range_args(0, (0,), None, True, 7, "id")
    with pytest.raises(ValueError, match="thresholds of shape"):
        check_range_args(5, (5, 1), None, False, None, "id")
    with pytest.raises(ValueError, match="thresholds of shape"):
        check_range_args(5, (4,), None, False, None, "id")
    with pytest.raises(ValueError, match="tie_ids of shape"):
        check_range_args(5, (5,), (5, 1), False, None, "id")
    with pytest.raises(ValueError, match="inclusive"):
        check_range_args(5, (5,), (5,), True, None, "id")
    with pytest.raises(ValueError, match="order must be"):
        check_range_args(5, (5,), None, False, None, "rank")
    with pytest.raises(ValueError, match="max_results"):
        check_range_args(5, (5,), None, False, -1, "id")
    for cls in (HipFlatIndex, HipNodeIndex):
        for method in ("range_search", "outranking", "posterior_support"):
            assert callable(getattr(cls, method))
