"""The rank calls (`rank_ids`, `count_above`), the parts that need no GPU:

* the NumPy restatement (tests/rank_ref.py) against a plain stable sort by (score desc, id asc), on random and on heavily tied data,
  with NaN rows, both zeros, infinities and a subset: the ranks of the eligible rows are a permutation of 0 .. n_eligible - 1;
* `count` against hand-made thresholds (strict, with tie ids, NaN, +-inf, -0.0 against +0.0) and `id_base`;
* `rank_metrics` on hand-made ranks;
* the host folds of a node index (vod_amd/csrc/rank_fold.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
  program (tests/sanitize/rank_fold_check.cpp); nothing is loaded into Python under a sanitizer;
* the five new symbols are declared in include/vodhip.h with the documented parameters, listed in `_native.SIGNATURES` with as many
  arguments, and exported by the built library.
"""
import math
import pathlib
import re
import subprocess

import numpy as np
import pytest

import rank_ref as R
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _random_scores(seed, nq, n, tied):
    rng = np.random.default_rng(seed)
    if tied:
        return rng.integers(-3, 4, size=(nq, n)).astype(np.float32)  # 7 values: hundreds of ties each
    return rng.standard_normal((nq, n)).astype(np.float32)


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("n", [1, 2, 257, 700])
def test_restatement_matches_a_plain_sort(n, tied):
    s = _random_scores(n, 5, n, tied)
    ids = np.broadcast_to(np.arange(n, dtype=np.int64), s.shape)
    rank, score = R.rank_ids(s, ids)
    np.testing.assert_array_equal(rank, R.ranks_by_argsort(s))
    np.testing.assert_array_equal(score.view(np.uint32), s.view(np.uint32))
    for q in range(len(s)):
        assert sorted(rank[q]) == list(range(n))  # a permutation
    # the order the ranks describe is (score desc, id asc)
    order = np.argsort(rank, axis=1)
    sorted_s = np.take_along_axis(s, order, axis=1)
    assert (np.diff(sorted_s, axis=1) <= 0).all()
    same = np.diff(sorted_s, axis=1) == 0
    assert (np.diff(order, axis=1)[same] > 0).all()


def test_restatement_zeros_nan_infinities_subset_and_id_base():
    s = np.array([[0.0, -0.0, 1.0, np.nan, -np.inf, np.inf, -0.0, 0.0, -2.0]], dtype=np.float32)
    n = s.shape[1]
    ids = np.arange(n, dtype=np.int64)[None]
    rank, score = R.rank_ids(s, ids)
    # +inf, 1, the four zeros in id order (the two signs are equal), -2, -inf; the NaN row is never ranked and never counted
    np.testing.assert_array_equal(rank, [[2, 3, 1, -1, 7, 0, 4, 5, 6]])
    assert np.isnan(score[0, 3]) and np.signbit(score[0, 1]) and not np.signbit(score[0, 0])
    np.testing.assert_array_equal(rank, R.ranks_by_argsort(s))
    # a subset: the rank is among the eligible rows, a target outside it is absent
    elig = np.array([[True, False, True, True, True, False, True, False, True]])
    rank, score = R.rank_ids(s, ids, eligible=elig)
    np.testing.assert_array_equal(rank, [[1, -1, 0, -1, 4, -1, 2, -1, 3]])
    assert np.isneginf(score[0, [1, 5, 7]]).all()
    np.testing.assert_array_equal(rank, R.ranks_by_argsort(s, elig))
    # id_base, absent slots (negative, below the base, past the end) and duplicates
    lst = np.array([[1002, 1002, -1, 999, 1009, 1008, 2]], dtype=np.int64)
    rank, score = R.rank_ids(s, lst, id_base=1000)
    np.testing.assert_array_equal(rank, [[1, 1, -1, -1, -1, 6, -1]])
    np.testing.assert_array_equal(score, np.array([[1.0, 1.0, -np.inf, -np.inf, -np.inf, -2.0, -np.inf]], dtype=np.float32))


def test_count_thresholds():
    s = np.array([[3.0, 1.0, 1.0, 0.0, -0.0, -1.0, np.nan, 1.0]], dtype=np.float32)
    thr = np.array([[1.0, 0.5, -0.0, 0.0, np.inf, -np.inf, np.nan, 3.0, 4.0]], dtype=np.float32)
    np.testing.assert_array_equal(R.count(s, thr), [[1, 4, 4, 4, 0, 7, -1, 0, 0]])
    tie = np.array([[2, 0, 4, 100, 0, 100, 0, 1, 0]], dtype=np.int64)
    # 1.0 with tie id 2: row 1 ties below it; -0.0 with tie id 4: row 3 (+0.0) ties below it; 0.0 with tie id 100: both zeros
    np.testing.assert_array_equal(R.count(s, thr, tie), [[2, 4, 5, 6, 0, 7, -1, 1, 0]])
    np.testing.assert_array_equal(R.count(s, thr, tie + 50, id_base=50), R.count(s, thr, tie))
    # count_above(q, score, tie_ids=ids) is rank_ids(q, ids).rank on the present, non-NaN slots
    ids = np.array([[0, 1, 2, 3, 4, 5, 7]], dtype=np.int64)
    rank, score = R.rank_ids(s, ids)
    np.testing.assert_array_equal(R.count(s, score, ids), rank)


def test_rank_metrics_on_hand_made_ranks():
    torch = pytest.importorskip("torch")
    from vod_amd.index import rank_metrics

    rank = torch.tensor([[0, 7, -1], [4, -1, 2], [-1, -1, -1], [150, 99, 3000]])
    got = rank_metrics(rank)
    # best present slot per query: 0, 2, (none), 99
    assert got["mrr"] == pytest.approx((1.0 + 1.0 / 3.0 + 1.0 / 100.0) / 3.0, rel=1e-12)
    assert got["hit@1"] == pytest.approx(1 / 3) and got["hit@5"] == pytest.approx(2 / 3)
    assert got["hit@20"] == pytest.approx(2 / 3) and got["hit@100"] == pytest.approx(1.0)
    present = [0, 7, 4, 2, 150, 99, 3000]
    assert got["mean_rank"] == pytest.approx(sum(present) / len(present))
    assert got["median_rank"] == 7.0
    assert set(got) == {"mrr", "hit@1", "hit@5", "hit@20", "hit@100", "mean_rank", "median_rank"}
    one = rank_metrics(torch.tensor([3, -1, 0]), ks=(1, 4))  # [nq]: one slot per query
    assert one == {"mrr": pytest.approx((0.25 + 1.0) / 2), "hit@1": 0.5, "hit@4": 1.0, "mean_rank": 1.5, "median_rank": 0.0}
    none = rank_metrics(torch.full((2, 2), -1))
    assert all(math.isnan(v) for v in none.values()) and set(none) == set(got)
    assert rank_metrics(np.array([[9223372036854775000, -1]]))["mean_rank"] == pytest.approx(9.223372036854775e18)


def test_shard_folds_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "rank_fold_check"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "sanitize" / "rank_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
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
    "vodhip_index_count_above": ["index", "queries", "q_dtype", "nq", "thresholds_dev", "tie_ids_dev", "m", "id_base", "q_labels_dev",
                                 "n_per_query", "out_counts", "stream"],
    "vodhip_index_rank_ids": ["index", "queries", "q_dtype", "nq", "ids_dev", "m", "id_base", "q_labels_dev", "n_per_query", "out_ranks",
                              "out_scores", "stream"],
    "vodhip_index_scan_score_ids": ["index", "queries", "q_dtype", "nq", "ids_dev", "m", "id_base", "q_labels_dev", "n_per_query",
                                    "out_scores", "out_rows", "stream"],
    "vodhip_node_index_rank_ids": ["index", "queries", "q_dtype", "nq", "ids", "m", "q_labels", "n_per_query", "out_ranks", "out_scores"],
    "vodhip_node_index_count_above": ["index", "queries", "q_dtype", "nq", "thresholds", "tie_ids", "m", "q_labels", "n_per_query",
                                      "out_counts"],
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
    assert "#define VODHIP_RANK_MAX_LISTED 64" in header
