"""`posterior_expectation`, the parts that need no GPU:

* the float64 restatement (tests/readout_ref.py) against a direct float64 softmax on small cases: a column of ones reads exactly the
  total mass (1 for live queries, 0 for dead ones), the masses of a one-hot label table add up to 1, subset masks, NaN rows, a +inf
  score, an empty store;
* the derived bound is non-negative and finite, and it states the group size of the header;
* the host pieces of a node index (vod_amd/csrc/readout_fold.h: argument checks, the shard split of the table, the fold) under
  AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (tests/sanitize/readout_fold_check.cpp); nothing is
  loaded into Python under a sanitizer;
* the new symbols are declared in include/vodhip.h, listed in `_native.SIGNATURES` with as many arguments, and exported;
* both indexes expose the three methods.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import readout_ref as R
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _softmax_readout(q, x, v, beta, eligible=None):
    """the definition, one query at a time, on values that fp16 and bf16 hold exactly"""
    out = np.zeros((len(q), v.shape[1]))
    for i in range(len(q)):
        s = x.astype(np.float64) @ q[i].astype(np.float64)
        keep = ~np.isnan(s)
        if eligible is not None:
            keep &= eligible[i]
        if not keep.any() or np.isposinf(s[keep]).any() or np.isneginf(s[keep]).all():
            continue
        w = np.exp(beta * (s[keep] - s[keep].max()))
        out[i] = (w / w.sum()) @ v[keep].astype(np.float64)
    return out


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("beta", [1.0, 1.0 / 64.0, 4.0])
def test_restatement_agrees_with_a_direct_softmax(beta, dtype):
    rng = np.random.default_rng(3)
    x = rng.integers(-8, 9, size=(700, 9)).astype(np.float32)
    q = rng.integers(-8, 9, size=(21, 9)).astype(np.float32)
    v = rng.integers(-8, 9, size=(700, 70)).astype(np.float32)
    x[11, 2] = np.nan  # a NaN row is left out
    elig = rng.random((21, 700)) < 0.5
    elig[4] = False    # a dead query
    for e in (None, elig):
        got, m, r = R.posterior_expectation(q, x, v, dtype, beta, e)
        want = _softmax_readout(q, x, v, beta, e)
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
        dead = ~np.isfinite(m)
        assert (got[dead] == 0).all()
        assert np.array_equal(dead, (np.arange(21) == 4) if e is not None else np.zeros(21, dtype=bool))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_a_column_of_ones_reads_the_total_mass_and_one_hot_masses_add_up_to_one(dtype):
    rng = np.random.default_rng(4)
    x = rng.integers(-8, 9, size=(500, 5)).astype(np.float32)
    q = rng.integers(-8, 9, size=(12, 5)).astype(np.float32)
    elig = np.ones((12, 500), dtype=bool)
    elig[3] = False
    ones = np.ones((500, 1), dtype=np.float32)
    got, m, _ = R.posterior_expectation(q, x, ones, dtype, 0.25, elig)
    live = np.isfinite(m)
    assert (~live == (np.arange(12) == 3)).all()
    np.testing.assert_allclose(got[live, 0], 1.0, rtol=0, atol=1e-14)
    assert (got[~live] == 0).all()  # exactly the total mass: 1 for live queries, 0 for dead ones
    cls = rng.integers(0, 7, size=500)
    table = np.eye(7, dtype=np.float32)[cls]
    mass, _, _ = R.posterior_expectation(q, x, table, dtype, 0.25, elig)
    np.testing.assert_allclose(mass[live].sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert (mass >= 0).all() and (mass[~live] == 0).all()
    np.testing.assert_allclose(mass, _softmax_readout(q, x, table, 0.25, elig), rtol=1e-12, atol=1e-14)


def test_infinite_scores_an_empty_store_and_a_vector_table():
    x = np.array([[1.0, 0.0], [np.inf, 0.0], [2.0, 1.0]], dtype=np.float32)
    q = np.array([[1.0, 0.0], [-1.0, 0.0]], dtype=np.float32)
    v = np.array([1.0, 2.0, 3.0], dtype=np.float32)  # a vector is one column
    got, m, r = R.posterior_expectation(q, x, v, "bfloat16", 1.0)  # (the fp16 restatement saturates an infinite input)
    assert np.isposinf(m[0]) and (got[0] == 0).all()       # a +inf score: the zero row
    s = np.array([-1.0, -2.0])                              # query 1: row 1 scores -inf and carries no weight
    w = np.exp(s - s.max())
    np.testing.assert_allclose(got[1, 0], (w / w.sum()) @ np.array([1.0, 3.0]), rtol=1e-14)
    got, m, r = R.posterior_expectation(q, x[:0], np.zeros((0, 4), dtype=np.float32), "float16", 1.0)
    assert got.shape == (2, 4) and (got == 0).all() and np.isneginf(m).all() and np.isneginf(r).all()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("dot", [False, True])
def test_bound_is_non_negative_and_finite(dot, dtype):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3000, 33)).astype(np.float32)
    q = rng.standard_normal((17, 33)).astype(np.float32)
    v = rng.standard_normal((3000, 5)).astype(np.float32)
    v[:, 4] = 0  # a column of zeros: the bound may be 0 there, not negative
    for beta in (1.0, 1.0 / 64.0, 4.0):
        b = R.device_bound(q, x, v, dtype, beta, dot=dot)
        assert b.shape == (17, 5) and np.isfinite(b).all() and (b >= 0).all() and (b[:, :4] > 0).all()
        assert (R.rel_bound(q, x, dtype, beta, 3000, 3000, dot=dot) >= R.EPS16[dtype]).all()
    elig = np.zeros((17, 3000), dtype=bool)
    assert np.isfinite(R.device_bound(q, x, v, dtype, 1.0, elig, dot=dot)).all()


def test_reference_group_size_is_the_headers():
    text = (ROOT / "include" / "vodhip.h").read_text()
    assert int(re.search(r"#define VODHIP_READOUT_GROUP_ROWS (\d+)", text).group(1)) == R.GROUP_ROWS
    assert R.GROUP_ROWS % R.TILE_ROWS == 0 and R.GROUP_TILES >= 1
    assert int(re.search(r"#define VODHIP_READOUT_MAX_COLS (\d+)", text).group(1)) == 256


def test_host_pieces_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([CLANG, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=600)
    if probed.returncode != 0:  # (decided on an empty program, before the program under test is built)
        pytest.skip("this toolchain does not link -fsanitize=address,undefined")
    exe = tmp_path / "readout_fold_check"
    cmd = [CLANG, *flags, str(ROOT / "tests" / "sanitize" / "readout_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


DECLARED = {
    "vodhip_index_set_row_values": ["index", "values", "n_rows", "n_cols", "src_dtype", "location", "stream"],
    "vodhip_index_row_values_info": ["index", "n_rows", "n_cols"],
    "vodhip_index_posterior_expectation": ["index", "queries", "q_dtype", "nq", "beta", "q_labels_dev", "n_per_query", "out_max", "out_log_rel",
                                           "out_values", "stream"],
    "vodhip_node_index_set_row_values": ["index", "values", "n_rows", "n_cols", "src_dtype"],
    "vodhip_node_index_row_values_info": ["index", "n_rows", "n_cols"],
    "vodhip_node_index_posterior_expectation": ["index", "queries", "q_dtype", "nq", "beta", "q_labels", "n_per_query", "out_max", "out_log_rel",
                                                "out_values"],
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


def test_both_indexes_expose_the_three_methods():
    pytest.importorskip("torch")
    from vod_amd.index import HipFlatIndex, HipNodeIndex, PosteriorExpectation

    for cls in (HipFlatIndex, HipNodeIndex):
        assert callable(cls.set_row_values) and callable(cls.posterior_expectation)
        assert isinstance(cls.row_values_shape, property)
    assert PosteriorExpectation._fields == ("values", "log_partition")
