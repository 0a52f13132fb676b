"""CPU-side checks of `update_rows` / `add_to_rows` (include/vodhip.h H2u):

* the NumPy restatement (tests/update_rows_ref.py) on hand-written lists: which slot writes, what is skipped, what counts as a
  duplicate, and the two-rounding float32 ADD;
* the host-only header vod_amd/csrc/update_fold.h - the argument check, the routing of a node call's slots, the dense split - in a
  stand-alone program under AddressSanitizer + UBSan (tests/sanitize/update_rows_check.cpp); nothing is loaded into Python under a
  sanitizer;
* the two symbols are declared in include/vodhip.h (which stays C99), listed in `_native.SIGNATURES` with as many arguments, and
  exported; both index classes expose both methods.
"""
from __future__ import annotations

import inspect
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import update_rows_ref as R
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def _x(n=6, dim=3):
    return np.arange(n * dim, dtype=np.float32).reshape(n, dim)


def test_three_slots_with_one_id_the_last_wins():
    rows = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3]], dtype=np.float32)
    out, counts = R.apply_update(_x(), rows, ids=[4, 4, 4])
    assert counts == (1, 0, 2)
    want = _x()
    want[4] = 3
    assert np.array_equal(out, want)
    byhand = _x()
    byhand[[4, 4, 4]] = rows  # NumPy's own rule for x[ids] = rows
    assert np.array_equal(out, byhand)


def test_all_slots_with_one_id():
    rows = np.arange(257 * 3, dtype=np.float32).reshape(257, 3)
    out, counts = R.apply_update(_x(), rows, ids=np.full(257, 2))
    assert counts == (1, 0, 256)
    assert np.array_equal(out[2], rows[256]) and np.array_equal(np.delete(out, 2, 0), np.delete(_x(), 2, 0))
    # ADD applies the last slot ONLY - not the sum of the slots
    out, counts = R.apply_update(_x(), rows, ids=np.full(257, 2), mode="add", alpha=0.5)
    assert counts == (1, 0, 256) and np.array_equal(out[2], _x()[2] + np.float32(0.5) * rows[256])


def test_pads_and_ids_below_and_above_the_range_are_skipped():
    rows = np.full((6, 3), 9, dtype=np.float32)
    out, counts = R.apply_update(_x(), rows, ids=[-1, 6, 0, -7, 2**40, 5])
    assert counts == (2, 4, 0)
    want = _x()
    want[[0, 5]] = 9
    assert np.array_equal(out, want)
    out, counts = R.apply_update(_x(), rows[:3], ids=[-1, -1, 100])
    assert counts == (0, 3, 0) and np.array_equal(out, _x())


def test_id_base_shifts_the_window():
    rows = np.full((5, 3), 9, dtype=np.float32)
    winner, counts = R.resolve_slots([99, 100, 105, 106, 100], ntotal=6, id_base=100)
    assert winner == {0: 4, 5: 2} and counts == (2, 2, 1)
    out, counts = R.apply_update(_x(), rows, ids=[99, 100, 105, 106, 100], id_base=100)
    assert counts == (2, 2, 1) and np.array_equal(np.flatnonzero((out != _x()).any(axis=1)), [0, 5])
    _, counts = R.resolve_slots([3], ntotal=6, id_base=100)  # a non-negative id below id_base
    assert counts == (0, 1, 0)
    _, counts = R.resolve_slots([-1], ntotal=6, id_base=-5)  # a negative id is a pad whatever id_base says
    assert counts == (0, 1, 0)


def test_the_empty_list_and_the_dense_form():
    out, counts = R.apply_update(_x(), np.zeros((0, 3), dtype=np.float32), ids=[])
    assert counts == (0, 0, 0) and np.array_equal(out, _x())
    out, counts = R.apply_update(_x(), np.zeros((0, 3), dtype=np.float32), begin=6)
    assert counts == (0, 0, 0) and np.array_equal(out, _x())
    rows = np.full((2, 3), 7, dtype=np.float32)
    out, counts = R.apply_update(_x(), rows, begin=4)
    assert counts == (2, 0, 0) and np.array_equal(out[4:], rows) and np.array_equal(out[:4], _x()[:4])
    with pytest.raises(AssertionError):
        R.apply_update(_x(), rows, begin=5)


def test_add_is_two_float32_roundings_not_a_fused_multiply_add():
    # alpha * d is rounded before the sum: 3e-4f * 3 = 9.0000004e-4 in float32; fused, the exact product would enter the sum
    alpha, d, x0 = np.float32(3e-4), np.float32(3.0), np.float32(1.0)
    out, _ = R.apply_update(np.array([[x0]]), np.array([[d]]), begin=0, mode="add", alpha=float(alpha))
    p = np.float32(alpha * d)
    assert out.dtype == np.float32 and out[0, 0] == np.float32(x0 + p)
    # over many values the two forms differ somewhere
    rng = np.random.default_rng(0)
    a = rng.standard_normal(200000).astype(np.float32)
    c = rng.standard_normal(200000).astype(np.float32)
    two = c + np.float32(0.7) * a  # (NumPy rounds every float32 operation)
    assert two.dtype == np.float32
    ref, _ = R.apply_update(c[:, None], a[:, None], begin=0, mode="add", alpha=0.7)
    assert np.array_equal(ref[:, 0], two)
    fused = (c.astype(np.float64) + np.float64(np.float32(0.7)) * a.astype(np.float64)).astype(np.float32)
    assert (fused != ref[:, 0]).any()  # the restatement is not the fused form
    # the input is not modified, and a float16 source is widened exactly
    x = _x()
    R.apply_update(x, np.ones((6, 3), dtype=np.float16), begin=0, mode="add")
    assert np.array_equal(x, _x())


# ---- the host-only header under the sanitizers ------------------------------------------------------------------------------------
def test_host_pieces_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([CLANG, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=600)
    if probed.returncode != 0:  # (decided on an empty program, before the program under test is built)
        pytest.skip("this toolchain does not link -fsanitize=address,undefined")
    exe = tmp_path / "update_rows_check"
    cmd = [CLANG, *flags, str(ROOT / "tests" / "sanitize" / "update_rows_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


# ---- the interface ------------------------------------------------------------------------------------------------------------------
DECLARED = {
    "vodhip_index_update_rows": ["index", "ids", "row_begin", "rows", "n", "src_dtype", "location", "mode", "alpha", "id_base", "stream"],
    "vodhip_node_index_update_rows": ["index", "ids", "row_begin", "rows", "n", "src_dtype", "mode", "alpha"],
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


def test_header_with_the_new_section_is_c99():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", str(ROOT / "include" / "vodhip.h")], check=True)
    header = (ROOT / "include" / "vodhip.h").read_text()
    assert "H2u." in header
    assert re.search(r"#define\s+VODHIP_UPDATE_SET\s+0\b", header) and re.search(r"#define\s+VODHIP_UPDATE_ADD\s+1\b", header)
    from vod_amd import _native

    assert (_native.UPDATE_SET, _native.UPDATE_ADD) == (0, 1)


def test_both_indexes_expose_both_methods():
    pytest.importorskip("torch")
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    for cls in (HipFlatIndex, HipNodeIndex):
        sig = inspect.signature(cls.update_rows)
        assert list(sig.parameters) == ["self", "vectors", "ids", "begin"]
        assert sig.parameters["ids"].default is None and sig.parameters["begin"].default == 0
        sig = inspect.signature(cls.add_to_rows)
        assert list(sig.parameters) == ["self", "delta", "alpha", "ids", "begin", "check"]
        assert sig.parameters["alpha"].default == 1.0 and sig.parameters["check"].default is True
    doc = HipFlatIndex.add_to_rows.__doc__
    assert "half an ulp" in doc and "exact_f32" in doc and "update_rows(keys)" in doc


def test_integration_guide_no_longer_re_ingests_after_a_step():
    text = (ROOT / "INTEGRATION.md").read_text()
    assert "index.reset(); index.add(...)" not in text
    assert "index.update_rows(keys.detach())" in text and "index.add_to_rows(keys.grad, alpha=-lr)" in text
