"""CPU-side checks of `remove_rows` (include/vodhip.h H2r):

* the host-only header vod_amd/csrc/remove_fold.h - the argument check, the slab plan against a brute-force simulation, the node
  index's segment plan - in a stand-alone program under AddressSanitizer + UBSan (tests/sanitize/remove_rows_check.cpp); nothing is
  loaded into Python under a sanitizer;
* the NumPy restatement (tests/remove_rows_ref.py) on hand-written lists;
* the Python argument handling (`remove_rows_args`): ids, range, mask -> ids, and the spellings that are refused;
* the symbols are declared in include/vodhip.h (which stays C99), listed in `_native.SIGNATURES` with as many arguments, and exported;
  both index classes expose the method.
"""
from __future__ import annotations

import inspect
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import remove_rows_ref as R
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


# ---- the host-only header under the sanitizers ------------------------------------------------------------------------------------
def test_planners_are_right_and_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([CLANG, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=600)
    if probed.returncode != 0:  # (decided on an empty program, before the program under test is built)
        pytest.skip("this toolchain does not link -fsanitize=address,undefined")
    exe = tmp_path / "remove_rows_check"
    cmd = [CLANG, *flags, str(ROOT / "tests" / "sanitize" / "remove_rows_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_pads_out_of_range_and_repeated_ids():
    keep, counts = R.resolve_removal(6, ids=[-1, 6, 0, -7, 2**40, 5, 0, 0])
    assert counts == (2, 4, 2) and np.array_equal(keep, [False, True, True, True, True, False])
    assert np.array_equal(R.new_ids(keep), [-1, 0, 1, 2, 3, -1])
    keep, counts = R.resolve_removal(6, ids=[-1, -1, 100])
    assert counts == (0, 3, 0) and keep.all()
    keep, counts = R.resolve_removal(6, ids=[99, 100, 105, 106, 100], id_base=100)
    assert counts == (2, 2, 1) and np.array_equal(np.flatnonzero(~keep), [0, 5])
    _, counts = R.resolve_removal(6, ids=[3], id_base=100)  # a non-negative id below id_base
    assert counts == (0, 1, 0)
    _, counts = R.resolve_removal(6, ids=[-1], id_base=-5)  # a negative id is a pad whatever id_base says
    assert counts == (0, 1, 0)


def test_the_range_form_and_the_map():
    keep, counts = R.resolve_removal(6, begin=2, n=3)
    assert counts == (3, 0, 0) and np.array_equal(R.new_ids(keep), [0, 1, -1, -1, -1, 2])
    keep, counts = R.resolve_removal(6, begin=6, n=0)
    assert counts == (0, 0, 0) and np.array_equal(R.new_ids(keep), np.arange(6))
    keep, counts = R.resolve_removal(6, begin=0, n=6)
    assert counts == (6, 0, 0) and (R.new_ids(keep) == -1).all()
    with pytest.raises(AssertionError):
        R.resolve_removal(6, begin=5, n=2)
    # the map is faiss's rule: a survivor's new id is its old id minus the removed rows below it
    rng = np.random.default_rng(0)
    keep = rng.random(1000) < 0.7
    m = R.new_ids(keep)
    below = np.concatenate([[0], np.cumsum(~keep)[:-1]])
    assert np.array_equal(m[keep], (np.arange(1000) - below)[keep]) and (m[~keep] == -1).all()


# ---- the Python argument handling -------------------------------------------------------------------------------------------------
def test_ids_range_and_mask_become_the_native_arguments():
    torch = pytest.importorskip("torch")
    from vod_amd.index import remove_rows_args

    ids, begin, n = remove_rows_args([5, 2, 2, -1], 0, None, None, 10)
    assert ids.dtype == np.int64 and ids.flags.c_contiguous and ids.tolist() == [5, 2, 2, -1] and (begin, n) == (0, 4)
    ids, begin, n = remove_rows_args(torch.tensor([[7], [1]], dtype=torch.int32), 0, None, None, 10)
    assert isinstance(ids, np.ndarray) and ids.dtype == np.int64 and ids.tolist() == [7, 1] and n == 2
    ids, begin, n = remove_rows_args(np.zeros(0, dtype=np.int64), 0, None, None, 10)
    assert ids.size == 0 and n == 0
    assert remove_rows_args(None, 3, 4, None, 10) == (None, 3, 4)
    assert remove_rows_args(None, 10, 0, None, 10) == (None, 10, 0)
    assert remove_rows_args(None, 0, 0, None, 0) == (None, 0, 0)
    mask = np.zeros(10, dtype=bool)
    mask[[9, 0, 4]] = True
    ids, begin, n = remove_rows_args(None, 0, None, mask, 10)
    assert ids.dtype == np.int64 and ids.tolist() == [0, 4, 9] and (begin, n) == (0, 3)
    ids, begin, n = remove_rows_args(None, 0, None, torch.from_numpy(mask), 10)
    assert isinstance(ids, np.ndarray) and ids.tolist() == [0, 4, 9] and n == 3
    ids, _, n = remove_rows_args(None, 0, None, np.zeros(10, dtype=bool), 10)
    assert ids.size == 0 and n == 0


def test_spellings_that_are_refused():
    pytest.importorskip("torch")
    from vod_amd.index import remove_rows_args

    with pytest.raises(ValueError, match="exactly one"):
        remove_rows_args([1], 0, 1, None, 10)  # ids together with a range
    with pytest.raises(ValueError, match="exactly one"):
        remove_rows_args([1], 2, None, None, 10)  # ids together with begin
    with pytest.raises(ValueError, match="exactly one"):
        remove_rows_args([1], 0, None, np.zeros(10, dtype=bool), 10)
    with pytest.raises(ValueError, match="exactly one"):
        remove_rows_args(None, 0, None, None, 10)
    with pytest.raises(ValueError, match="exactly one"):
        remove_rows_args(None, 3, None, None, 10)  # begin without n
    for begin, n in ((-1, 1), (4, 7), (11, 0), (0, -1)):
        with pytest.raises(ValueError, match="outside"):
            remove_rows_args(None, begin, n, None, 10)
    with pytest.raises(ValueError, match="boolean mask of length 10"):
        remove_rows_args(None, 0, None, np.zeros(9, dtype=bool), 10)
    with pytest.raises(ValueError, match="boolean mask"):
        remove_rows_args(None, 0, None, np.zeros(10, dtype=np.int64), 10)
    with pytest.raises(ValueError, match="boolean mask"):
        remove_rows_args(None, 0, None, np.zeros((2, 5), dtype=bool), 10)


# ---- the interface ------------------------------------------------------------------------------------------------------------------
DECLARED = {
    "vodhip_index_remove_rows": ["index", "ids", "row_begin", "n", "location", "id_base", "new_ids", "n_removed", "stream"],
    "vodhip_node_index_remove_rows": ["index", "ids", "row_begin", "n", "new_ids", "n_removed"],
    "vodhip_index_plane": ["index", "which", "dev_ptr", "n_rows", "row_stride_elems"],
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


def test_header_with_the_new_section_is_c99_and_update_no_longer_lists_removal_as_missing():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", str(ROOT / "include" / "vodhip.h")], check=True)
    header = (ROOT / "include" / "vodhip.h").read_text()
    assert "H2r." in header and "WAITS FOR THE DEVICE ONCE" in header and "remove_slab_rows" in header
    assert "NOT BUILT: removing rows" not in header


def test_both_indexes_expose_the_method():
    pytest.importorskip("torch")
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    for cls in (HipFlatIndex, HipNodeIndex):
        sig = inspect.signature(cls.remove_rows)
        assert list(sig.parameters) == ["self", "ids", "begin", "n", "mask", "return_map"]
        p = sig.parameters
        assert p["ids"].default is None and p["begin"].default == 0 and p["n"].default is None and p["mask"].default is None and p["return_map"].default is False


def test_the_kernel_file_is_built_and_has_its_scratch_check():
    make = (ROOT / "vod_amd" / "csrc" / "Makefile").read_text()
    assert "kernels_remove.hip" in make and "remove_fold.h" in make and re.search(r"^check-remove:", make, flags=re.M)
    src = (ROOT / "vod_amd" / "csrc" / "kernels_remove.hip").read_text()
    assert "__launch_bounds__(256) void remove_gather_kernel" in src
    assert "DESIGN.md" in (ROOT / "include" / "vodhip.h").read_text() and "Row removal" in (ROOT / "DESIGN.md").read_text()
