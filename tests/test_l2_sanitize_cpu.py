"""The bias split of an L2 store (vod_amd/csrc/l2_bias.h and the host side of vod_amd/csrc/kernels_l2.hip) under AddressSanitizer and
UndefinedBehaviorSanitizer: the two files are compiled as HOST C++ into the stand-alone tests/sanitize/l2_split_check.cpp, which sweeps
the split for both store dtypes on the CPU.  Nothing is loaded into Python; any sanitizer report fails the test."""
import pathlib
import subprocess

import pytest

from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_l2_split_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "l2_split_check"
    csrc = ROOT / "vod_amd" / "csrc"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-x", "c++", str(csrc / "kernels_l2.hip"), str(ROOT / "tests" / "sanitize" / "l2_split_check.cpp"),
           "-I", str(ROOT / "include"), "-I", str(csrc), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if built.returncode != 0 and "sanitizer" in built.stderr.lower() and "unsupported" in built.stderr.lower():
        pytest.skip("-fsanitize=address,undefined is not supported by this toolchain")
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]
