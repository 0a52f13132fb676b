"""`log_partition`, the parts that need no GPU:

* the float64 restatement (tests/partition_ref.py) equals a naive float64 log(sum(exp)) on small inputs, 0 <= log_rel <= log n, a one-row
  store gives log_rel == 0, eligibility / NaN / +inf / no row behave as the contract states;
* the derived device bound grows with n, with the width and with beta;
* `topk_log_coverage` on CPU tensors: 0 within float32 rounding of the two sums when k >= n, strictly negative with fewer rows, pads drop out;
* the host fold of per-shard pairs (vod_amd/csrc/partition_fold.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
  program (tests/sanitize/partition_fold_check.cpp); nothing is loaded into Python under a sanitizer;
* both new symbols are declared in include/vodhip.h and listed in `_native.SIGNATURES`.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import partition_ref as P
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _small(seed, n, d, nq=7, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((nq, d))).astype(np.float32), (scale * rng.standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("n,d,beta", [(1, 3, 1.0), (5, 1, 4.0), (37, 16, 0.25), (300, 65, 1.0)])
def test_restatement_matches_naive_float64(n, d, beta, dtype):
    q, x = _small(n + d, n, d)
    m, r = P.log_partition(q, x, dtype, beta)
    s = P.scores(q, x, dtype)
    naive = np.log(np.exp(beta * s).sum(axis=1))  # (small inputs: no overflow)
    np.testing.assert_allclose(beta * m + r, naive, rtol=0, atol=1e-12 * np.abs(naive).max() + 1e-12)
    np.testing.assert_array_equal(m, s.max(axis=1))
    assert (r >= 0).all() and (r <= np.log(n) + 1e-15).all()
    if n == 1:
        assert (r == 0).all()


def test_restatement_eligibility_nan_inf_and_no_row():
    q, x = _small(3, 40, 8, nq=4)
    s = P.scores(q, x, "float16")
    elig = np.zeros((4, 40), dtype=bool)
    elig[0, ::4] = True
    elig[1, 5] = True
    elig[3] = True
    m, r = P.log_partition(q, x, "float16", 2.0, elig)
    np.testing.assert_allclose(2.0 * m[0] + r[0], np.log(np.exp(2.0 * s[0, ::4]).sum()), rtol=1e-13)
    assert m[1] == s[1, 5] and r[1] == 0.0
    assert m[2] == -np.inf and r[2] == -np.inf  # no eligible row
    x2 = x.copy()
    x2[7, 0] = np.nan
    m2, r2 = P.log_partition(q, x2, "float16", 2.0)
    keep = np.ones(40, dtype=bool)
    keep[7] = False
    m3, r3 = P.log_partition(q, x[keep], "float16", 2.0)
    np.testing.assert_array_equal(m2, m3)
    np.testing.assert_array_equal(r2, r3)
    m4, r4 = P.from_scores(np.array([[1.0, np.inf, -2.0]]), 1.0)
    assert m4[0] == np.inf and r4[0] == np.inf
    m5, r5 = P.log_partition(q, x[:0], "float16", 1.0)
    assert np.isneginf(m5).all() and np.isneginf(r5).all()


def test_device_bound_is_monotone_in_n_dim_and_beta():
    q, x = _small(5, 64, 200, nq=9)
    by_n = [P.device_bound(q, x, "float16", 1.0, n) for n in (1, 2, 255, 256, 257, 3000, 10 ** 6)]
    assert all((a < b).all() for a, b in zip(by_n, by_n[1:]))
    by_d = [P.device_bound(q[:, :d], x[:, :d], "float16", 1.0, 64) for d in (1, 64, 65, 128, 200)]
    assert all((a <= b).all() for a, b in zip(by_d, by_d[1:])) and (by_d[0] < by_d[-1]).all()
    by_b = [P.device_bound(q, x, "float16", b, 64) for b in (1 / 64, 1.0, 4.0)]
    assert all((a < b).all() for a, b in zip(by_b, by_b[1:]))
    # without the dot-product part the bound no longer depends on the data or on beta
    a = P.device_bound(q, x, "float16", 1.0, 64, dot=False)
    b = P.device_bound(q, 3 * x, "bfloat16", 4.0, 64, dot=False)
    np.testing.assert_array_equal(a, b)
    assert (P.max_bound(q, x, "float16") > 0).all()


def test_topk_log_coverage_on_cpu_tensors():
    torch = pytest.importorskip("torch")
    from vod_amd.index import LogPartition, topk_log_coverage

    q, x = _small(9, 50, 12, nq=6)
    for T in (1.0, 0.5, 8.0):
        beta = 1.0 / T
        s = P.scores(q, x, "float16")
        m, r = P.from_scores(s, beta)
        lp = LogPartition(torch.from_numpy((beta * m + r).astype(np.float32)), torch.from_numpy(m.astype(np.float32)), torch.from_numpy(r.astype(np.float32)))
        top = np.sort(s, axis=1)[:, ::-1]
        full = torch.from_numpy(np.concatenate([top, np.full((6, 14), -np.inf)], axis=1).astype(np.float32))  # k = 64 >= n, pads -inf
        cov = topk_log_coverage(full, lp, T)
        assert cov.dtype == torch.float32 and cov.shape == (6,) and not cov.is_cuda
        # two float32 sums of <= 50 terms each (relative 50 u each), the float32 roundings of max and log_rel, and the rounded scores
        tol = 2 * 50 * P.U + 4 * P.U * np.log(50) + 2 * beta * np.abs(s).max() * P.U * 2
        assert cov.abs().max().item() <= tol
        part = topk_log_coverage(full[:, :10], lp, T)
        assert (part < 0).all()
        np.testing.assert_allclose(part.numpy(), P.coverage(s, 10, beta), rtol=0, atol=tol)
        assert (topk_log_coverage(full[:, :10], lp, T) <= topk_log_coverage(full[:, :20], lp, T)).all()


def test_shard_fold_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "partition_fold_check"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "sanitize" / "partition_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if built.returncode != 0 and "sanitizer" in built.stderr.lower() and "unsupported" in built.stderr.lower():
        pytest.skip("-fsanitize=address,undefined is not supported by this toolchain")
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


def test_both_symbols_are_declared_and_listed():
    from vod_amd import _native

    header = (ROOT / "include" / "vodhip.h").read_text()
    for name in ("vodhip_index_log_partition", "vodhip_node_index_log_partition"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _native.SIGNATURES
    lib = _native.load_library()
    assert hasattr(lib, "vodhip_index_log_partition") and hasattr(lib, "vodhip_node_index_log_partition")
