"""`posterior_mean` / `log_z`, the parts that need no GPU:

* the float64 restatement (tests/posterior_ref.py) equals a naive float64 softmax average on small inputs, the rows of p sum to 1 and the
  mean lies in the per-column [min, max] of the eligible rows; eligibility, NaN scores and the zero row behave as the contract states;
* the derived relative bound grows with n, with the width and with beta;
* the backward of `log_z` (`vod_amd.index.log_z_backward`, and the autograd function around an injected `posterior_mean`) equals
  `torch.autograd` of a float64 `logsumexp` on CPU tensors;
* the host fold of per-shard means (vod_amd/csrc/partition_fold.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
  program (tests/sanitize/posterior_fold_check.cpp); nothing is loaded into Python under a sanitizer;
* both new symbols are declared in include/vodhip.h and listed in `_native.SIGNATURES`.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import partition_ref as P
import posterior_ref as R
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _small(seed, n, d, nq=7, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((nq, d))).astype(np.float32), (scale * rng.standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("n,d,beta", [(1, 3, 1.0), (5, 1, 4.0), (37, 16, 0.25), (300, 65, 1.0)])
def test_restatement_matches_naive_float64(n, d, beta, dtype):
    from l2_ref import round_store

    q, x = _small(n + d, n, d)
    mean, m, r = R.posterior_mean(q, x, dtype, beta)
    s = P.scores(q, x, dtype)
    e = np.exp(beta * s)  # (small inputs: no overflow)
    xr = round_store(x, dtype)
    naive = (e / e.sum(axis=1, keepdims=True)) @ xr
    np.testing.assert_allclose(mean, naive, rtol=0, atol=1e-12 * np.abs(xr).max())
    p, m2, r2 = R.weights(s, beta)
    np.testing.assert_array_equal(m, m2)
    np.testing.assert_array_equal(r, r2)
    np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert (mean >= xr.min(axis=0) - 1e-12).all() and (mean <= xr.max(axis=0) + 1e-12).all()
    if n == 1:
        np.testing.assert_allclose(mean, np.repeat(xr, len(q), axis=0), rtol=0, atol=0)


def test_restatement_eligibility_nan_and_the_zero_row():
    from l2_ref import round_store

    q, x = _small(3, 40, 8, nq=4)
    xr = round_store(x, "float16")
    elig = np.zeros((4, 40), dtype=bool)
    elig[0, ::4] = True
    elig[1, 5] = True
    elig[3] = True
    mean, m, r = R.posterior_mean(q, x, "float16", 2.0, elig)
    p, _, _ = R.weights(P.scores(q, x, "float16"), 2.0, elig)
    np.testing.assert_allclose(p.sum(axis=1), [1.0, 1.0, 0.0, 1.0], rtol=0, atol=1e-12)
    assert (p[0, ~elig[0]] == 0).all()
    np.testing.assert_array_equal(mean[1], xr[5])              # one eligible row: that row
    assert (mean[2] == 0).all() and m[2] == -np.inf            # no eligible row: the zero row
    lo, hi = xr[::4].min(axis=0), xr[::4].max(axis=0)
    assert (mean[0] >= lo - 1e-12).all() and (mean[0] <= hi + 1e-12).all()
    x2 = x.copy()
    x2[7, 0] = np.nan                                          # every score of row 7 is NaN: the row is left out
    keep = np.ones(40, dtype=bool)
    keep[7] = False
    a, _, _ = R.posterior_mean(q, x2, "float16", 2.0)
    b, _, _ = R.posterior_mean(q, x[keep], "float16", 2.0)
    np.testing.assert_array_equal(a, b)
    p3, m3, _ = R.weights(np.array([[1.0, np.inf, -2.0], [0.0, 1.0, np.nan]]), 1.0)  # a +inf score: no weights, the zero row
    assert np.isposinf(m3[0]) and (p3[0] == 0).all() and p3[1, 2] == 0 and abs(p3[1].sum() - 1) < 1e-12
    d, m4, _ = R.posterior_mean(q, x[:0], "float16", 1.0)
    assert d.shape == (4, 8) and (d == 0).all() and np.isneginf(m4).all()


def test_device_bound_is_monotone_in_n_dim_and_beta():
    q, x = _small(5, 64, 200, nq=9)
    by_n = [R.rel_bound(q, x, "float16", 1.0, n, n) for n in (1, 2, 255, 256, 257, 3000, 10 ** 6)]
    assert all((a < b).all() for a, b in zip(by_n, by_n[1:]))
    by_d = [R.rel_bound(q[:, :d], x[:, :d], "float16", 1.0, 64, 64) for d in (1, 64, 65, 128, 200)]
    assert all((a <= b).all() for a, b in zip(by_d, by_d[1:])) and (by_d[0] < by_d[-1]).all()
    by_b = [R.rel_bound(q, x, "float16", b, 64, 64) for b in (1 / 64, 1.0, 4.0)]
    assert all((a < b).all() for a, b in zip(by_b, by_b[1:]))
    # never below the one rounding of the weight; bf16's is the coarser one
    assert (by_n[0] > R.EPS16["float16"]).all()
    assert (R.rel_bound(q, x, "bfloat16", 1.0, 64, 64) > R.rel_bound(q, x, "float16", 1.0, 64, 64)).all()
    # the full bound: a floor for fp16 only, and it scales with the rows
    f16 = R.device_bound(q, x, "float16", 1.0, dot=False)
    b16 = R.device_bound(q, x, "bfloat16", 1.0, dot=False)
    assert f16.shape == (9, 200) and (f16 > 0).all() and (b16 > 0).all()
    np.testing.assert_allclose(R.device_bound(q, 2 * x, "bfloat16", 0.5, dot=False), 2 * b16, rtol=1e-12)


def test_log_z_backward_equals_autograd_of_a_float64_logsumexp():
    torch = pytest.importorskip("torch")
    from vod_amd.index import LogPartition, PosteriorMean, _LogZ, log_z_backward

    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((50, 12)))
    for T in (1.0, 0.25, 8.0):
        beta = 1.0 / T
        q = torch.from_numpy(rng.standard_normal((6, 12))).requires_grad_(True)
        lz = torch.logsumexp(beta * q @ x.T, dim=1)
        w = torch.from_numpy(rng.standard_normal(6))
        (lz * w).sum().backward()
        mean = torch.softmax(beta * q.detach() @ x.T, dim=1) @ x
        got = log_z_backward(w, mean, lz.detach(), beta, torch.float64)
        assert got.dtype == torch.float64
        torch.testing.assert_close(got, q.grad, rtol=0, atol=4e-7 * float(q.grad.abs().max()))  # (the formula runs in float32)

        class Fake:  # the device call, injected
            def posterior_mean(self, queries, temperature, subset):
                assert not queries.requires_grad and subset is None
                s = (1.0 / temperature) * queries.double() @ x.T
                m = (queries.double() @ x.T).max(dim=1).values
                z = torch.logsumexp(s, dim=1)
                return PosteriorMean((torch.softmax(s, dim=1) @ x).float(), LogPartition(z.float(), m.float(), (z - m / temperature).float()))

        for dt in (torch.float32, torch.float16):
            q2 = q.detach().to(dt).requires_grad_(True)
            out = _LogZ.apply(q2, Fake(), T, None)
            assert out.dtype == torch.float32 and out.shape == (6,)
            (out * w.float()).sum().backward()
            assert q2.grad.dtype == dt and q2.grad.shape == q2.shape
            ref = w[:, None] * beta * (torch.softmax(beta * q2.detach().double() @ x.T, dim=1) @ x)
            eps = 2.0 ** -10 if dt == torch.float16 else 1e-6
            torch.testing.assert_close(q2.grad.double(), ref, rtol=0, atol=eps * float(ref.abs().max()))
    # rows whose log_z is not finite get a zero gradient, whatever grad_out and mean hold
    lz = torch.tensor([0.5, float("-inf"), float("inf")])
    g = log_z_backward(torch.tensor([2.0, float("nan"), 3.0]), torch.ones(3, 4), lz, 0.5, torch.float32)
    assert torch.equal(g, torch.tensor([[1.0] * 4, [0.0] * 4, [0.0] * 4]))


def test_shard_fold_of_the_means_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "posterior_fold_check"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "sanitize" / "posterior_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
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
    for name in ("vodhip_index_posterior_mean", "vodhip_node_index_posterior_mean"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _native.SIGNATURES
    assert "VODHIP_POSTERIOR_GROUP_ROWS " + str(R.GROUP_ROWS) in header
    lib = _native.load_library()
    assert hasattr(lib, "vodhip_index_posterior_mean") and hasattr(lib, "vodhip_node_index_posterior_mean")
