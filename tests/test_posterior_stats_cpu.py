"""`posterior_stats`, the parts that need no GPU:

* the float64 restatement (tests/stats_ref.py) equals naive float64 softmax moments on small inputs, 0 <= entropy <= log n, a one-row
  store gives (0, 0, 0), eligibility / NaN row / -inf score / +inf score / no row behave as the contract states;
* the derived device bound grows with n, with the width and with beta;
* the host fold of per-shard words (vod_amd/csrc/stats_fold.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
  program (tests/sanitize/stats_fold_check.cpp); nothing is loaded into Python under a sanitizer;
* both new symbols are declared in include/vodhip.h and listed in `_native.SIGNATURES`;
* `_LogZ` with a NumPy-backed fake index: grad_T and grad_q equal torch autograd of the dense float64 logsumexp(q @ x.T / T), and
  `posterior_mean` is never called when only T requires grad.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch

import partition_ref as P
import stats_ref as S
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _small(seed, n, d, nq=7, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((nq, d))).astype(np.float32), (scale * rng.standard_normal((n, d))).astype(np.float32)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("n,d,beta", [(1, 3, 1.0), (5, 1, 4.0), (37, 16, 0.25), (300, 65, 1.0)])
def test_restatement_matches_naive_float64_softmax_moments(n, d, beta, dtype):
    q, x = _small(n + d, n, d)
    words = S.posterior_stats(q, x, dtype, beta)
    m, r, mean_rel, var = words
    s = P.scores(q, x, dtype)
    p = np.exp(beta * s)
    p /= p.sum(axis=1, keepdims=True)  # (small inputs: no overflow)
    mu = (p * s).sum(axis=1)
    scale = np.abs(s).max() + 1.0
    np.testing.assert_array_equal(m, s.max(axis=1))
    np.testing.assert_array_equal(r, P.log_partition(q, x, dtype, beta)[1])
    np.testing.assert_allclose(S.mean_score(words), mu, rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(var, (p * (s - mu[:, None]) ** 2).sum(axis=1), rtol=0, atol=1e-12 * scale ** 2)
    np.testing.assert_allclose(S.entropy(words, beta), -(p * np.log(p)).sum(axis=1), rtol=0, atol=1e-12 * (1 + beta * scale))
    h = S.entropy(words, beta)
    assert (mean_rel <= 0).all() and (var >= 0).all()
    assert (h >= -1e-15).all() and (h <= np.log(n) + 1e-12).all()
    if n == 1:
        assert (h == 0).all() and (mean_rel == 0).all() and (var == 0).all()


def test_restatement_eligibility_nan_inf_and_no_row():
    q, x = _small(3, 40, 8, nq=4)
    s = P.scores(q, x, "float16")
    elig = np.zeros((4, 40), dtype=bool)
    elig[0, ::4] = True
    elig[1, 5] = True
    elig[3] = True
    m, r, a, v = S.posterior_stats(q, x, "float16", 2.0, elig)
    m0, r0, a0, v0 = S.from_scores(s[:1, ::4], 2.0)
    assert (m[0], r[0], a[0], v[0]) == (m0[0], r0[0], a0[0], v0[0])
    assert m[1] == s[1, 5] and (r[1], a[1], v[1]) == (0.0, 0.0, 0.0)  # one row: (0, 0, 0)
    assert m[2] == -np.inf and r[2] == -np.inf and np.isnan(a[2]) and np.isnan(v[2])  # no eligible row
    # a NaN row is left out
    x2 = x.copy()
    x2[7, 0] = np.nan
    keep = np.ones(40, dtype=bool)
    keep[7] = False
    for got, want in zip(S.posterior_stats(q, x2, "float16", 2.0), S.posterior_stats(q, x[keep], "float16", 2.0)):
        np.testing.assert_array_equal(got, want)
    # a -inf score adds nothing and makes no NaN; all -inf counts as no row; a +inf score
    w = S.from_scores(np.array([[1.0, -np.inf, -2.0], [1.0, -2.0, -1e150], [-np.inf, -np.inf, -np.inf], [1.0, np.inf, -2.0]]), 1.0)
    ref = S.from_scores(np.array([[1.0, -2.0]]), 1.0)
    for k in range(4):  # (word k; queries 0 and 1: a score that underflows adds nothing either)
        assert w[k][0] == ref[k][0] and w[k][1] == ref[k][0] and np.isfinite(ref[k][0])
    assert w[0][2] == -np.inf and w[1][2] == -np.inf and np.isnan(w[2][2]) and np.isnan(w[3][2])
    assert w[0][3] == np.inf and w[1][3] == np.inf and np.isnan(w[2][3]) and np.isnan(w[3][3])
    e = S.posterior_stats(q, x[:0], "float16", 1.0)
    assert np.isneginf(e[0]).all() and np.isneginf(e[1]).all() and np.isnan(e[2]).all() and np.isnan(e[3]).all()


def test_device_bound_is_monotone_in_n_dim_and_beta():
    q, x = _small(5, 64, 200, nq=9)
    mean_rel, var = -np.linspace(0.5, 30.0, 9), np.linspace(0.1, 9.0, 9)

    def both(*a, **k):
        return np.stack(S.device_bound(*a, **k))

    by_n = [both(q, x, "float16", 1.0, n, mean_rel, var) for n in (1, 257, 3000, 10 ** 6, 10 ** 9)]
    assert all((a <= b).all() for a, b in zip(by_n, by_n[1:])) and (by_n[0] < by_n[-1]).all()
    by_d = [both(q[:, :d], x[:, :d], "float16", 1.0, 64, mean_rel, var) for d in (1, 64, 65, 128, 200)]
    assert all((a <= b).all() for a, b in zip(by_d, by_d[1:])) and (by_d[0] < by_d[-1]).all()
    by_b = [both(q, x, "float16", b, 64, mean_rel, var) for b in (1 / 64, 1.0, 4.0)]
    assert all((a < b).all() for a, b in zip(by_b, by_b[1:]))
    # without the dot-product part the bound does not depend on the data, and it is (2 rho_e + gamma_36) twice, about 915 u, of the word's magnitude
    a = both(q, x, "float16", 1.0, 3000, mean_rel, var, dot=False)
    b = both(7 * q, x, "float16", 1.0, 3000, mean_rel, var, dot=False)
    np.testing.assert_array_equal(a, b)
    assert (a[0] <= 1000 * S.U * np.abs(mean_rel)).all() and (a[0] >= 800 * S.U * np.abs(mean_rel)).all()
    assert (a[1] <= 3000 * S.U * (var + mean_rel ** 2)).all()
    assert (a < both(q, x, "float16", 1.0, 3000, mean_rel, var)).all()
    # it grows with the magnitude of the words
    assert (both(q, x, "float16", 1.0, 64, 2 * mean_rel, var) > both(q, x, "float16", 1.0, 64, mean_rel, var)).all()


def test_shard_fold_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "stats_fold_check"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "sanitize" / "stats_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
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
    for name in ("vodhip_index_posterior_stats", "vodhip_node_index_posterior_stats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _native.SIGNATURES
    lib = _native.load_library()
    assert hasattr(lib, "vodhip_index_posterior_stats") and hasattr(lib, "vodhip_node_index_posterior_stats")


class _FakeIndex:
    """NumPy-backed: float64 words of the dense scores, returned as NumPy arrays as a node index returns them."""

    def __init__(self, x):
        self.x = x
        self.mean_calls = self.stats_calls = 0

    def _words(self, queries, temperature, subset):
        assert not queries.requires_grad and subset is None
        return S.from_scores(queries.double().numpy() @ self.x.T, 1.0 / temperature)

    def posterior_stats(self, queries, temperature, subset):
        from vod_amd.index import LogPartition, PosteriorStats

        self.stats_calls += 1
        beta = 1.0 / temperature
        m, r, mean_rel, var = self._words(queries, temperature, subset)
        with np.errstate(invalid="ignore"):
            return PosteriorStats(r - beta * mean_rel, m + mean_rel, var, mean_rel, LogPartition(beta * m + r, m, r))

    def posterior_mean(self, queries, temperature, subset):
        from vod_amd.index import LogPartition, PosteriorMean

        self.mean_calls += 1
        beta = 1.0 / temperature
        m, r, _, _ = self._words(queries, temperature, subset)
        s = queries.double().numpy() @ self.x.T
        p = np.exp(beta * (s - m[:, None]) - r[:, None])
        return PosteriorMean(p @ self.x, LogPartition(beta * m + r, m, r))


def test_log_z_with_a_tensor_temperature_matches_dense_float64_autograd():
    from vod_amd.index import _LogZ, log_z_temperature_backward

    rng = np.random.default_rng(12)
    x = rng.standard_normal((50, 12))
    xt = torch.from_numpy(x)
    w = torch.from_numpy(rng.standard_normal(6))
    for T0 in (1.0, 0.25, 8.0):
        q = torch.from_numpy(rng.standard_normal((6, 12))).requires_grad_(True)
        T = torch.tensor([T0], dtype=torch.float64, requires_grad=True)
        (torch.logsumexp(q @ xt.T / T, dim=1) * w).sum().backward()

        # both gradients
        fake = _FakeIndex(x)
        q2 = q.detach().clone().requires_grad_(True)
        T2 = torch.tensor([T0], dtype=torch.float64, requires_grad=True)
        out = _LogZ.apply(q2, fake, T2, None)
        assert out.shape == (6,)
        (out * w).sum().backward()
        assert (fake.stats_calls, fake.mean_calls) == (1, 1)
        assert T2.grad.shape == T.grad.shape and T2.grad.dtype == T.grad.dtype
        torch.testing.assert_close(T2.grad, T.grad, rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(q2.grad, q.grad, rtol=0, atol=4e-7 * float(q.grad.abs().max()))  # (grad_q's formula runs in float32)
        # ... and grad_q is what the float-temperature path gives, bit for bit
        q3 = q.detach().clone().requires_grad_(True)
        (_LogZ.apply(q3, _FakeIndex(x), T0, None) * w).sum().backward()
        assert torch.equal(q3.grad, q2.grad)

        # only T requires grad: posterior_mean is never called
        fake = _FakeIndex(x)
        T3 = torch.tensor(T0, dtype=torch.float32, requires_grad=True)  # (0-d, float32)
        out = _LogZ.apply(q.detach(), fake, T3, None)
        (out * w).sum().backward()
        assert (fake.stats_calls, fake.mean_calls) == (1, 0)
        assert T3.grad.shape == () and T3.grad.dtype == torch.float32
        torch.testing.assert_close(T3.grad.double(), T.grad[0], rtol=2e-7, atol=0)

        # only q requires grad, T a plain tensor
        fake = _FakeIndex(x)
        q4 = q.detach().clone().requires_grad_(True)
        (_LogZ.apply(q4, fake, torch.tensor([T0]), None) * w).sum().backward()
        assert fake.mean_calls == 1 and torch.equal(q4.grad, q2.grad)

    with pytest.raises(ValueError):
        _LogZ.apply(q.detach(), _FakeIndex(x), torch.tensor([1.0, 2.0], requires_grad=True), None)
    # queries whose log_z is not finite contribute 0, whatever grad_out and mean_score hold
    g = log_z_temperature_backward(torch.tensor([2.0, float("nan"), 3.0]), torch.tensor([1.5, float("nan"), float("inf")]),
                                   torch.tensor([0.5, float("-inf"), float("inf")]), 2.0)
    assert g.item() == -2.0 * 1.5 / 4.0
