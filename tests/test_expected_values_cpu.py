"""`expected_values` / `posterior_expectation_backward`, the parts that need no GPU:

* the float64 restatement (tests/readout_grad_ref.py) equals `torch.autograd.grad` of `(softmax(beta q~ x~^T) @ v~ * g).sum()` in
  float64 on the CPU, for both dtypes' roundings and with `eligible` masks; a dead query gets the zero row;
* a column of ones gives a zero gradient in the reference (pure cancellation);
* the derived bound is non-negative and finite, its g term vanishes when g is exact in 16 bits, and the staging restatement puts the
  largest entry of a row in [1, 2);
* the host pieces of a node index (vod_amd/csrc/readout_grad_fold.h: argument checks, the fold) under AddressSanitizer and
  UndefinedBehaviorSanitizer, as a stand-alone program (tests/sanitize/readout_grad_fold_check.cpp); nothing is loaded into Python
  under a sanitizer;
* the new symbols are declared in include/vodhip.h, listed in `_native.SIGNATURES` with as many arguments, and exported;
* both indexes expose the two methods.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import readout_grad_ref as G
from conftest import ROOT
from l2_ref import round_store

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _case(seed, n=700, d=9, nq=21, w=70):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    v = rng.standard_normal((n, w)).astype(np.float32)
    g = rng.standard_normal((nq, w)).astype(np.float32)
    return q, x, v, g


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("beta", [1.0, 1.0 / 64.0, 4.0])
def test_restatement_equals_float64_autograd(beta, dtype):
    torch = pytest.importorskip("torch")
    q, x, v, g = _case(3)
    elig = np.random.default_rng(4).random((len(q), len(x))) < 0.5
    elig[4] = False  # a dead query
    xr, vr, qr = (torch.from_numpy(round_store(a, dtype)) for a in (x, v, q))
    gt = torch.from_numpy(g.astype(np.float64))
    for e in (None, elig):
        got, y, m, _ = G.expected_values_grad(q, x, v, g, dtype, beta, e)
        qt = qr.clone().requires_grad_(True)
        s = beta * (qt @ xr.T)
        if e is not None:
            s = s.masked_fill(~torch.from_numpy(e), float("-inf"))
        live = torch.isfinite(s).any(dim=1)
        out = torch.softmax(s[live], dim=1) @ vr
        (want,) = torch.autograd.grad((out * gt[live]).sum(), qt)
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(y[live.numpy()], out.detach().numpy(), rtol=1e-12, atol=1e-14)
        dead = ~np.isfinite(m)
        assert np.array_equal(dead, ~live.numpy()) and (got[dead] == 0).all()
        assert np.array_equal(dead, (np.arange(len(q)) == 4) if e is not None else np.zeros(len(q), dtype=bool))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_a_column_of_ones_has_a_zero_gradient(dtype):
    q, x, v, g = _case(5, w=1)
    ones = np.ones((len(x), 1), dtype=np.float32)
    got, y, _, _ = G.expected_values_grad(q, x, ones, g, dtype, 0.25)
    np.testing.assert_allclose(y, 1.0, rtol=0, atol=1e-14)
    scale = np.abs(g) * np.abs(round_store(x, dtype)).max(axis=0)[None, :]
    assert (np.abs(got) <= 1e-13 * scale).all()  # u_z - ubar = g (1 - sum p): zero up to the float64 rounding of the weights
    # and next to other columns it contributes nothing
    v2 = np.concatenate([v[:, :0], np.ones((len(x), 1), dtype=np.float32), _case(5, w=3)[2]], axis=1)
    g2 = np.concatenate([g[:, :1], _case(6, w=3)[3]], axis=1)
    a, _, _, _ = G.expected_values_grad(q, x, v2, g2, dtype, 0.25)
    b, _, _, _ = G.expected_values_grad(q, x, v2[:, 1:], g2[:, 1:], dtype, 0.25)
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("dot", [False, True])
def test_bound_is_non_negative_and_finite(dot, dtype):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3000, 33)).astype(np.float32)
    q = rng.standard_normal((17, 33)).astype(np.float32)
    v = rng.standard_normal((3000, 5)).astype(np.float32)
    g = (rng.standard_normal((17, 5)) * 1e-6).astype(np.float32)
    g[3] = 0  # a zero row: the bound may be 0 there, not negative
    for beta in (1.0, 1.0 / 64.0, 4.0):
        b = G.device_bound(q, x, v, g, dtype, beta, dot=dot)
        assert b.shape == (17, 33) and np.isfinite(b).all() and (b >= 0).all() and (np.delete(b, 3, axis=0) > 0).all()
    elig = np.zeros((17, 3000), dtype=bool)
    assert np.isfinite(G.device_bound(q, x, v, g, dtype, 1.0, elig, dot=dot)).all()
    # g exact in 16 bits after the power-of-two scale: the bound is no larger than for an inexact g of the same size
    g16 = (rng.integers(-4, 5, size=(17, 5)) * 2.0 ** -10).astype(np.float32)
    exact = G.device_bound(q, x, v, g16, dtype, 1.0, dot=dot)
    inexact = G.device_bound(q, x, v, (g16 * (1 + 2.0 ** -13)).astype(np.float32), dtype, 1.0, dot=dot)
    assert (exact <= inexact * (1 + 1e-3)).all()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_staging_restatement_normalises_each_row(dtype):
    rng = np.random.default_rng(6)
    g = (rng.standard_normal((9, 7)) * 10.0 ** rng.integers(-30, 5, size=(9, 1))).astype(np.float32)
    g[2] = 0
    y = rng.standard_normal((9, 7))
    vmax = np.abs(rng.standard_normal(7)) + 0.1
    k, g_hat, R = G.staging(g, y, vmax, dtype)
    top = np.abs(g).max(axis=1) * 2.0 ** -k
    assert ((top >= 1) & (top < 2))[np.arange(9) != 2].all() and k[2] == 0 and R[2] == 1
    assert (np.abs(g_hat - g) <= G.EPS16[dtype] * np.abs(g).max(axis=1, keepdims=True)).all()
    need = (np.abs(g_hat * 2.0 ** -k[:, None]) * vmax).sum(axis=1) + np.abs((g_hat * 2.0 ** -k[:, None] * y).sum(axis=1))
    assert (R >= need).all() and (R == 2.0 ** np.round(np.log2(R))).all() and (R[np.arange(9) != 2] < 4.1 * need[np.arange(9) != 2]).all()


def test_host_pieces_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([CLANG, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=600)
    if probed.returncode != 0:  # (decided on an empty program, before the program under test is built)
        pytest.skip("this toolchain does not link -fsanitize=address,undefined")
    exe = tmp_path / "readout_grad_fold_check"
    cmd = [CLANG, *flags, str(ROOT / "tests" / "sanitize" / "readout_grad_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


DECLARED = {
    "vodhip_index_posterior_expectation_backward": ["index", "queries", "q_dtype", "nq", "beta", "q_labels_dev", "n_per_query", "max_score", "log_rel",
                                                    "values", "grad_values", "out_grad_queries", "stream"],
    "vodhip_node_index_posterior_expectation_backward": ["index", "queries", "q_dtype", "nq", "beta", "q_labels", "n_per_query", "max_score", "log_rel",
                                                         "values", "grad_values", "out_grad_queries"],
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


def test_both_indexes_expose_the_two_methods():
    pytest.importorskip("torch")
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    for cls in (HipFlatIndex, HipNodeIndex):
        assert callable(cls.posterior_expectation_backward) and callable(cls.expected_values)
