"""`posterior_adjoint` / `row_mass` / `read_out`, the parts that need no GPU:

* the float64 restatement (tests/readout_adjoint_ref.py) equals `torch.autograd.grad` of `(softmax(beta q~ x~^T) @ V * g).sum()` in V,
  in float64 on the CPU, for both dtypes' roundings, with and without `eligible` masks and with a dead query;
* `row_mass` sums to the number of live queries; the adjoint identity <g, P V> == <P^T g, V> holds in float64;
* the derived bound is finite and non-negative, and its W term vanishes for a W that is exact in 16 bits; the staging restatement puts
  the largest entry of a column in [1, 2);
* the host pieces (vod_amd/csrc/readout_adjoint_fold.h: argument checks, the padded width, the shard slabs) under AddressSanitizer and
  UndefinedBehaviorSanitizer, as a stand-alone program (tests/sanitize/readout_adjoint_check.cpp); nothing is loaded into Python under
  a sanitizer;
* the two symbols are declared in include/vodhip.h, listed in `_native.SIGNATURES` with as many arguments, and exported;
* both indexes expose the three methods.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import partition_ref as P
import posterior_ref as M
import readout_adjoint_ref as A
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


def _masks(q, x):
    elig = np.random.default_rng(4).random((len(q), len(x))) < 0.5
    elig[4] = False  # a dead query
    return elig


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("beta", [1.0, 1.0 / 64.0, 4.0])
def test_restatement_equals_float64_autograd_in_the_table(beta, dtype):
    torch = pytest.importorskip("torch")
    q, x, v, g = _case(3)
    elig = _masks(q, x)
    xr, qr = (torch.from_numpy(round_store(a, dtype)).double() for a in (x, q))
    gt = torch.from_numpy(g.astype(np.float64))
    for e in (None, elig):
        got, m, _ = A.posterior_adjoint(q, x, g, dtype, beta, e)
        vt = torch.from_numpy(v.astype(np.float64)).requires_grad_(True)
        s = beta * (qr @ xr.T)
        if e is not None:
            s = s.masked_fill(~torch.from_numpy(e), float("-inf"))
        live = torch.isfinite(s).any(dim=1)
        out = torch.softmax(s[live], dim=1) @ vt
        (want,) = torch.autograd.grad((out * gt[live]).sum(), vt)
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-13)
        dead = ~np.isfinite(m)
        assert np.array_equal(dead, ~live.numpy())
        assert np.array_equal(dead, (np.arange(len(q)) == 4) if e is not None else np.zeros(len(q), dtype=bool))
        # the dead query contributes nothing: dropping it changes no value
        if e is not None:
            keep = np.arange(len(q)) != 4
            again, _, _ = A.posterior_adjoint(q[keep], x, g[keep], dtype, beta, e[keep])
            np.testing.assert_allclose(got, again, rtol=1e-13, atol=0)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_row_mass_sums_to_the_number_of_live_queries(dtype):
    q, x, _, _ = _case(5)
    elig = _masks(q, x)
    for beta in (1.0, 0.25):
        np.testing.assert_allclose(A.row_mass(q, x, dtype, beta).sum(), len(q), rtol=1e-12)
        mass = A.row_mass(q, x, dtype, beta, elig)
        np.testing.assert_allclose(mass.sum(), len(q) - 1, rtol=1e-12)
        assert (mass >= 0).all() and (mass[~elig.any(axis=0)] == 0).all()
        qw = np.arange(len(q), dtype=np.float32)
        np.testing.assert_allclose(A.row_mass(q, x, dtype, beta, elig, qw).sum(), qw.sum() - 4, rtol=1e-12)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_adjoint_identity_in_float64(dtype):
    q, x, v, g = _case(6)
    elig = _masks(q, x)
    for e in (None, elig):
        p, _, _ = M.weights(P.scores(q, x, dtype), 0.5, e)
        y = p @ v.astype(np.float64)                                   # the read-out P V
        adj, _, _ = A.posterior_adjoint(q, x, g, dtype, 0.5, e)        # P^T g
        lhs, rhs = (g.astype(np.float64) * y).sum(), (adj * v.astype(np.float64)).sum()
        scale = (np.abs(g).astype(np.float64) * (p @ np.abs(v).astype(np.float64))).sum()
        assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("dot", [False, True])
def test_bound_is_non_negative_and_finite_and_its_w_term_vanishes_for_exact_w(dot, dtype):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3000, 33)).astype(np.float32)
    q = rng.standard_normal((17, 33)).astype(np.float32)
    w = (rng.standard_normal((17, 5)) * 1e-6).astype(np.float32)
    w[:, 3] = 0  # a zero column: the bound is 0 there, not negative
    for beta in (1.0, 1.0 / 64.0, 4.0):
        b = A.device_bound(q, x, w, dtype, beta, dot=dot)
        assert b.shape == (3000, 5) and np.isfinite(b).all() and (b >= 0).all() and (b[:, 3] == 0).all() and (np.delete(b, 3, axis=1) > 0).all()
    elig = np.zeros((17, 3000), dtype=bool)
    assert np.isfinite(A.device_bound(q, x, w, dtype, 1.0, elig, dot=dot)).all()
    # W exact in 16 bits after the column's power of two: no W term
    w16 = (rng.integers(-4, 5, size=(17, 5)) * 2.0 ** -10).astype(np.float32)
    _, w_hat, werr = A.staging(w16, dtype)
    assert (werr == 0).all() and np.array_equal(np.ldexp(w_hat, A.column_exponents(w16)[None, :]), w16.astype(np.float64))
    exact = A.device_bound(q, x, w16, dtype, 1.0, dot=dot)
    w_in = (w16 * (1 + 2.0 ** -13)).astype(np.float32)
    _, _, werr_in = A.staging(w_in, dtype)
    assert (werr_in[w_in != 0] > 0).all()
    inexact = A.device_bound(q, x, w_in, dtype, 1.0, dot=dot)
    assert (exact <= inexact * (1 + 1e-3)).all() and (exact < inexact)[:, np.abs(w16).max(axis=0) > 0].all()
    # a node index's folded log_rel only widens it
    assert (A.device_bound(q, x, w16, dtype, 1.0, dot=dot, rel_extra=1e-6) >= exact).all()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_staging_restatement_normalises_each_column(dtype):
    rng = np.random.default_rng(6)
    w = (rng.standard_normal((9, 7)) * 10.0 ** rng.integers(-30, 5, size=(1, 7))).astype(np.float32)
    w[:, 2] = 0
    k, w_hat, werr = A.staging(w, dtype)
    top = np.abs(w).max(axis=0) * 2.0 ** -k.astype(np.float64)
    assert ((top >= 1) & (top < 2))[np.arange(7) != 2].all() and k[2] == 0
    assert (np.abs(w_hat) <= 2).all() and (np.abs(w_hat - np.ldexp(w.astype(np.float64), -k[None, :])) <= werr).all()
    assert A.column_exponents(np.zeros((0, 3), dtype=np.float32)).tolist() == [0, 0, 0]


def test_host_pieces_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([CLANG, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=600)
    if probed.returncode != 0:  # (decided on an empty program, before the program under test is built)
        pytest.skip("this toolchain does not link -fsanitize=address,undefined")
    exe = tmp_path / "readout_adjoint_check"
    cmd = [CLANG, *flags, str(ROOT / "tests" / "sanitize" / "readout_adjoint_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


DECLARED = {
    "vodhip_index_posterior_adjoint": ["index", "queries", "q_dtype", "nq", "beta", "q_labels_dev", "n_per_query", "max_score", "log_rel", "weights",
                                       "n_cols", "accumulate", "out", "stream"],
    "vodhip_node_index_posterior_adjoint": ["index", "queries", "q_dtype", "nq", "beta", "q_labels", "n_per_query", "max_score", "log_rel", "weights",
                                            "n_cols", "out"],
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
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    for cls in (HipFlatIndex, HipNodeIndex):
        assert callable(cls.posterior_adjoint) and callable(cls.row_mass) and callable(cls.read_out)
