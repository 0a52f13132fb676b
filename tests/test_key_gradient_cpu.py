"""`key_gradient` and the `keys` keyword of `log_z` / `read_out`, the parts that need no GPU:

* the float64 restatement (tests/key_grad_ref.py) IS the gradient: central differences in float64 of sum_q a_q log Z_q + sum_qc G_qc y_qc
  in the stored rows, at 5 queries x 7 rows x dim 3 x 2 columns, within the truncation error of the difference quotient derived from
  the step; and it equals `torch.autograd.grad` through a dense float64 softmax, with masks and a dead query;
* the identities of the operator in float64: the rows sum to beta sum_q a_q q~_q, a table column of ones adds nothing;
* the staging arithmetic (batch exponent, a', G^, ubar, B, R, flags) of the NumPy restatement on hand-computed batches;
* the derived bound is finite and non-negative, its G term vanishes for a G that is exact in 16 bits, a node's folded words widen it;
* the host pieces (vod_amd/csrc/key_grad_fold.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program
  (tests/sanitize/key_grad_check.cpp); nothing is loaded into Python under a sanitizer;
* the two symbols are declared in include/vodhip.h (which stays C99), listed in `_native.SIGNATURES` with as many arguments, and
  exported; both indexes expose `key_gradient` and the `keys` keyword.
"""
import inspect
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import key_grad_ref as K
from conftest import ROOT
from l2_ref import round_store

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _objective(x, q, v, a, G, beta):
    """sum_q a_q log Z_q + sum_qc G_qc y_qc in float64, nothing rounded"""
    s = beta * (q @ x.T)
    m = s.max(axis=1, keepdims=True)
    e = np.exp(s - m)
    z = e.sum(axis=1, keepdims=True)
    return float((a * (m[:, 0] + np.log(z[:, 0]))).sum() + (G * ((e / z) @ v)).sum())


@pytest.mark.parametrize("beta", [1.0, 1.0 / 64.0, 4.0])
def test_the_reference_is_the_gradient_by_central_differences(beta):
    rng = np.random.default_rng(11)
    nq, n, d, c = 5, 7, 3, 2
    # multiples of 1/8 below 4: exact in fp16 and bf16, so the restatement's rounding changes nothing
    x = rng.integers(-16, 17, size=(n, d)) / 8.0
    q = rng.integers(-16, 17, size=(nq, d)) / 8.0
    v = rng.integers(-16, 17, size=(n, c)) / 8.0
    a = rng.integers(-8, 9, size=nq) / 4.0
    G = rng.integers(-8, 9, size=(nq, c)) / 4.0
    h = 2.0 ** -10
    # |third derivative| of the objective along e_zd: the tilt of query q is w = beta q_qd 1[row z], centred |w| <= b = |beta q_qd|.
    # log Z: the third cumulant of w, at most b^3.  y_c: the joint cumulant k(v, w, w, w) = E[v w^3] - 3 E[v w] E[w^2] of the centred
    # variables, at most 4 V_c b^3 with V_c = max v_c - min v_c.  A central difference is off by at most h^2 / 6 of that; the float64
    # evaluation of the objective by a few ulps of its size F, divided by h
    V = v.max(axis=0) - v.min(axis=0)
    for dtype in ("float16", "bfloat16"):
        got, _, _, _ = K.key_gradient(q.astype(np.float32), x.astype(np.float32), dtype, beta, a, G, v.astype(np.float32))
        F = float((np.abs(a) * np.abs(beta * (q @ x.T)).max(axis=1)).sum() + (np.abs(G) * np.abs(v).max(axis=0)[None, :]).sum()) + 1.0
        worst = 0.0
        for z in range(n):
            for i in range(d):
                b3 = np.abs(beta * q[:, i]) ** 3
                third = float((np.abs(a) * b3).sum() + (np.abs(G) * 4 * V[None, :] * b3[:, None]).sum())
                tol = h * h / 6 * third + 16 * 2.0 ** -53 * F / h
                xp, xm = x.copy(), x.copy()
                xp[z, i] += h
                xm[z, i] -= h
                fd = (_objective(xp, q, v, a, G, beta) - _objective(xm, q, v, a, G, beta)) / (2 * h)
                assert abs(fd - got[z, i]) <= tol, (z, i, fd, got[z, i], tol)
                worst = max(worst, tol)
        assert worst < 1e-2 * np.abs(got).max()  # (the check is far below the gradient's size)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("beta", [1.0, 1.0 / 64.0, 4.0])
def test_restatement_equals_float64_autograd_in_the_rows(beta, dtype):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(3)
    n, d, nq, c = 300, 9, 21, 5
    x, q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    v, G = rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((nq, c)).astype(np.float32)
    a = rng.standard_normal(nq).astype(np.float32)
    elig = rng.random((nq, n)) < 0.5
    elig[4] = False  # a dead query
    qr, vr = (torch.from_numpy(round_store(t, dtype)).double() for t in (q, v))
    for e in (None, elig):
        for aa, GG in ((a, None), (None, G), (a, G)):
            got, _, m, _ = K.key_gradient(q, x, dtype, beta, aa, GG, v if GG is not None else None, e)
            xt = torch.from_numpy(round_store(x, dtype)).double().requires_grad_(True)
            s = beta * (qr @ xt.T)
            if e is not None:
                s = s.masked_fill(~torch.from_numpy(e), float("-inf"))
            live = torch.isfinite(s).any(dim=1)
            loss = 0.0
            if aa is not None:
                loss = loss + (torch.from_numpy(aa.astype(np.float64))[live] * torch.logsumexp(s[live], dim=1)).sum()
            if GG is not None:
                loss = loss + (torch.from_numpy(GG.astype(np.float64))[live] * (torch.softmax(s[live], dim=1) @ vr)).sum()
            (want,) = torch.autograd.grad(loss, xt)
            np.testing.assert_allclose(got, want.numpy(), rtol=1e-9, atol=1e-12)
            assert np.array_equal(~np.isfinite(m), ~live.numpy())


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_identities_of_the_operator_in_float64(dtype):
    rng = np.random.default_rng(8)
    n, d, nq, c = 200, 7, 13, 4
    x, q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    v, G = rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((nq, c)).astype(np.float32)
    a = rng.standard_normal(nq).astype(np.float32)
    beta = 0.5
    qr = round_store(q, dtype).astype(np.float64)
    both, _, _, _ = K.key_gradient(q, x, dtype, beta, a, G, v)
    # (ii) the read-out term sums to zero over the rows
    np.testing.assert_allclose(both.sum(axis=0), beta * (a.astype(np.float64)[:, None] * qr).sum(axis=0), rtol=1e-10, atol=1e-12)
    # (iv) a column of ones adds nothing, whatever its gradient
    v1, G1 = np.concatenate([v, np.ones((n, 1), dtype=np.float32)], axis=1), np.concatenate([G, rng.standard_normal((nq, 1)).astype(np.float32)], axis=1)
    ones, _, _, _ = K.key_gradient(q, x, dtype, beta, a, G1, v1)
    np.testing.assert_allclose(ones, both, rtol=1e-10, atol=1e-12)
    # linear in (a, G)
    only_a, _, _, _ = K.key_gradient(q, x, dtype, beta, a, None, None)
    only_g, _, _, _ = K.key_gradient(q, x, dtype, beta, None, G, v)
    np.testing.assert_allclose(only_a + only_g, both, rtol=1e-10, atol=1e-12)
    assert K.key_gradient(q, x[:0], dtype, beta, a)[0].shape == (0, d)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_staging_restatement_on_hand_computed_batches(dtype):
    # log Z only: k from the largest |a| = 3 -> 1; a' = a / 2; B = |a'|; R = the power of two above 1.5 (1 + 2^-10) = 2
    st = K.staging(np.array([3, -0.5, 0], dtype=np.float32), None, None, None, dtype)
    assert st["k"] == 1 and st["a"].tolist() == [1.5, -0.25, 0.0] and st["B"].tolist() == [1.5, 0.25, 0.0]
    assert st["flag"].tolist() == [0, 0, 1] and not st["nan"] and st["e"] == 1 and st["shift"] == 2
    # with a table: k from the largest |G| = 4 -> 2, whatever a is
    G = np.array([[4, 0], [1, -2]], dtype=np.float32)
    y = np.array([[1, 2], [0.5, 0.25]], dtype=np.float32)
    vmax = np.array([3, 5], dtype=np.float32)
    st = K.staging(np.array([8, 0], dtype=np.float32), G, y, vmax, dtype)
    assert st["k"] == 2 and st["g_hat"].tolist() == [[1.0, 0.0], [0.25, -0.5]] and st["a"].tolist() == [2.0, 0.0]
    assert st["ubar"].tolist() == [1.0, 0.0] and st["B"].tolist() == [2 + 3 + 1, 0.75 + 2.5]
    assert st["flag"].tolist() == [0, 0] and st["e"] == 3 and st["shift"] == 5       # 6 (1 + 2^-10) = 0.75.. * 2^3
    # B exactly a power of two: R is the NEXT one (R > B (1 + 2^-10))
    st = K.staging(np.array([4, 1], dtype=np.float32), None, None, None, dtype)
    assert st["k"] == 2 and st["B"].max() == 1.0 and st["e"] == 1
    # G all zero: k from a; a zero query is flag 1
    st = K.staging(np.array([0.75, 0], dtype=np.float32), np.zeros((2, 2), dtype=np.float32), y, vmax, dtype)
    assert st["k"] == -1 and st["a"].tolist() == [1.5, 0.0] and st["flag"].tolist() == [0, 1]
    # non-finite input: flag 2 and the batch is NaN; the exponent comes from the finite entries
    Gn = G.copy()
    Gn[1, 0] = np.nan
    st = K.staging(np.array([np.inf, 1, 1], dtype=np.float32)[:2], Gn, y, vmax, dtype)
    assert st["flag"].tolist() == [2, 2] and st["nan"] and st["k"] == 2
    yn = y.copy()
    yn[0, 0] = np.inf  # under a non-zero g^
    st = K.staging(None, G, yn, vmax, dtype)
    assert st["flag"].tolist() == [2, 0] and st["nan"]
    yn = y.copy()
    yn[0, 1] = np.nan  # under a zero g^: not used
    assert K.staging(None, G, yn, vmax, dtype)["flag"].tolist() == [0, 0]
    # an all-zero batch
    st = K.staging(np.zeros(3, dtype=np.float32), None, None, None, dtype)
    assert st["k"] == 0 and st["e"] == 0 and st["flag"].tolist() == [1, 1, 1] and not st["nan"]
    # scaling a and G by a power of two moves k and nothing else
    a, G2 = np.array([0.3, -1.7], dtype=np.float32), np.array([[0.1, 0.9], [-0.4, 0.2]], dtype=np.float32)
    s0, s1 = K.staging(a, G2, y, vmax, dtype), K.staging(a * 2.0 ** -20, G2 * 2.0 ** -20, y, vmax, dtype)
    assert s1["k"] == s0["k"] - 20 and s1["e"] == s0["e"] and np.array_equal(s1["g_hat"], s0["g_hat"]) and np.array_equal(s1["a"], s0["a"])
    top = np.abs(G2).max() * 2.0 ** -s0["k"]
    assert 1 <= top < 2


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("dot", [False, True])
def test_bound_is_non_negative_and_finite_and_its_g_term_vanishes_for_exact_g(dot, dtype):
    rng = np.random.default_rng(5)
    n, d, nq, c = 600, 33, 17, 5
    x, q = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((nq, d)).astype(np.float32)
    v = rng.standard_normal((n, c)).astype(np.float32)
    a = (rng.standard_normal(nq) * 1e-6).astype(np.float32)
    G = (rng.standard_normal((nq, c)) * 1e-6).astype(np.float32)
    for beta in (1.0, 1.0 / 64.0, 4.0):
        for aa, GG in ((a, None), (None, G), (a, G)):
            b = K.device_bound(q, x, dtype, beta, aa, GG, v if GG is not None else None, dot=dot)
            assert b.shape == (n, d) and np.isfinite(b).all() and (b > 0).all()
    elig = np.zeros((nq, n), dtype=bool)
    assert np.isfinite(K.device_bound(q, x, dtype, 1.0, a, G, v, elig, dot=dot)).all()
    assert K.device_bound(q, x[:0], dtype, 1.0, a).shape == (0, d)
    G16 = (rng.integers(-4, 5, size=(nq, c)) * 2.0 ** -10).astype(np.float32)
    exact = K.device_bound(q, x, dtype, 1.0, None, G16, v, dot=dot)
    inexact = K.device_bound(q, x, dtype, 1.0, None, (G16 * (1 + 2.0 ** -13)).astype(np.float32), v, dot=dot)
    assert (exact <= inexact * (1 + 1e-3)).all() and (exact < inexact).mean() > 0.99
    assert (K.device_bound(q, x, dtype, 1.0, a, G16, v, dot=dot, rel_extra=1e-6) >= K.device_bound(q, x, dtype, 1.0, a, G16, v, dot=dot)).all()
    wide = K.device_bound(q, x, dtype, 1.0, None, G16, v, dot=dot, values_bound=np.full((nq, c), 1.0))  # (far above the flat read-out's own bound)
    assert (wide > exact).all()


def test_host_pieces_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([CLANG, *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=600)
    if probed.returncode != 0:  # (decided on an empty program, before the program under test is built)
        pytest.skip("this toolchain does not link -fsanitize=address,undefined")
    exe = tmp_path / "key_grad_check"
    cmd = [CLANG, *flags, str(ROOT / "tests" / "sanitize" / "key_grad_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


DECLARED = {
    "vodhip_index_posterior_key_gradient": ["index", "queries", "q_dtype", "nq", "beta", "q_labels_dev", "n_per_query", "max_score", "log_rel", "grad_log_z",
                                            "values", "grad_values", "accumulate", "out", "stream"],
    "vodhip_node_index_posterior_key_gradient": ["index", "queries", "q_dtype", "nq", "beta", "q_labels", "n_per_query", "max_score", "log_rel", "grad_log_z",
                                                 "values", "grad_values", "out"],
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


def test_header_with_the_new_section_is_c99_and_corrects_the_adjoints_note():
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", str(ROOT / "include" / "vodhip.h")], check=True)
    header = (ROOT / "include" / "vodhip.h").read_text()
    assert "H2k." in header and "would give it" not in header
    h2a = header[header.index("/* H2a."):header.index("int vodhip_index_posterior_adjoint")]
    assert "log Z term only" in h2a


def test_both_indexes_expose_the_method_and_the_keys_keyword():
    pytest.importorskip("torch")
    from vod_amd.index import HipFlatIndex, HipNodeIndex

    for cls in (HipFlatIndex, HipNodeIndex):
        sig = inspect.signature(cls.key_gradient)
        assert [p for p in sig.parameters][:2] == ["self", "queries"]
        kw = {n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY}
        assert kw == {"grad_log_z", "grad_values", "expectation", "log_partition", "temperature", "subset", "out", "accumulate"}
        assert inspect.signature(cls.read_out).parameters["keys"].default is None
    assert inspect.signature(HipFlatIndex.log_z).parameters["keys"].default is None
