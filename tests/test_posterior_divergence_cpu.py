"""`posterior_divergence` and `kl_to`, the parts that need no GPU:

* the float64 restatement (tests/divergence_ref.py) equals naive float64 `sum p (log p - log r)` on small inputs, kl >= 0, kl == 0 for
  identical pairs, the closed form of one query at two temperatures on a two-valued score vector, eligibility / NaN row / -inf on both
  sides / -inf on one side under mass (+inf KL) / +inf / no row behave as the contract states;
* `posterior_divergence_words` forms the derived words in the stated grouping (0.0 exactly for identical words, NaN and +inf pass);
* the derived bounds grow with n, with the width and with beta;
* the host fold of per-shard words (vod_amd/csrc/divergence_fold.h) under AddressSanitizer and UndefinedBehaviorSanitizer, as a
  stand-alone program (tests/sanitize/divergence_fold_check.cpp); nothing is loaded into Python under a sanitizer;
* both new symbols are declared in include/vodhip.h, listed in `_native.SIGNATURES` with the header's argument counts, and exported;
* `kl_to` with a NumPy-backed fake index: grad_student equals torch autograd of the dense float64 KL, no `posterior_mean` call is made
  when the student does not require grad, no gradient flows to the teacher, rows whose KL is not finite get zero gradient.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch

import divergence_ref as D
import partition_ref as P
import stats_ref as S
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _small(seed, n, d, nq=7, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((scale * rng.standard_normal((nq, d))).astype(np.float32), (scale * rng.standard_normal((nq, d))).astype(np.float32),
            (scale * rng.standard_normal((n, d))).astype(np.float32))


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("n,d,beta_a,beta_b", [(1, 3, 1.0, 1.0), (5, 1, 4.0, 1.0), (37, 16, 0.25, 2.0), (300, 65, 1.0, 1.0 / 64)])
def test_restatement_matches_naive_float64_kl(n, d, beta_a, beta_b, dtype):
    qa, qb, x = _small(n + d, n, d)
    ref = D.posterior_divergence(qa, qb, x, dtype, beta_a, beta_b)
    sa, sb = P.scores(qa, x, dtype), P.scores(qb, x, dtype)
    ent_a, ent_b, ce_ab, ce_ba, kl_ab, kl_ba = D.derived(ref.words, beta_a, beta_b)
    scale = 1.0 + (beta_a + beta_b) * (np.abs(sa).max() + np.abs(sb).max())
    np.testing.assert_allclose(kl_ab, D.naive_kl(sa, sb, beta_a, beta_b), rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(kl_ba, D.naive_kl(sb, sa, beta_b, beta_a), rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(ce_ab - ent_a, kl_ab, rtol=0, atol=1e-12 * scale)
    assert (kl_ab >= 0).all() and (kl_ba >= 0).all() and (ce_ab >= ent_a - 1e-12 * scale).all()
    # each side's words are stats_ref's, the cross words are <= 0, the cross variances >= 0
    for side, s, beta in ((0, sa, beta_a), (4, sb, beta_b)):
        for got, want in zip(ref.words[side : side + 3], S.from_scores(s, beta)[:3]):
            np.testing.assert_array_equal(got, want)
    assert (ref.words[3] <= 0).all() and (ref.words[7] <= 0).all() and (ref.cvar_ab >= 0).all() and (ref.cvar_ba >= 0).all()
    assert (ref.n == n).all()
    if n == 1:
        assert all((w == 0).all() for w in (kl_ab, kl_ba, ref.words[3], ref.words[7]))
    # identical pairs: kl == 0.0 exactly, the cross word is mean_rel
    same = D.posterior_divergence(qa, qa, x, dtype, beta_a, beta_a)
    d6 = D.derived(same.words, beta_a, beta_a)
    assert (d6[4] == 0.0).all() and (d6[5] == 0.0).all()
    np.testing.assert_array_equal(same.words[3], same.words[2])
    np.testing.assert_array_equal(same.words[7], same.words[6])


def test_one_query_at_two_temperatures_has_the_closed_form_on_a_two_valued_score_vector():
    # k rows score h, n - k rows score 0: p_hi(beta) = k e^{beta h} / (k e^{beta h} + n - k) and KL(p || r) is the Bernoulli KL of the two
    n, k, h = 1200, 10, 3.0
    s = np.zeros((1, n))
    s[0, 800:810] = h
    for beta_a, beta_b in ((1.0, 1.0 / 64), (4.0, 1.0), (1.0 / 64, 4.0)):
        ref = D.from_scores(s, s, beta_a, beta_b)
        pa = k * np.exp(beta_a * h) / (k * np.exp(beta_a * h) + n - k)
        pb = k * np.exp(beta_b * h) / (k * np.exp(beta_b * h) + n - k)
        want = pa * np.log(pa / pb) + (1 - pa) * np.log((1 - pa) / (1 - pb))
        d6 = D.derived(ref.words, beta_a, beta_b)
        np.testing.assert_allclose(d6[4], want, rtol=1e-11)
        np.testing.assert_allclose(ref.words[3], -(1 - pa) * h, rtol=1e-12)
        np.testing.assert_allclose(ref.cvar_ab, h * h * pa * (1 - pa), rtol=1e-10)


def test_restatement_eligibility_nan_inf_and_no_row():
    qa, qb, x = _small(3, 40, 8, nq=4)
    sa, sb = P.scores(qa, x, "float16"), P.scores(qb, x, "float16")
    elig = np.zeros((4, 40), dtype=bool)
    elig[0, ::4] = True
    elig[1, 5] = True
    elig[3] = True
    ref = D.posterior_divergence(qa, qb, x, "float16", 2.0, 0.5, elig)
    sub = D.from_scores(sa[:1, ::4], sb[:1, ::4], 2.0, 0.5)
    for got, want in zip(ref.words, sub.words):
        assert got[0] == want[0]
    w1 = [w[1] for w in ref.words]
    assert w1 == [sa[1, 5], 0.0, 0.0, 0.0, sb[1, 5], 0.0, 0.0, 0.0]  # one row
    w2 = [w[2] for w in ref.words]
    assert w2[0] == -np.inf and w2[1] == -np.inf and w2[4] == -np.inf and w2[5] == -np.inf and all(np.isnan(w2[k]) for k in (2, 3, 6, 7))
    assert list(ref.n) == [10, 1, 0, 40]
    # a NaN against ONE side leaves the row out of BOTH
    s2 = sa.copy()
    s2[:, 7] = np.nan
    keep = np.ones(40, dtype=bool)
    keep[7] = False
    for got, want in zip(D.from_scores(s2, sb, 2.0, 0.5).words, D.from_scores(sa[:, keep], sb[:, keep], 2.0, 0.5).words):
        np.testing.assert_array_equal(got, want)
    for got, want in zip(D.from_scores(sb, s2, 2.0, 0.5).words, D.from_scores(sb[:, keep], sa[:, keep], 2.0, 0.5).words):
        np.testing.assert_array_equal(got, want)
    ninf, inf = -np.inf, np.inf
    a = np.array([[1.0, ninf, -2.0], [1.0, 0.0, -2.0], [1.0, 0.5, -2.0], [ninf, ninf, ninf], [1.0, 2.0, 3.0], [1.0, 2.0, 3.0]])
    b = np.array([[0.0, ninf, 1.0], [0.0, ninf, 1.0], [0.0, inf, 1.0], [0.0, 1.0, 2.0], [0.0, 1.0, 2.0], [0.0, 1.0, 2.0]])
    r = D.from_scores(a, b, 1.0, 1.0, np.array([[True] * 3] * 5 + [[False] * 3]))
    d6 = D.derived(r.words, 1.0, 1.0)
    two = D.from_scores(a[:1, [0, 2]], b[:1, [0, 2]], 1.0, 1.0)
    # pair 0: -inf on both sides adds nothing and makes no NaN
    assert all(r.words[k][0] == two.words[k][0] and np.isfinite(two.words[k][0]) for k in range(8))
    # pair 1: -inf on side b under mass of side a: cross_rel_ab = -inf, H(p, r) = KL(p || r) = +inf; the other direction stays finite
    assert r.words[3][1] == ninf and d6[2][1] == inf and d6[4][1] == inf and np.isfinite(r.words[7][1]) and np.isfinite(d6[5][1])
    assert np.isfinite(r.words[2][1]) and np.isfinite(r.words[6][1])
    # pair 2: +inf on side b: (+inf, +inf, NaN), both cross words NaN, side a's three words intact
    assert r.words[4][2] == inf and r.words[5][2] == inf and np.isnan(r.words[6][2]) and np.isnan(r.words[3][2]) and np.isnan(r.words[7][2])
    assert all(r.words[k][2] == S.from_scores(a[2:3], 1.0)[k][0] for k in range(3))
    # pair 3: side a all -inf counts as no row on that side; pairs 4 (fine) and 5 (no eligible row)
    assert r.words[0][3] == ninf and r.words[1][3] == ninf and np.isnan(r.words[2][3]) and np.isnan(r.words[3][3]) and np.isnan(r.words[7][3])
    assert all(r.words[4 + k][3] == S.from_scores(b[3:4], 1.0)[k][0] for k in range(3))
    assert all(np.isfinite(r.words[k][4]) for k in range(8)) and d6[4][4] == 0.0  # (b = a - 1: the same posterior)
    assert r.words[0][5] == ninf and r.words[4][5] == ninf and all(np.isnan(r.words[k][5]) for k in (2, 3, 6, 7))
    e = D.posterior_divergence(qa, qb, x[:0], "float16", 1.0, 1.0)
    assert np.isneginf(e.words[0]).all() and np.isneginf(e.words[5]).all() and np.isnan(e.words[3]).all() and np.isnan(e.words[6]).all()


def test_the_derived_words_are_formed_in_the_stated_grouping():
    from vod_amd.index import posterior_divergence_words

    rng = np.random.default_rng(4)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    base = [rng.standard_normal(6).astype(np.float32) for _ in range(4)]
    base[1], base[2], base[3] = np.abs(base[1]), -np.abs(base[2]), -np.abs(base[2])
    words = [w.copy() for w in base + base]  # identical pairs: cross_rel == mean_rel, the same words on both sides
    for beta in (1.0 / 64, 1.0 / 3, 4.0):
        for conv in (lambda t: t, torch.from_numpy):
            r = posterior_divergence_words(tuple(conv(w.copy()) for w in words), beta, beta)
            kl_ab, kl_ba = np.asarray(r.kl_ab), np.asarray(r.kl_ba)
            assert kl_ab.dtype == np.float32 and (kl_ab == 0.0).all() and (kl_ba == 0.0).all()
            np.testing.assert_array_equal(np.asarray(r.entropy_a), np.asarray(r.cross_entropy_ab))
    words = [np.array(v, dtype=np.float32) for v in
             ([1, 1, 1, -inf], [0.5, 0.5, 0.5, -inf], [-0.25, -0.25, -0.25, nan], [-0.5, -inf, nan, nan],
              [2, 2, inf, 2], [0.75, 0.75, inf, 0.75], [-0.125, -0.125, nan, -0.125], [-1.0, -1.0, nan, nan])]
    for conv in (lambda t: t, torch.from_numpy):
        r = posterior_divergence_words(tuple(conv(w.copy()) for w in words), 2.0, 0.5)
        got = [np.asarray(t) for t in r[:6]]
        want = D.derived(tuple(w.astype(np.float64) for w in words), 2.0, 0.5)
        for g, w in zip(got, (want[4], want[5], want[2], want[3], want[0], want[1])):
            np.testing.assert_array_equal(g, w.astype(np.float32))
        assert got[0][1] == inf and got[2][1] == inf and np.isnan(got[0][2]) and np.isnan(got[0][3]) and np.isnan(got[1][3])
        assert np.asarray(r.stats_a.log_partition.log_z)[3] == -inf and np.asarray(r.stats_b.log_partition.log_z)[2] == inf
        np.testing.assert_array_equal(np.asarray(r.stats_a.log_partition.log_z)[:2], np.float32([2.5, 2.5]))
    # a negative rounding residue is clamped to 0
    words = [np.float32([v]) for v in (1.0, 0.5, -0.25, -0.25 + 2.0 ** -20, 1.0, 0.5, -0.25, -0.25)]
    assert posterior_divergence_words(tuple(words), 1.0, 1.0).kl_ab[0] == 0.0


def test_bounds_are_monotone_in_n_dim_and_beta():
    qa, qb, x = _small(5, 64, 200, nq=9)
    cross, sigma, spread = -np.linspace(0.5, 30.0, 9), np.linspace(0.1, 3.0, 9), np.linspace(5.0, 60.0, 9)

    def cb(q_own, q_other, xx, beta, n, c=cross, dot=True, **k):
        if not dot:
            return D.cross_bound(beta, n, c, spread, **k)
        return D.cross_bound(beta, n, c, spread, P.dot_bound(q_own, xx, "float16"), P.dot_bound(q_other, xx, "float16"), sigma, **k)

    by_n = [cb(qa, qb, x, 1.0, n) for n in (1, 257, 3000, 10 ** 6, 10 ** 9)]
    assert all((a <= b).all() for a, b in zip(by_n, by_n[1:])) and (by_n[0] < by_n[-1]).all()
    by_d = [cb(qa[:, :d], qb[:, :d], x[:, :d], 1.0, 64) for d in (1, 64, 65, 128, 200)]
    assert all((a <= b).all() for a, b in zip(by_d, by_d[1:])) and (by_d[0] < by_d[-1]).all()
    by_b = [cb(qa, qb, x, b, 64) for b in (1 / 64, 1.0, 4.0)]
    assert all((a < b).all() for a, b in zip(by_b, by_b[1:]))
    # without the dot-product part the bound is the arithmetic of posterior_stats' accumulator a: the same share of the word's magnitude
    a = cb(qa, qb, x, 1.0, 3000, dot=False)
    mean_bound = S.device_bound(np.zeros((9, 1)), None, None, 1.0, 3000, cross, np.zeros(9), dot=False)[0]
    np.testing.assert_allclose(a, mean_bound, rtol=1e-6)
    assert (a <= 1000 * S.U * np.abs(cross)).all() and (a >= 800 * S.U * np.abs(cross)).all()
    assert (a < cb(qa, qb, x, 1.0, 3000)).all() and (a < cb(qa, qb, x, 1.0, 3000, dot=False, node=True)).all()
    assert (cb(qa, qb, x, 1.0, 64, c=2 * cross) > cb(qa, qb, x, 1.0, 64)).all()
    # the full set: eight words, six derived words, all growing with n
    ref = D.posterior_divergence(qa, qb, x, "float16", 1.0, 0.5)
    b8 = D.bounds(qa, qb, x, "float16", 1.0, 0.5, ref)
    big = ref._replace(n=ref.n * 1000)
    assert all((u <= v).all() for u, v in zip(b8, D.bounds(qa, qb, x, "float16", 1.0, 0.5, big)))
    b6 = D.derived_bounds(1.0, 0.5, ref.words, b8)
    assert len(b8) == 8 and len(b6) == 6 and all((b > 0).all() and np.isfinite(b).all() for b in b8 + b6)
    assert (b6[4] >= b8[1] + b8[5] + 1.0 * b8[2] + 0.5 * b8[3]).all()


def test_shard_fold_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "divergence_fold_check"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "sanitize" / "divergence_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if built.returncode != 0 and "sanitizer" in built.stderr.lower() and "unsupported" in built.stderr.lower():
        pytest.skip("-fsanitize=address,undefined is not supported by this toolchain")
    assert built.returncode == 0, built.stderr[-3000:]
    env = {"ASAN_OPTIONS": "detect_leaks=1 exitcode=66", "UBSAN_OPTIONS": "print_stacktrace=1", "PATH": "/usr/bin:/bin"}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    text = out.stdout + out.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert out.returncode == 0 and " 0 errors" in out.stdout, text[-2000:]


def test_both_symbols_are_declared_listed_and_exported():
    from vod_amd import _native

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vodhip.h").read_text(), flags=re.S)
    for name in ("vodhip_index_posterior_divergence", "vodhip_node_index_posterior_divergence"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == n_args, (name, n_args)
    assert len(_native.SIGNATURES["vodhip_index_posterior_divergence"][1]) == 18
    assert len(_native.SIGNATURES["vodhip_node_index_posterior_divergence"][1]) == 17
    lib = _native.load_library()
    assert hasattr(lib, "vodhip_index_posterior_divergence") and hasattr(lib, "vodhip_node_index_posterior_divergence")


class _FakeIndex:
    """NumPy-backed: float64 words of the dense scores, returned as NumPy arrays as a node index returns them."""

    def __init__(self, x):
        self.x = x
        self.mean_calls = self.div_calls = 0

    def posterior_divergence(self, queries_a, queries_b, temperature_a, temperature_b, subset):
        from vod_amd.index import posterior_divergence_words

        assert not queries_a.requires_grad and not queries_b.requires_grad and subset is None
        self.div_calls += 1
        ref = D.from_scores(queries_a.double().numpy() @ self.x.T, queries_b.double().numpy() @ self.x.T, 1.0 / temperature_a, 1.0 / temperature_b)
        return posterior_divergence_words(ref.words, 1.0 / temperature_a, 1.0 / temperature_b)

    def posterior_mean(self, queries, temperature, subset):
        from vod_amd.index import LogPartition, PosteriorMean

        assert not queries.requires_grad and subset is None
        self.mean_calls += 1
        beta = 1.0 / temperature
        s = queries.double().numpy() @ self.x.T
        m, r = P.from_scores(s, beta)
        with np.errstate(invalid="ignore"):
            p = np.exp(beta * (s - m[:, None]) - r[:, None])
        return PosteriorMean(np.nan_to_num(p) @ self.x, LogPartition(beta * m + r, m, r))


def test_kl_to_matches_dense_float64_autograd_and_touches_only_the_student():
    from vod_amd.index import _KlTo, kl_to_backward

    rng = np.random.default_rng(21)
    x = rng.standard_normal((50, 12))
    xt = torch.from_numpy(x)
    w = torch.from_numpy(rng.standard_normal(6))
    for t_s, t_t in ((1.0, 1.0), (0.5, 2.0), (4.0, 0.25)):  # (exact in float32: the fake index sees the betas the formula uses)
        teacher = torch.from_numpy(rng.standard_normal((6, 12))).requires_grad_(True)
        student = torch.from_numpy(rng.standard_normal((6, 12))).requires_grad_(True)
        lp = torch.log_softmax(teacher.detach() @ xt.T / t_t, dim=1)
        lr = torch.log_softmax(student @ xt.T / t_s, dim=1)
        dense = (lp.exp() * (lp - lr)).sum(dim=1)
        (dense * w).sum().backward()

        fake = _FakeIndex(x)
        s2 = student.detach().clone().requires_grad_(True)
        out = _KlTo.apply(s2, fake, teacher, t_s, t_t, None)
        assert out.shape == (6,) and out.dtype == torch.float32 and out.requires_grad
        torch.testing.assert_close(out.double(), dense.detach(), rtol=0, atol=2e-7 * float(1 + dense.detach().max()))
        (out * w).sum().backward()
        assert (fake.div_calls, fake.mean_calls) == (1, 2)
        assert s2.grad.dtype == student.grad.dtype
        torch.testing.assert_close(s2.grad, student.grad, rtol=0, atol=4e-7 * float(student.grad.abs().max()))  # (the formula runs in float32)
        assert teacher.grad is None  # the teacher is a constant

        # the student does not require grad: no posterior_mean call, nothing to differentiate
        fake = _FakeIndex(x)
        out = _KlTo.apply(student.detach(), fake, teacher.detach(), t_s, t_t, None)
        assert (fake.div_calls, fake.mean_calls) == (1, 0) and not out.requires_grad
        # the gradient is cast to the student's dtype
        s3 = student.detach().float().requires_grad_(True)
        (_KlTo.apply(s3, _FakeIndex(x), teacher.detach().float(), t_s, t_t, None) * w.float()).sum().backward()
        assert s3.grad.dtype == torch.float32
        torch.testing.assert_close(s3.grad.double(), student.grad, rtol=0, atol=2e-5 * float(student.grad.abs().max()))
    # rows whose KL is not finite get zero gradient, whatever grad_out and the means hold
    g = kl_to_backward(torch.tensor([2.0, float("nan"), 3.0, 1.0]), torch.tensor([[1.5, 1.0], [float("nan"), 1.0], [2.0, 2.0], [1.0, 1.0]]),
                       torch.tensor([[0.5, 2.0], [1.0, 1.0], [float("inf"), 0.0], [0.0, 0.0]]),
                       torch.tensor([0.25, float("nan"), float("inf"), 0.0]), 0.5, torch.float64)
    assert g.dtype == torch.float64 and g.tolist() == [[1.0, -1.0], [0.0, 0.0], [0.0, 0.0], [0.5, 0.5]]
