"""`sample_posterior`, the parts that need no GPU:

* the Philox4x32-10 known-answer vectors of the restatement (tests/sample_posterior_ref.py), the counter layout and the range of v;
* statistics of the restatement on a 5-row store with 4096 identical queries that differ only in their stream index: first-draw
  frequencies against the softmax, and at k = 2 the mean of sum_S w f against E_p[f] and of sum_S w against 1 - the seed is picked once
  (1234), every statistic is gated at 4 standard errors;
* `sample_fold.h` semantics through the Python twin of the fold: the merge of per-shard lists equals the sample of the whole store;
* the host fold under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program (tests/sanitize/sample_fold_check.cpp);
  nothing is loaded into Python under a sanitizer;
* the derived key bound is positive, grows with the dot term and covers a float32 emulation of the device's key; a float32 emulation
  of the scan's high-word upper bound (`key_upper`) lies above every key the device can compute, and within 2e-3 of it for small v;
* both new symbols are declared in include/vodhip.h, listed in `_native.SIGNATURES` and exported; the Python methods refuse a bad k
  and a bad seed before any device call.
"""
import pathlib
import re
import subprocess

import numpy as np
import pytest

import partition_ref as P
import sample_posterior_ref as R
from conftest import ROOT

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SEED = 1234


def test_philox_known_answers_and_the_counter_layout():
    out = R.philox4x32_10(0, 0, 0, 0, 0, 0)
    assert [int(w) for w in out] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    out = R.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)  # (Random123 kat_vectors)
    assert [int(w) for w in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    out = R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)
    assert [int(w) for w in out] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # row g reads word g & 3 of counter (g >> 2, g >> 34, qs, j), j = 0: high word, j = 1: low word
    seed = (0x299F31D0 << 32) | 0xA4093822
    for g in (0, 1, 2, 3, 4, 7, (1 << 34) + 6, (5 << 34) + (9 << 2) + 1):
        hi, lo = R.words(seed, 77, g)
        c = g >> 2
        want_hi = R.philox4x32_10(c & 0xFFFFFFFF, c >> 32, 77, 0, seed & 0xFFFFFFFF, seed >> 32)[g & 3]
        want_lo = R.philox4x32_10(c & 0xFFFFFFFF, c >> 32, 77, 1, seed & 0xFFFFFFFF, seed >> 32)[g & 3]
        assert int(hi) == int(want_hi) and int(lo) == int(want_lo), g
    # the noise of (query stream index, global row) does not depend on how the batch or the store is cut
    whole = R.uniforms(SEED, np.arange(40)[:, None], np.arange(1000)[None, :])
    part = R.uniforms(SEED, 17 + np.arange(3)[:, None], 333 + np.arange(50)[None, :])
    assert np.array_equal(whole[17:20, 333:383], part)
    assert whole.min() > 0 and whole.max() <= 1 - 2.0 ** -24 and abs(whole.mean() - 0.5) < 4 / np.sqrt(12 * whole.size)
    assert len(np.unique(whole)) == whole.size


def _five_rows():
    s = np.array([[2.0, 1.0, 0.5, 0.0, -1.5]]).repeat(4096, axis=0)
    p = np.exp(s[0] - s[0].max())
    return s, p / p.sum()


def test_first_draw_frequencies_match_the_softmax():
    s, p = _five_rows()
    r = R.sample_from_scores(s, 1, 1.0, SEED)
    n = len(s)
    freq = np.bincount(r["ids"][:, 0], minlength=5) / n
    z = (freq - p) / np.sqrt(p * (1 - p) / n)
    print("first-draw z scores:", np.round(z, 2))
    assert (np.abs(z) <= 4).all()
    # k = 1 has a threshold (5 > 2 rows): every weight is finite and at least the probability
    assert np.isfinite(r["log_weight"]).all() and (r["log_weight"] >= r["log_p"] - 1e-12).all()


def test_priority_weights_are_unbiased_at_k_2():
    s, p = _five_rows()
    f = np.array([1.0, -2.0, 0.5, 4.0, 3.0])
    r = R.sample_from_scores(s, 2, 1.0, SEED)
    w = np.exp(r["log_weight"])
    assert (r["ids"] >= 0).all() and (r["ids"][:, 0] != r["ids"][:, 1]).all()  # without replacement
    for name, est, want in (("sum w f", (w * f[r["ids"]]).sum(axis=1), float(p @ f)), ("sum w", w.sum(axis=1), 1.0)):
        se = est.std(ddof=1) / np.sqrt(len(est))
        z = (est.mean() - want) / se
        print(f"{name}: mean {est.mean():.5f} want {want:.5f} z {z:.2f}")
        assert abs(z) <= 4, name
    # the inclusion probability of row z is 1 - exp(-p_z / tau): the weight is p_z over it
    tau = np.exp(r["log_tau"])[:, None]
    np.testing.assert_allclose(w, np.exp(r["log_p"]) / -np.expm1(-np.exp(r["log_p"]) / tau), rtol=1e-12)


def test_restatement_pads_eligibility_and_special_scores():
    s = np.array([[1.0, 3.0, np.nan, -np.inf, 2.0], [np.inf, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    elig = np.ones((3, 5), dtype=bool)
    elig[2] = False
    r = R.sample_from_scores(s, 4, 1.0, SEED, eligible=elig)
    assert sorted(r["ids"][0][:3]) == [0, 1, 4] and r["ids"][0][3] == -1  # NaN and -inf rows are never drawn; 3 rows < k: a pad
    assert np.isneginf(r["log_tau"][0]) and np.array_equal(r["log_weight"][0][:3], r["log_p"][0][:3])
    assert abs(np.exp(r["log_p"][0][:3]).sum() - 1) < 1e-12 and np.isneginf(r["keys"][0][3:]).all()
    assert (np.diff(r["keys"][0][:3]) <= 0).all()
    for a in (1, 2):  # a +inf score / no eligible row: all pads
        assert (r["ids"][a] == -1).all() and np.isneginf(r["keys"][a]).all() and np.isneginf(r["log_weight"][a]).all()
    # id_base shifts the ids and the noise together: a slice of the store draws what the whole store would restricted to it
    rng = np.random.default_rng(5)
    s = rng.standard_normal((6, 300))
    whole = R.keys_from_scores(s, 1.0, SEED, query_offset=9)[0]
    part = R.keys_from_scores(s[:, 100:180], 1.0, SEED, query_offset=9, id_base=100)[0]
    assert np.array_equal(whole[:, 100:180], part)
    got = R.sample_from_scores(s[:, 100:180], 5, 1.0, SEED, query_offset=9, id_base=100)
    assert ((got["ids"] >= 100) & (got["ids"] < 180)).all()
    assert R.sample_from_scores(np.zeros((2, 0)), 3, 1.0, SEED)["ids"].shape == (2, 3)


@pytest.mark.parametrize("k", [1, 4, 32])
@pytest.mark.parametrize("cuts", [(0, 700), (0, 350, 700), (0, 10, 20, 700), (0, 0, 700, 700)])
def test_the_fold_of_shard_lists_equals_the_sample_of_the_whole_store(cuts, k):
    rng = np.random.default_rng(k + len(cuts))
    s = np.round(rng.standard_normal((9, 700)) * 4) / 2  # many equal scores
    beta = 0.5
    s32 = s.astype(np.float32)
    whole = R.sample_from_scores(s, k, beta, SEED, query_offset=3)
    shards = [R.sample_from_scores(s[:, a:b], k, beta, SEED, query_offset=3, id_base=a) for a, b in zip(cuts, cuts[1:])]
    for q in range(len(s)):
        m, lr = np.float32(whole["max"][q]), np.float32(whole["log_rel"][q])
        ids, sc, lp, lw, keys = R.fold_sample([sh["keys"][q].astype(np.float32) for sh in shards], [sh["ids"][q] for sh in shards],
                                              [sh["scores"][q].astype(np.float32) for sh in shards], k, beta, m, lr)
        assert np.array_equal(ids, whole["ids"][q]) and np.array_equal(sc, s32[q][ids])
        assert np.array_equal(keys, whole["keys"][q].astype(np.float32))
        np.testing.assert_allclose(lp, whole["log_p"][q], rtol=0, atol=2e-6)
        np.testing.assert_allclose(lw, whole["log_weight"][q], rtol=0, atol=2e-5)  # (the float32 keys move log_tau by 1e-6)
    dead = R.fold_sample([sh["keys"][0].astype(np.float32) for sh in shards], [sh["ids"][0] for sh in shards],
                         [sh["scores"][0].astype(np.float32) for sh in shards], k, beta, np.float32(np.inf), np.float32(np.inf))
    assert (dead[0] == -1).all() and all(np.isneginf(a).all() for a in dead[1:])


def _device_key_f32(s32, beta, hi, lo):
    """the device's key in NumPy float32 arithmetic (log1p / log of NumPy's float32 loops stand in for the library's)"""
    v = (((hi.astype(np.float64) * 2.0 ** 32 + lo.astype(np.float64)) + 0.5) * 2.0 ** -64).astype(np.float32)
    v = np.minimum(v, np.float32(1 - 2.0 ** -24))
    e = -np.log1p(-v)
    assert e.dtype == np.float32
    return (np.float32(beta) * s32.astype(np.float32)).astype(np.float32) - np.log(e)


def test_device_key_bound_is_positive_monotone_and_covers_a_float32_emulation():
    rng = np.random.default_rng(2)
    q = rng.integers(-8, 9, size=(20, 65)).astype(np.float32)
    x = rng.integers(-8, 9, size=(500, 65)).astype(np.float32)
    s = P.scores(q, x, "float16")
    for beta in (1.0 / 64.0, 1.0, 4.0):
        exact = R.key_bound(q, x, "float16", beta, SEED, dot=False)
        full = R.key_bound(q, x, "float16", beta, SEED, dot=True)
        assert exact.shape == (20, 500) and (exact > 0).all() and (full > exact).all() and np.isfinite(full).all()
        hi, lo = R.words(SEED, np.arange(20)[:, None], np.arange(500)[None, :])
        key64 = R.keys_from_scores(s, beta, SEED)[0]
        err = np.abs(_device_key_f32(s.astype(np.float32), beta, hi, lo).astype(np.float64) - key64)
        print(f"beta {beta:g}: float32 emulation max err / bound = {(err / exact).max():.3f}")
        assert (err <= exact).all()
    # at the two ends of v: the slope of E near 1 and the relative rounding near 2^-65 are inside the bound's own evaluation
    v = np.array([[2.0 ** -65, 2.0 ** -40, 0.5, 1 - 2.0 ** -20, 1 - 2.0 ** -24]])
    b = R.device_key_bound(np.zeros((1, 5)), np.zeros((1, 5)), 64, 1.0, v, dot=False)
    assert (b > 0).all() and b[0, 4] > 100 * b[0, 2] and b[0, 4] < 0.1 and b[0, 0] < 1e-5


def _key_upper_f32(s32, beta, hi):
    """`key_upper` of kernels_sample_posterior.hip in NumPy float32 arithmetic (np.log2 stands in for the native log2)"""
    f = np.float32
    hm = (hi & np.uint64(0xFFFFFF00)).astype(np.float32)
    t1 = (f(beta) * s32.astype(np.float32)).astype(np.float32)
    with np.errstate(divide="ignore"):
        vl = hm * f(2.0 ** -32)
        x = f(0.5) * vl
        nl = f(-0.69314718) * np.log2(vl) - (x - f(0.5) * x * x)
        ub = t1 + nl + ((np.abs(t1) + f(32)) * f(2.0 ** -21) + f(2e-4))
    assert ub.dtype == np.float32
    return np.where(hm == 0, np.inf, ub)


def test_the_high_word_bound_is_above_every_key_the_device_can_compute():
    rng = np.random.default_rng(8)
    n = 400_000
    hi = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    hi[: n // 4] >>= rng.integers(0, 32, size=n // 4).astype(np.uint64)  # small v: where the large keys live
    hi[:8] = [0, 1, 255, 256, 257, 0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFEFF]
    s = np.round(rng.standard_normal(n) * 300).astype(np.float64)
    for beta in (2.0 ** -7, 1.0, 4.0):
        for lo in (np.zeros(n, dtype=np.uint64), np.full(n, 0xFFFFFFFF, dtype=np.uint64), rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)):
            v = np.minimum((hi.astype(np.float64) * 2.0 ** 32 + lo.astype(np.float64) + 0.5) * 2.0 ** -64, R.V_MAX)
            key64 = beta * s + R.neg_log_e(v)
            tol = R.device_key_bound(s[None, :], np.zeros((1, n)), 64, beta, v[None, :], dot=False)[0]
            ub = _key_upper_f32(s.astype(np.float32), beta, hi).astype(np.float64)
            native = 2.0 ** -22 * 32 * 0.7  # the native log2 against np.log2: 2^-22 relative of at most 32, times ln 2
            slack = ub - native - (key64 + tol)
            assert (slack > 0).all(), (beta, slack.min())
            fin = np.isfinite(ub) & (v < 0.05)
            print(f"beta {beta:g}: the bound sits {np.median(slack[fin]):.2e} (median), {slack[fin].max():.2e} (max) above the key for v < 0.05")
            assert np.median(slack[fin]) < 2e-3  # ... and it is tight where it matters


def test_shard_merge_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    if not pathlib.Path(CLANG).exists():
        pytest.skip("ROCm clang++ not available")
    exe = tmp_path / "sample_fold_check"
    cmd = [CLANG, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           str(ROOT / "tests" / "sanitize" / "sample_fold_check.cpp"), "-I", str(ROOT / "vod_amd" / "csrc"), "-o", str(exe)]
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

    header = (ROOT / "include" / "vodhip.h").read_text()
    for name in ("vodhip_index_sample_posterior", "vodhip_node_index_sample_posterior"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _native.SIGNATURES
    assert len(_native.SIGNATURES["vodhip_index_sample_posterior"][1]) == 19
    assert len(_native.SIGNATURES["vodhip_node_index_sample_posterior"][1]) == 17
    assert re.search(r"#define\s+VODHIP_SAMPLE_SLACK_TILES\s+2\b", header)
    lib = _native.load_library()
    assert hasattr(lib, "vodhip_index_sample_posterior") and hasattr(lib, "vodhip_node_index_sample_posterior")


def test_python_refusals_that_need_no_device():
    from vod_amd import index as I

    assert I.PosteriorSample._fields == ("ids", "scores", "log_p", "log_weight", "log_tau", "keys", "log_partition")

    class Stub(I.HipFlatIndex):  # no handle: every refusal below comes before the first native call
        def __init__(self):
            self.dim, self.device = 4, "cpu"

        def _prep_queries(self, queries):
            return queries

        def __del__(self):
            pass

    import torch

    q = torch.zeros((2, 4))
    for k in (0, 256, -1):
        with pytest.raises(ValueError, match=r"k must be in \[1, 255\]"):
            Stub().sample_posterior(q, k, seed=1)
    for seed in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="seed must be in"):
            Stub().sample_posterior(q, 3, seed=seed)
    with pytest.raises(TypeError):
        Stub().sample_posterior(q, 3)  # the seed is required
    with pytest.raises(ValueError, match="expected subset labels"):
        Stub().sample_posterior(q, 3, seed=1, subset=np.zeros((3, 2), dtype=np.int32))
