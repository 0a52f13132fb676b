"""GPU parity tests for labeled priority sampling (H7) against the golden vectors produced by the reference's
`_labeled_priority_sampling_2d_` with explicit noise, and against the CPU oracle on random cases.

Selected columns / labels: exact wherever the reference's weight is finite (slots whose key is -inf / NaN are
padding-like; numpy's order among equal keys is unspecified).  Log-weights and lse: rtol/atol 2e-5 (float32
exp/log and tree vs sequential sums)."""
import json

import numpy as np
import pytest

from conftest import GOLDEN

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
TOL = dict(rtol=2e-5, atol=2e-5)


def _run(scores, labels, noise, p, support="reference"):
    from vod_amd.core.sample import labeled_priority_sampling_tensors

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out = labeled_priority_sampling_tensors(
        t(scores), t(labels), t(noise), p["k_positive"], p["k_total"], normalized=True, temperature=p["temperature"],
        max_support_size=p["max_support_size"], support=support,
    )
    return [o.cpu().numpy() for o in out]


def _compare(got, ref):
    smp, logw, lab, lse = got
    r_smp, r_logw, r_lab, r_lse = ref
    finite = np.isfinite(r_logw)
    np.testing.assert_array_equal(smp[finite], r_smp[finite])
    np.testing.assert_array_equal(lab, r_lab)
    np.testing.assert_array_equal(smp < 0, r_smp < 0)            # same number of samples per row
    np.testing.assert_array_equal(np.isfinite(logw), finite)
    np.testing.assert_allclose(logw[finite], r_logw[finite], **TOL)
    both = np.isfinite(r_lse)
    np.testing.assert_array_equal(np.isfinite(lse), both)
    np.testing.assert_allclose(lse[both], r_lse[both], **TOL)
    for r in range(smp.shape[0]):  # no duplicate columns in a row
        v = smp[r][smp[r] >= 0]
        assert len(set(v.tolist())) == len(v)


def test_matches_reference_golden():
    g = np.load(GOLDEN / "sampling_fixed_noise.npz")
    cases = json.loads((GOLDEN / "manifest.json").read_text())["sampling_fixed_noise"]["params"]["cases"]
    for c, p in enumerate(cases):
        # the fixture holds what the reference's inner function received: max_support_size already raised to k_total
        got = _run(g[f"scores_{c}"], g[f"labels_{c}"], g[f"noise_{c}"], p)
        _compare(got, (g[f"out_samples_{c}"], g[f"out_logw_{c}"], g[f"out_labels_{c}"], g[f"out_lse_{c}"]))


@pytest.mark.parametrize("nq,n,k_pos,k_tot,support,temp", [
    (64, 385, 8, 32, 100, 1.0),   # shipped training shape: merged width 385, support 100
    (64, 385, 8, 32, -1, 1.0),
    (16, 1000, 16, 64, -1, 0.0),  # deterministic top-k
    (8, 40, 8, 64, -1, 1.0),      # fewer candidates than k_total
    (5, 4096, 32, 128, 2000, 0.5),
])
def test_matches_oracle_random(nq, n, k_pos, k_tot, support, temp):
    from oracle.sampling import labeled_priority_sampling_2d

    rng = np.random.default_rng(nq + n)
    scores = (rng.normal(size=(nq, n)) * 3).astype(np.float32)
    scores[rng.uniform(size=scores.shape) < 0.1] = -np.inf
    labels = rng.uniform(size=scores.shape) < 0.05
    noise = rng.exponential(size=scores.shape).astype(np.float32)
    p = {"k_positive": k_pos, "k_total": k_tot, "temperature": temp, "max_support_size": support}
    got = _run(scores, labels, noise, p)
    sup = max(support, k_tot) if support >= 0 else -1
    ref = labeled_priority_sampling_2d(scores, labels, noise, k_pos, k_tot, True, temp, sup)
    _compare(got, ref)


@pytest.mark.parametrize("nq,n,k_pos,k_tot,support,temp", [
    (64, 385, 8, 32, 100, 1.0),   # shipped training shape
    (16, 1000, 16, 64, 200, 0.0),
    (5, 4096, 32, 128, 2000, 0.5),
    (8, 300, 4, 16, 16, 1.0),     # support = k_total: the sample is the support
])
def test_corrected_support_mode_keeps_the_best_candidates(nq, n, k_pos, k_tot, support, temp):
    """the reference's truncation REMOVES each class's `max_support_size` best candidates; `support="keep_top"` keeps
    them instead.  Against the oracle's restatement of that mode (the same code with the comparison turned around), and by its
    defining property: every sampled column ranks among its class's `support` best scores."""
    from oracle.sampling import labeled_priority_sampling_2d

    rng = np.random.default_rng(7 * nq + n)
    scores = (rng.normal(size=(nq, n)) * 3).astype(np.float32)
    scores[rng.uniform(size=scores.shape) < 0.1] = -np.inf
    labels = rng.uniform(size=scores.shape) < 0.3
    noise = rng.exponential(size=scores.shape).astype(np.float32)
    p = {"k_positive": k_pos, "k_total": k_tot, "temperature": temp, "max_support_size": support}
    got = _run(scores, labels, noise, p, support="keep_top")
    sup = max(support, k_tot)
    _compare(got, labeled_priority_sampling_2d(scores, labels, noise, k_pos, k_tot, True, temp, sup, keep_top=True))
    smp, logw, lab, _ = got
    for r in range(nq):
        for cls in (True, False):
            members = np.flatnonzero(labels[r] == cls)
            if len(members) <= sup:
                continue
            thr = np.sort(scores[r][members])[-sup]
            picked = smp[r][(smp[r] >= 0) & (lab[r] == cls) & np.isfinite(logw[r])]
            assert np.all(scores[r][picked] >= thr)
    # and the reference mode on the same inputs picks from the OTHER end (the quirk, kept as the default)
    ref_mode = _run(scores, labels, noise, p)
    assert not np.array_equal(ref_mode[0], smp)


def test_sample_search_results_wrapper_contract():
    from vod_amd import types as vt
    from vod_amd.core.sample import sample_search_results

    rng = np.random.default_rng(0)
    nq, w = 6, 50
    idx = np.stack([rng.choice(1000, size=w, replace=False) for _ in range(nq)]).astype(np.int64)
    scr = rng.normal(size=(nq, w)).astype(np.float32)
    idx[:, -1], scr[:, -1] = -1, -np.inf  # the merge's trailing pad column
    lbl = (rng.uniform(size=(nq, w)) < 0.1).astype(np.int64)
    raw = {"dense": rng.normal(size=(nq, w)).astype(np.float32), "sparse": rng.normal(size=(nq, w)).astype(np.float32)}
    np.random.seed(123)
    out = sample_search_results(search_results=vt.RetrievalBatch(scores=scr, indices=idx, labels=lbl), raw_scores=raw,
                                total=16, max_pos_sections=4, temperature=1.0, max_support_size=None)
    assert out.batch.indices.shape == (nq, 16) and out.log_weights.shape == (nq, 16)
    assert out.batch.labels.dtype == np.bool_ and out.lse_pos.shape == (nq,) and out.max_sampling_id.shape == (nq,)
    for r in range(nq):
        assert len(set(out.batch.indices[r].tolist())) == 16            # without replacement
        pos = out.batch.labels[r]
        assert np.all(lbl[r][[list(idx[r]).index(i) for i in out.batch.indices[r][pos]]] > 0)
        for name in raw:                                                   # raw scores follow the sampled ids
            cols = [list(idx[r]).index(i) for i in out.batch.indices[r]]
            np.testing.assert_array_equal(out.raw_scores[name][r], raw[name][r][cols])
        for grp in (pos, ~pos):                                            # self-normalised weights per label
            if grp.any():
                np.testing.assert_allclose(np.exp(out.log_weights[r][grp]).sum(), 1.0, rtol=1e-4)


def test_flatten_samples_matches_reference_golden():
    """`flatten_samples` (in_batch_negatives.py:10-52) against the vectors produced by the reference's own function
    (tests/golden/make_golden.py) - bit for bit, NaN positions included.  This batch, like every case of this file (at most
    8192 ids, 2 raw-score arrays), takes the one-launch `vodhip_flatten_inbatch`; tests/test_collate_limits_gpu.py runs
    the `vodhip_gather_by_id` path."""
    from vod_amd import types as vt
    from vod_amd.core.in_batch_negatives import flatten_samples
    from vod_amd.core.sample import PrioritySampledSections

    g = np.load(GOLDEN / "flatten_inbatch.npz")
    ps = PrioritySampledSections(
        batch=vt.RetrievalBatch(indices=g["idx"], scores=g["scr"], labels=g["lbl"]),
        log_weights=g["logw"], max_sampling_id=np.zeros(4), lse_pos=np.zeros(4), lse_neg=np.zeros(4),
        raw_scores={"dense": g["raw_dense"], "sparse": g["raw_sparse"]},
    )
    out = flatten_samples(ps, padding=True)
    np.testing.assert_array_equal(out.batch.indices, g["out_idx"])
    np.testing.assert_array_equal(out.batch.scores, g["out_scr"])
    np.testing.assert_array_equal(out.batch.labels, g["out_lbl"])
    assert out.batch.labels.dtype == np.bool_
    np.testing.assert_array_equal(out.log_weights, g["out_logw"])
    np.testing.assert_array_equal(out.raw_scores["dense"], g["out_raw_dense"])
    np.testing.assert_array_equal(out.raw_scores["sparse"], g["out_raw_sparse"])


@pytest.mark.parametrize("b,n,pool", [(64, 32, 3000), (7, 130, 200), (1, 1, 5), (16, 512, 100000)])
def test_flatten_samples_matches_oracle_random(b, n, pool):
    from oracle import sampling as osmp
    from vod_amd import types as vt
    from vod_amd.core.in_batch_negatives import flatten_samples
    from vod_amd.core.sample import PrioritySampledSections

    rng = np.random.default_rng(b * 1000 + n)
    idx = rng.integers(-1, pool, size=(b, n)).astype(np.int64)  # duplicates inside a row and -1 pads occur
    scr = rng.standard_normal((b, n)).astype(np.float32)
    scr[idx < 0] = -np.inf
    lbl = rng.random((b, n)) < 0.2
    logw = rng.standard_normal((b, n)).astype(np.float32)
    raw = {"dense": rng.standard_normal((b, n)).astype(np.float32), "sparse": np.where(rng.random((b, n)) < 0.3, np.nan, 1.0).astype(np.float32)}
    ps = PrioritySampledSections(batch=vt.RetrievalBatch(indices=idx, scores=scr, labels=lbl), log_weights=logw,
                                 max_sampling_id=np.zeros(b), lse_pos=np.zeros(b), lse_neg=np.zeros(b), raw_scores=raw)
    for padding in (True, False):
        out = flatten_samples(ps, padding=padding)
        ref = osmp.flatten_samples(idx, scr, lbl, logw, raw, padding=padding)
        np.testing.assert_array_equal(out.batch.indices, ref["indices"])
        np.testing.assert_array_equal(out.batch.scores, ref["scores"])
        np.testing.assert_array_equal(out.batch.labels, ref["labels"])
        np.testing.assert_array_equal(out.log_weights, ref["log_weights"])
        for key in raw:
            np.testing.assert_array_equal(out.raw_scores[key], ref["raw"][key])
