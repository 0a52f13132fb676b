"""GPU tests of the sampler's proposal (include/vodhip.h H7: `vodhip_priority_sample_proposal`, `vodhip_priority_sample_merged_proposal`,
`vodhip_collate_proposal`): log_p of every sample, the log-mass of each stratum and the joint weights, from the launches that sample.

  1. bit compatibility: what the old entry points write is what the new ones write, with the new pointers set and with all of them NULL
  2. values against the float64 restatement (tests/proposal_ref.py).  Samples and labels are exact; every float output sits within
     GATE = max(4 * e32, 32 * 2^-24) of it, e32 = the restatement's own float32 evaluation against float64 and the floor the 32 float32
     ulps of a tree reduction plus exp / log (the scheme of tests/test_vod_gpu.py), as max |got - want| / max(1, max |want|); non-finite
     positions must match exactly.  Each case prints `PROPERR <case> <output> err=... gate=...` before it asserts (run with `-s`)
  3. flattening: the two proposal arrays fill with -inf, the reference's arrays still with NaN; more than 8 value arrays are refused
  4. end to end on the device: collate -> to_dict(weights=...) -> VodGradients(alpha=0) is MarginalLikelihoodGradients under full
     enumeration, for both feeding modes, 3-D sections and the flattened batch (fed as it comes: no nan_to_num_)
  5. / 6. two runs, and a captured replay, give the same bits.
nq <= 8 everywhere.
"""
import ctypes
import functools

import numpy as np
import pytest

import marginal_ref
import proposal_ref

torch = pytest.importorskip("torch")
import vod_ref  # noqa: E402

pytestmark = pytest.mark.gpu
FLOOR = 32 * 2.0 ** -24
FLOATS = ("log_weights", "lse", "log_p", "log_mass", "joint")
NEW_POINTERS = ("out_log_proposal", "out_log_mass_pos", "out_log_mass_neg", "out_joint_log_weights", "flat_log_proposal",
                "flat_joint_log_weights")


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")  # (a copy: the shared inputs are read-only)


def _same_bytes(a, b):
    """Bitwise equality: NaN-safe, and +0.0 is not -0.0."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def _sample(scores, labels, noise, k_pos, k_tot, *, temperature=1.0, max_support=-1, keep_top=False, entry="proposal", normalized=True,
            check=True):
    """One launch of `vodhip_priority_sample` (entry="old") or `vodhip_priority_sample_proposal` ("proposal": every new pointer set;
    "null": all NULL).  Returns a dict of device tensors; the new outputs are pre-filled with 7 so that an unwritten slot shows."""
    from vod_amd import _native

    lib = _native.load_library()
    sc, lb, nz = _t(np.asarray(scores, np.float32)), _t((np.asarray(labels) > 0).astype(np.uint8)), _t(np.asarray(noise, np.float32))
    nq, width = sc.shape
    out = {"samples": torch.full((nq, k_tot), -7, dtype=torch.int64, device="cuda"), "log_weights": torch.full((nq, k_tot), 7.0, device="cuda"),
           "labels": torch.full((nq, k_tot), 7, dtype=torch.uint8, device="cuda"), "lse": torch.full((nq, 2), 7.0, device="cuda"),
           "log_p": torch.full((nq, k_tot), 7.0, device="cuda"), "log_mass": torch.full((nq, 2), 7.0, device="cuda"),
           "joint": torch.full((nq, k_tot), 7.0, device="cuda")}
    args = [sc.data_ptr(), lb.data_ptr(), nz.data_ptr(), nq, width, int(k_pos), int(k_tot), float(temperature), int(max_support),
            int(bool(normalized)) | (2 if keep_top else 0), out["samples"].data_ptr(), out["log_weights"].data_ptr(), out["labels"].data_ptr(),
            out["lse"].data_ptr()]
    stream = _native.current_stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    if entry == "old":
        status = lib.vodhip_priority_sample(*args, stream)
    else:
        new = [out[k].data_ptr() if entry == "proposal" else None for k in ("log_p", "log_mass", "joint")]
        status = lib.vodhip_priority_sample_proposal(*args, *new, stream)
    if check:
        _native.check(status)
    out["status"] = status
    return out


def _compare(tag, got, scores, labels, noise, k_pos, k_tot, **kw):
    want = proposal_ref.sample(scores, labels, noise, k_pos, k_tot, **kw)
    w32 = proposal_ref.sample(scores, labels, noise, k_pos, k_tot, dtype=np.float32, **kw)
    np.testing.assert_array_equal(got["samples"], want["samples"], err_msg=tag)
    np.testing.assert_array_equal(got["labels"] != 0, want["labels"], err_msg=tag)
    pad = want["samples"] < 0
    assert np.isneginf(got["log_p"][pad]).all() and np.isneginf(got["joint"][pad]).all() and np.isneginf(got["log_weights"][pad]).all(), tag
    assert not np.isnan(got["joint"]).any(), tag
    failures = []
    for key in FLOATS:
        e32 = proposal_ref.scaled_error(w32[key], want[key])
        gate = max(4 * e32, FLOOR)
        e = proposal_ref.scaled_error(got[key], want[key])  # (asserts that the non-finite positions match)
        print(f"PROPERR {tag} {key} err={e:.3e} gate={gate:.3e}")
        if not e <= gate:
            failures.append(f"{key}: {e:.3e} > {gate:.3e}")
    assert not failures, f"{tag}: " + "; ".join(failures)
    return want


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items() if k != "status"}


@functools.lru_cache(maxsize=None)
def _rows(width, mode, p_inf=0.1, seed=0, nq=4):
    """Seeded rows, computed once and never modified.  `mode`: "mixed" (a handful of positives: the one-wave path; the rest negatives),
    "half", "nopos", "noneg"."""
    rng = np.random.default_rng(8000 + 13 * width + seed)
    scores = (rng.normal(size=(nq, width)) * 3).astype(np.float32)
    scores[rng.uniform(size=scores.shape) < p_inf] = -np.inf
    p_pos = {"mixed": 0.08, "half": 0.5, "nopos": 0.0, "noneg": 1.0}[mode]
    labels = rng.uniform(size=scores.shape) < p_pos
    if mode == "mixed" and width >= 2:
        labels[:, 0], labels[:, 1] = True, False  # both strata exist
    noise = rng.exponential(size=scores.shape).astype(np.float32)
    for a in (scores, labels, noise):
        a.setflags(write=False)
    return scores, labels, noise


# ---- 1. bit compatibility ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,mode,support", [(40, "mixed", -1), (65, "nopos", -1), (300, "half", 40), (1000, "mixed", -1)])
def test_sampling_writes_the_old_bits_with_the_new_pointers_set_and_null(width, mode, support):
    scores, labels, noise = _rows(width, mode)
    kw = dict(temperature=1.0, max_support=support)
    old = _sample(scores, labels, noise, 4, 32, entry="old", **kw)
    for entry in ("proposal", "null"):
        new = _sample(scores, labels, noise, 4, 32, entry=entry, **kw)
        for key in ("samples", "log_weights", "labels", "lse"):
            assert _same_bytes(old[key], new[key]), (entry, key)
        if entry == "null":  # nothing else was touched
            assert all(bool((new[k] == 7).all()) for k in ("log_p", "log_mass", "joint"))


def _collate_inputs(B, n_lookup, ks, pool, seed):
    rng = np.random.default_rng(seed)
    names = ["dense", "sparse", "extra"][: len(ks)]
    engines = {}
    for name, k in zip(names, ks):
        idx = np.stack([rng.choice(pool, size=k, replace=False) for _ in range(B)]).astype(np.int64) + 2  # (no id 1: the flattening pads with it)
        engines[name] = (_t(idx), _t((rng.normal(size=(B, k)) * 2).astype(np.float32)))
    l_idx = engines[names[0]][0][:, :n_lookup].clone()
    l_lbl = _t((rng.uniform(size=(B, n_lookup)) < 0.6).astype(np.int64))
    stride = n_lookup + sum(ks) + 1
    noise = _t(rng.exponential(size=(B, stride)).astype(np.float32))
    return l_idx, l_lbl, engines, {n: 1.0 for n in names}, noise


FIELDS = ("indices", "scores", "labels", "log_weights", "lse_pos", "lse_neg", "max_sampling_id")


def _fields(out):
    return {**{k: getattr(out, k) for k in FIELDS}, **{f"raw_{k}": v for k, v in out.raw_scores.items()},
            **({"local_ids": out.local_ids} if out.local_ids is not None else {"n_unique": out.n_unique})}


class _NullingLib:
    """libvodhip with `vodhip_collate_proposal` called with every new pointer NULL."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def vodhip_collate_proposal(self, ref, stream):
        for f in NEW_POINTERS:
            setattr(ref._obj, f, None)
        return self._lib.vodhip_collate_proposal(ref, stream)


@pytest.mark.parametrize("flat", [False, True])
def test_collate_writes_the_old_bits_with_the_new_pointers_set_and_null(flat, monkeypatch):
    from vod_amd import _native
    from vod_amd.core import collate

    l_idx, l_lbl, engines, weights, noise = _collate_inputs(8, 4, (40, 30), 200, 8101)
    kw = dict(total=16, max_pos_sections=4, temperature=1.0, in_batch_negatives=flat)
    old = _fields(collate.collate_on_device(l_idx, l_lbl, engines, weights, noise, **kw))
    new = collate.collate_on_device(l_idx, l_lbl, engines, weights, noise, proposal=True, **kw)
    assert new.log_proposal.shape == new.scores.shape == new.joint_log_weights.shape and new.log_mass.shape == (8, 2)
    for key, val in _fields(new).items():
        assert _same_bytes(old[key], val), key
    lib = _native.load_library()
    monkeypatch.setattr(collate._native, "load_library", lambda: _NullingLib(lib))
    null = _fields(collate.collate_on_device(l_idx, l_lbl, engines, weights, noise, proposal=True, **kw))
    for key, val in null.items():
        assert _same_bytes(old[key], val), ("null", key)


def test_staged_merge_then_sample_writes_the_old_bits():
    from vod_amd.core.collate import sample_merged_on_device
    from vod_amd.core.merge import merge_hybrid_device

    l_idx, l_lbl, engines, weights, noise = _collate_inputs(8, 4, (40, 30), 200, 8102)
    merged = merge_hybrid_device(l_idx, l_lbl, engines, weights)
    kw = dict(total=16, max_pos_sections=4, temperature=0.5)
    old, new = _fields(sample_merged_on_device(merged, noise, **kw)), sample_merged_on_device(merged, noise, proposal=True, **kw)
    for key, val in _fields(new).items():
        assert _same_bytes(old[key], val), key
    assert new.log_proposal is not None and new.log_mass.shape == (8, 2)


# ---- 2. values against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mixed", "nopos"])
@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 128, 256, 257, 1000])
def test_widths_and_sample_counts_match_the_restatement(width, mode):
    """A class of 64 against 65 members switches the one-wave path to the LDS path ("nopos": the negatives are the whole row); 256 / 257
    crosses the sort size.  k_total 1, 4, 32: beyond the width there are pads."""
    scores, labels, noise = _rows(width, mode)
    for k_tot in (1, 4, 32):
        k_pos = min(2, k_tot)
        got = _host(_sample(scores, labels, noise, k_pos, k_tot))
        want = _compare(f"w{width}-{mode}-k{k_tot}", got, scores, labels, noise, k_pos, k_tot)
        if mode == "nopos":
            assert np.isneginf(got["log_mass"][:, 0]).all() and np.isfinite(got["log_mass"][:, 1]).all()
        assert (want["samples"] < 0).any() == (k_tot > width)


@pytest.mark.parametrize("temperature", [0.5, 1.0, 0.0])
@pytest.mark.parametrize("width,mode", [(40, "half"), (300, "half"), (300, "mixed")])
def test_temperatures_match_the_restatement(width, mode, temperature):
    scores, labels, noise = _rows(width, mode, seed=1)
    got = _host(_sample(scores, labels, noise, 4, 16, temperature=temperature))
    _compare(f"w{width}-{mode}-T{temperature:g}", got, scores, labels, noise, 4, 16, temperature=temperature)


def test_a_stratum_that_runs_dry_grows_the_other_one():
    scores, labels, noise = _rows(40, "noneg", seed=2)     # no negatives: every sample is a positive
    got = _host(_sample(scores, labels, noise, 4, 16))
    _compare("noneg", got, scores, labels, noise, 4, 16)
    assert (got["labels"] != 0).all() and np.isneginf(got["log_mass"][:, 1]).all()
    scores, labels, noise = _rows(130, "half", p_inf=0.0, seed=3)
    scores = scores.copy()
    neg = np.flatnonzero(~labels[0])
    scores[:, neg[5:]] = -np.inf                           # 5 finite negatives in row 0: its k_positive grows from 4 to 27
    got = _host(_sample(scores, labels, noise, 4, 32))
    want = _compare("few-negatives", got, scores, labels, noise, 4, 32)
    assert want["labels"][0].sum() == 32 - 5


def test_strata_without_mass_nan_scores_and_empty_rows_of_samples():
    scores, labels, noise = (a.copy() for a in _rows(70, "mixed", seed=4))
    scores[0, labels[0]] = -np.inf                         # the positives of row 0 are all -inf: mass -inf, joint -inf, log_p NaN
    scores[1, ::7] = np.nan                                # NaN scores count as -inf
    scores[2, :] = -np.inf                                 # nothing has mass: both masses -inf, every joint weight -inf
    labels[3, :] = False
    got = _host(_sample(scores, labels, noise, 2, 8))
    _compare("massless", got, scores, labels, noise, 2, 8)
    assert np.isneginf(got["log_mass"][0, 0]) and np.isneginf(got["log_mass"][2]).all() and np.isneginf(got["joint"][2]).all()
    assert np.isneginf(got["joint"][0][got["labels"][0] != 0]).all()


@pytest.mark.parametrize("keep_top", [False, True])
@pytest.mark.parametrize("width,mode,support,k_tot", [(300, "half", 40, 32), (100, "half", 8, 4), (1000, "mixed", 100, 32)])
def test_truncated_support_sets_the_mass(width, mode, support, k_tot, keep_top):
    """`max_support_size` below the class size, both truncation modes (a class of <= 64 members that is truncated takes the LDS path):
    log_mass runs over the truncated support."""
    scores, labels, noise = _rows(width, mode, p_inf=0.0, seed=5)
    got = _host(_sample(scores, labels, noise, 2, k_tot, max_support=support, keep_top=keep_top))
    want = _compare(f"w{width}-support{support}-{'keep' if keep_top else 'ref'}", got, scores, labels, noise, 2, k_tot, max_support=support,
                    keep_top=keep_top)
    full = proposal_ref.sample(scores, labels, noise, 2, k_tot)
    cut = (~labels).sum(1) > support
    assert cut.all() and (want["log_mass"][:, 1] < full["log_mass"][:, 1] - 1e-4).all()


def test_joint_weights_need_the_normalized_bit():
    scores, labels, noise = _rows(40, "mixed")
    out = _sample(scores, labels, noise, 2, 8, normalized=False, check=False)
    assert out["status"] < 0 and bool((out["samples"] == -7).all())  # refused before anything was launched
    from vod_amd import _native

    assert b"normalized" in _native.load_library().vodhip_last_error()


def test_merged_rows_with_the_width_derived_on_the_device():
    from vod_amd.core.collate import collate_on_device
    from vod_amd.core.merge import merge_hybrid_device

    l_idx, l_lbl, engines, weights, noise = _collate_inputs(8, 4, (40, 30), 200, 8103)
    out = collate_on_device(l_idx, l_lbl, engines, weights, noise, total=16, max_pos_sections=4, temperature=0.5, proposal=True)
    m_idx, m_scr, m_lbl, _ = merge_hybrid_device(l_idx, l_lbl, engines, weights).cut()
    width = m_scr.shape[1]
    assert 40 < width < noise.shape[1]
    got = {"samples": out.local_ids, "labels": out.labels, "log_weights": out.log_weights, "lse": torch.stack([out.lse_pos, out.lse_neg], 1),
           "log_p": out.log_proposal, "log_mass": out.log_mass, "joint": out.joint_log_weights}
    _compare("merged", _host(got), m_scr.cpu().numpy(), m_lbl.cpu().numpy() > 0, noise.cpu().numpy()[:, :width], 4, 16, temperature=0.5)


# ---- 3. flattening ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n,ks,pool", [(4, 8, (12, 10), 30), (8, 32, (40, 30), 90)])
def test_flattened_proposal_fills_with_minus_infinity(B, n, ks, pool):
    from vod_amd.core.collate import collate_on_device

    l_idx, l_lbl, engines, weights, noise = _collate_inputs(B, 3, ks, pool, 8200 + B)
    kw = dict(total=n, max_pos_sections=2, proposal=True)
    rows = collate_on_device(l_idx, l_lbl, engines, weights, noise, **kw)
    flat = collate_on_device(l_idx, l_lbl, engines, weights, noise, in_batch_negatives=True, **kw)
    ids = rows.indices.cpu().numpy()
    U = B * n
    assert flat.log_proposal.shape == flat.joint_log_weights.shape == (B, U) and flat.log_mass.shape == (B, 2)
    assert _same_bytes(flat.log_mass, rows.log_mass)
    uq = flat.indices.cpu().numpy()
    missing = ~(uq[None, :, None] == ids[:, None, :]).any(-1)
    assert missing.any() and (~missing).any()
    # the gather is a copy: exactly the sampled rows' values, by first occurrence
    for name in ("log_proposal", "joint_log_weights"):
        want_ids, want = proposal_ref.flatten(ids, getattr(rows, name).cpu().numpy())
        np.testing.assert_array_equal(uq, want_ids)
        got = getattr(flat, name).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=name)
        assert np.isneginf(got[missing]).all() and not np.isnan(got).any(), name
    # ... and the sampled rows' values are the restatement's
    merged_out = {"samples": rows.local_ids, "labels": rows.labels, "log_weights": rows.log_weights,
                  "lse": torch.stack([rows.lse_pos, rows.lse_neg], 1), "log_p": rows.log_proposal, "log_mass": rows.log_mass,
                  "joint": rows.joint_log_weights}
    from vod_amd.core.merge import merge_hybrid_device

    _, m_scr, m_lbl, _ = merge_hybrid_device(l_idx, l_lbl, engines, weights).cut()
    width = m_scr.shape[1]
    _compare(f"flat-{B}x{n}", _host(merged_out), m_scr.cpu().numpy(), m_lbl.cpu().numpy() > 0, noise.cpu().numpy()[:, :width], 2, n)
    # the reference's arrays keep their NaN
    for arr in (flat.scores, flat.log_weights, *flat.raw_scores.values()):
        assert np.isnan(arr.cpu().numpy()[missing]).all()
    assert not flat.labels.cpu().numpy()[missing].any()


def test_more_than_eight_value_arrays_are_refused():
    from vod_amd import _native
    from vod_amd.core.collate import DeviceSampledSections, flatten_on_device

    lib = _native.load_library()
    B, n = 4, 8
    ids = torch.arange(B * n, device="cuda").reshape(B, n)
    vals = [torch.zeros((B, n), device="cuda") for _ in range(9)]
    outs = [torch.full((B, B * n), 7.0, device="cuda") for _ in range(9)]
    uq = torch.full((B * n,), -7, dtype=torch.int64, device="cuda")
    ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    status = lib.vodhip_flatten_inbatch(ids.data_ptr(), B, n, 9, ptrs(vals), (ctypes.c_float * 9)(*[0.0] * 9), ptrs(outs), None, None,
                                        uq.data_ptr(), None, _native.current_stream_ptr(torch.device("cuda", torch.cuda.current_device())))
    assert status < 0 and bool((uq == -7).all()) and all(bool((o == 7).all()) for o in outs)
    z = torch.zeros((B, n), device="cuda")
    s = DeviceSampledSections(indices=ids, scores=z, labels=z > 0, log_weights=z, lse_pos=z[:, 0], lse_neg=z[:, 0], max_sampling_id=z[:, 0],
                              raw_scores={f"e{i}": z for i in range(5)}, log_proposal=z, log_mass=z[:, :2], joint_log_weights=z)
    with pytest.raises(ValueError, match="at most 8"):
        flatten_on_device(s, proposal=True)  # 2 + 5 + 2 = 9
    assert flatten_on_device(s).scores.shape == (B, B * n)  # 7 without the proposal: as before


# ---- 4. end to end on the device -----------------------------------------------------------------------------------------------------
E2E = dict(B=4, D=8, H=64, L=8, V=96)


@functools.lru_cache(maxsize=None)
def _e2e_inputs():
    """4 rows over the same 7 sections (merged width 8 with the merge's pad column = k_total = D: full enumeration), 2 lookup hits each."""
    B, D, H, L, V = (E2E[k] for k in "BDHLV")
    rng = np.random.default_rng(8300)
    e_idx = np.stack([rng.permutation(np.arange(10, 17)) for _ in range(B)]).astype(np.int64)
    e_scr = (rng.normal(size=(B, 7)) * 2).astype(np.float32)
    l_idx = e_idx[:, [2, 5]].copy()
    l_lbl = np.array([[1, 1], [1, 0], [1, 1], [0, 1]], np.int64)
    noise = rng.exponential(size=(B, 2 + 7 + 1)).astype(np.float32)
    mask = (rng.random(size=(B, B * D, L)) >= 0.25).astype(np.int64)
    mask[..., :2] = 1
    lm = {"q": (rng.normal(size=(B, H)) * 2 * H ** -0.5).astype(np.float32), "s3": rng.normal(size=(B, D, H)).astype(np.float32),
          "s2": rng.normal(size=(B * D, H)).astype(np.float32), "logits": (rng.normal(size=(B, B * D, L, V)) * 2).astype(np.float32),
          "ids": rng.integers(0, V - 1, size=(B, B * D, L)).astype(np.int64), "mask": mask}
    return l_idx, l_lbl, e_idx, e_scr, noise, lm


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("mode", ["stratum", "joint"])
def test_collate_feeds_the_objective_exactly(mode, flat):
    from vod_amd.core.collate import collate_on_device
    from vod_amd.gradients import MarginalLikelihoodGradients, VodGradients

    B, D, H, L, V = (E2E[k] for k in "BDHLV")
    l_idx, l_lbl, e_idx, e_scr, noise, lm = _e2e_inputs()
    out = collate_on_device(_t(l_idx), _t(l_lbl), {"dense": (_t(e_idx), _t(e_scr))}, {"dense": 1.0}, _t(noise), total=D, temperature=1.0,
                            in_batch_negatives=flat, proposal=True)
    n_sec = B * D if flat else D
    batch = out.to_dict("section__", weights=mode)  # as it comes: no nan_to_num_ in between
    assert ("section__log_proposal" in batch) == (mode == "stratum") and batch["section__log_weight"].shape == (B, n_sec)
    if flat:
        assert int(out.n_unique.item()) == 8 and bool(torch.isnan(batch["section__score"]).any())
    else:
        assert bool((out.local_ids >= 0).all())  # every candidate of every row, the merge's pad column included
    sec = lm["s2"] if flat else lm["s3"]
    logits, ids, mask = lm["logits"][:, :n_sec], lm["ids"][:, :n_sec], lm["mask"][:, :n_sec]
    batch["lm__input_ids"], batch["lm__attention_mask"] = _t(ids), _t(mask)

    def run(gradients, b):
        q, s, lg = (_t(x).requires_grad_() for x in (lm["q"], sec, logits))
        o = gradients(batch=b, query_encoding=q, section_encoding=s, lm_logits=lg)
        o.loss.backward()
        return {"loss": o.loss.detach(), "retriever_scores": o.retriever_scores, "dq": q.grad, "ds": s.grad, "dlogits": lg.grad}

    got = {k: v.double().cpu().numpy() for k, v in run(VodGradients(alpha=0.0, temperature=1.0), batch).items()}
    # the marginal likelihood of the same tensors.  It knows one way to leave a section out, a score of -inf, so the sections a row did
    # not sample (NaN in the flattened scores) are marked so for IT; VodGradients above got the scores as the collate wrote them.
    score = batch["section__score"]
    ml_batch = {"section__score": torch.where(torch.isnan(score), torch.full_like(score, float("-inf")), score),
                "lm__input_ids": batch["lm__input_ids"], "lm__attention_mask": batch["lm__attention_mask"]}
    ml = {k: v.double().cpu().numpy() for k, v in run(MarginalLikelihoodGradients(), ml_batch).items()}
    # the gate of tests/test_vod_gpu.py: max(4 * e32, 32 * 2^-24), e32 from the float32 restatement of the objective on these tensors
    host = lambda k: batch[k].cpu().numpy()  # noqa: E731
    args = (lm["q"], sec, host("section__score"), host("section__log_weight"), logits, ids, mask)
    kw = {"alpha": 0.0, "temperature": 1.0, "log_proposal": host("section__log_proposal") if mode == "stratum" else None}
    w64, w32 = vod_ref.vod(*args, **kw), vod_ref.vod(*args, dtype=torch.float32, **kw)
    live = np.isfinite(ml["retriever_scores"])
    assert live.sum() == B * 7  # 7 sections per row; the pad column and what a row did not sample take no part
    for key in ("loss", "retriever_scores", "dq", "ds", "dlogits"):
        g, m = got[key], ml[key]
        if key == "retriever_scores":  # (VodGradients reports the inner product where the score is NaN, the marginal -inf: compare the live ones)
            g, m = g[live], m[live]
        gate = max(4 * marginal_ref.scaled_error(w32[key], w64[key]), FLOOR)
        e = marginal_ref.scaled_error(g, m)
        print(f"PROPERR e2e-{mode}-{'flat' if flat else '3d'} {key} err={e:.3e} gate={gate:.3e}")
        assert e <= gate, key
    assert np.isfinite(got["loss"])


# ---- 5. / 6. run to run, and captured -------------------------------------------------------------------------------------------------
def _all_fields(out):
    return {**_fields(out), "log_proposal": out.log_proposal, "log_mass": out.log_mass, "joint_log_weights": out.joint_log_weights}


@pytest.mark.parametrize("flat", [False, True])
def test_two_runs_give_the_same_bits(flat):
    from vod_amd.core.collate import collate_on_device

    l_idx, l_lbl, engines, weights, noise = _collate_inputs(8, 4, (40, 30), 200, 8401)
    kw = dict(total=16, max_pos_sections=4, in_batch_negatives=flat, proposal=True)
    a = _all_fields(collate_on_device(l_idx, l_lbl, engines, weights, noise, **kw))
    b = _all_fields(collate_on_device(l_idx, l_lbl, engines, weights, noise, **kw))
    for key in a:
        assert _same_bytes(a[key], b[key]), key


def test_collate_proposal_captures_and_replays_to_the_same_bits():
    from vod_amd.core.collate import collate_on_device

    l_idx, l_lbl, engines, weights, noise = _collate_inputs(8, 4, (40, 30), 200, 8402)
    kw = dict(total=16, max_pos_sections=4, in_batch_negatives=True, proposal=True)
    step = lambda: collate_on_device(l_idx, l_lbl, engines, weights, noise, **kw)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            eager = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in _all_fields(eager).items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one chain on one stream: merge -> sample -> flatten, no parallel branch
        out = step()
    got = _all_fields(out)
    for v in got.values():  # the replay must recompute everything
        v.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    for key in eager:
        assert _same_bytes(got[key], eager[key]), key
