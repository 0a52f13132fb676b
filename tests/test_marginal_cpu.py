"""The marginal-likelihood objective without a GPU: the float64 restatement (tests/marginal_ref.py) against what the reference computed
(tests/golden/marginal_likelihood.npz), and the new entry points in the header and the ctypes table."""
import json
import pathlib
import re

import numpy as np
import pytest

import marginal_ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
OUTPUTS = ("loss", "retriever_scores", "dq", "ds", "dlogits")
E_REF_CEILING = 1e-5  # also asserted by tests/golden/make_golden_marginal.py when it writes the fixture
NEW_SYMBOLS = {"vodhip_lm_token_logprob_forward": 11, "vodhip_marginal_forward": 19, "vodhip_lm_token_logprob_backward": 13}


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = np.load(golden_dir / "marginal_likelihood.npz")
    return z, json.loads(str(z["params_json"]))


def load_case(z, name):
    inp = {k: z[f"{name}__{k}"] for k in ("q", "s", "score", "logits", "ids", "mask")}
    inp["ids"] = inp["ids"].astype(np.int64)
    return inp


def test_fixture_holds_the_cases_and_only_data(fixture, golden_dir):
    z, params = fixture
    assert (golden_dir / "marginal_likelihood.npz").stat().st_size < 1_000_000
    shapes = {tuple(v[:5]): v[5] for v in params["cases"].values()}
    for shape in ((1, 1, 2, 7, 8), (3, 5, 17, 264, 8)):
        assert {v[5] for v in params["cases"].values() if tuple(v[:5]) == shape} == {True, False}, shape
    assert shapes[(4, 70, 3, 40, 520)] is False
    assert (2, 2, 3, 2049, 8) in shapes and (2, 2, 3, 4104, 8) in shapes
    for key in z.files:
        assert z[key].dtype.kind in "fiuU", (key, z[key].dtype)  # numbers and the parameter string: no pickled objects
    mid = load_case(z, "mid_3d")
    assert np.isinf(mid["score"]).any() and (np.isfinite(mid["score"]).sum(axis=1) == 1).any()   # a padded section, a one-section row
    assert np.isinf(mid["logits"]).any() and np.abs(mid["logits"][np.isfinite(mid["logits"])]).max() >= 1e4
    tgt_logit = np.take_along_axis(mid["logits"][:, :, :-1], mid["ids"][:, :, 1:, None], axis=-1)[..., 0]
    assert np.isinf(tgt_logit[mid["mask"][:, :, 1:] != 0]).any()                                   # -inf on a live target
    m = mid["mask"].astype(np.int64)
    assert ((np.diff(m, axis=-1) == 1).any(axis=-1)).any()                                           # a hole: 0 followed by 1


@pytest.mark.parametrize("name", ["tiny_3d", "tiny_2d", "mid_3d", "mid_2d", "wide_2d", "oddv_3d", "tailv_2d"])
def test_restatement_meets_the_reference(fixture, name):
    z, params = fixture
    inp = load_case(z, name)
    want = marginal_ref.marginal(inp["q"], inp["s"], inp["score"], inp["logits"], inp["ids"], inp["mask"])
    for key in OUTPUTS:
        ref = z[f"{name}__ref_{key}"]
        assert ref.dtype == np.float32
        err = marginal_ref.scaled_error(ref, want[key])
        # the stored unit itself is bounded: a float32 pipeline of these sizes stays below 1e-5 of a correct float64 evaluation, and a
        # wrong restatement (a shifted target, a dropped mask) is off by 1e-3 or more - it must not loosen the gates built on e_ref
        assert params["e_ref"][name][key] <= E_REF_CEILING and err <= E_REF_CEILING, (name, key, err)
        gate = 4 * params["e_ref"][name][key]
        assert err <= gate, (name, key, err, gate)
    live = inp["mask"][..., 1:] != 0
    assert np.all(want["dlogits"][..., -1, :] == 0) and np.all(want["dlogits"][..., :-1, :][~live] == 0)


def test_restatement_corner_rules():
    rng = np.random.default_rng(7)
    B, D, L, V, H = 2, 3, 4, 9, 4
    q, s = rng.normal(size=(B, H)), rng.normal(size=(B, D, H))
    score, logits = np.zeros((B, D)), rng.normal(size=(B, D, L, V))
    ids, mask = rng.integers(0, V - 1, size=(B, D, L)), np.ones((B, D, L), dtype=np.int64)
    base = marginal_ref.marginal(q, s, score, logits, ids, mask)
    assert np.isfinite(base["loss"])
    mask2 = mask.copy()
    mask2[0, 1, 2] = 0
    for bad in (-100, V + 5):  # ids at masked positions are not looked at
        ids2 = ids.copy()
        ids2[0, 1, 2] = bad
        ids0 = ids.copy()
        ids0[0, 1, 2] = 0
        a, b = marginal_ref.marginal(q, s, score, logits, ids2, mask2), marginal_ref.marginal(q, s, score, logits, ids0, mask2)
        assert all(np.array_equal(a[k], b[k]) for k in a)
    for bad in (V - 1, -1, V + 5):  # a live one: NaN loss, finite scores
        ids2 = ids.copy()
        ids2[1, 0, 3] = bad
        out = marginal_ref.marginal(q, s, score, logits, ids2, mask)
        assert np.isnan(out["loss"]) and np.isfinite(out["retriever_scores"]).all()
    mask3 = mask.copy()
    mask3[1, 2, 1:] = 0  # n = 0
    assert np.isnan(marginal_ref.marginal(q, s, score, logits, ids, mask3)["loss"])
    with pytest.raises(ValueError):
        marginal_ref.marginal(q, s, score, logits[:, :, :1], ids[:, :, :1], mask[:, :, :1])


def test_header_declares_the_entry_points_and_signatures_carry_them():
    from vod_amd import _native

    header = (ROOT / "include" / "vodhip.h").read_text()
    for name, n_args in NEW_SYMBOLS.items():
        assert re.search(rf"\bint {name}\s*\(", header), name
        res, args = _native.SIGNATURES[name]
        assert len(args) == n_args, name
    from vod_amd import gradients

    assert hasattr(gradients, "MarginalLikelihoodGradients")
