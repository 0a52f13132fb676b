"""The Renyi VOD objective without a GPU: the float64 restatement (tests/vod_ref.py) against the identities that pin it without a
reference - with exact weights it IS the marginal likelihood (tests/marginal_ref.py), it is non-decreasing in alpha, its closed-form
gradients are what autograd gives, it is continuous at alpha -> 1 - and the new entry point in the header and the ctypes table."""
import pathlib
import re

import numpy as np
import pytest

import marginal_ref

torch = pytest.importorskip("torch")
import vod_ref  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent
ALPHAS = (0.0, 0.25, 0.5, 0.75, 1 - 1e-4, 1.0)


def make(seed, B=4, D=9, H=6, L=5, V=13, three_d=True, excluded=True):
    """Random inputs with a padded section in rows 0 and 2, 25 % masked tokens and (with `excluded`) a section of finite score and
    log-weight -inf in rows 1 and 2."""
    rng = np.random.default_rng(seed)
    inp = {"q": rng.normal(size=(B, H)), "s": rng.normal(size=(B, D, H) if three_d else (D, H)),
           "score": rng.normal(size=(B, D)) * 2, "logw": rng.normal(size=(B, D)) * 1.5, "logits": rng.normal(size=(B, D, L, V)) * 2,
           "ids": rng.integers(0, V - 1, size=(B, D, L)), "mask": (rng.random(size=(B, D, L)) >= 0.25).astype(np.int64)}
    inp["mask"][..., 1] = 1  # every section keeps a live position
    inp["score"][0, D - 1] = inp["score"][2, 0] = -np.inf
    inp["logw"][0, D - 1] = inp["logw"][2, 0] = -np.inf  # what the sampler leaves at a padded section
    if excluded:
        inp["logw"][1, 3 % D] = inp["logw"][2, D - 1] = -np.inf
    return inp


def run(inp, **kw):
    return vod_ref.vod(inp["q"], inp["s"], inp["score"], inp["logw"], inp["logits"], inp["ids"], inp["mask"], **kw)


@pytest.mark.parametrize("three_d", [True, False])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_exact_weights_recover_the_marginal_likelihood(three_d, temperature):
    inp = make(11, three_d=three_d, excluded=False)
    pad = np.isinf(inp["score"])
    c = temperature * np.where(pad, 0.0, inp["score"])
    z = np.where(pad, -np.inf, c)
    inp["logw"] = z - np.log(np.exp(z).sum(-1, keepdims=True))  # log_softmax over the live set, in float64
    got = run(inp, alpha=0.0, temperature=temperature, token_reduction="mean")
    want = marginal_ref.marginal(inp["q"], inp["s"], inp["score"], inp["logits"], inp["ids"], inp["mask"])
    for key in ("loss", "retriever_scores", "dq", "ds", "dlogits"):
        assert marginal_ref.scaled_error(got[key], want[key]) <= 1e-12, key
    assert abs(got["iw_bound"] + got["loss"]) <= 1e-12


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_loss_is_non_decreasing_in_alpha(reduction):
    inp = make(12)
    losses = [float(run(inp, alpha=a, token_reduction=reduction)["loss"]) for a in ALPHAS]
    assert all(np.isfinite(losses))
    assert all(b >= a - 1e-12 for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] > losses[0] + 1e-3  # (and not by being constant)
    out = run(inp, alpha=0.5, token_reduction=reduction)
    assert out["elbo"] <= -out["loss"] + 1e-12 <= out["iw_bound"] + 2e-12
    assert 1.0 <= out["ess"] <= inp["score"].shape[1]


@pytest.mark.parametrize("three_d", [True, False])
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_closed_form_gradients_are_what_autograd_gives(alpha, reduction, three_d):
    """dq / ds from d_scores = -(omega - pi) / B and dlogits from coef = -omega / (B n), against float64 autograd."""
    inp = make(13, three_d=three_d)
    out = run(inp, alpha=alpha, token_reduction=reduction, grad_out=1.5)
    q, s, dr = inp["q"], inp["s"], out["d_scores"]
    if three_d:
        dq, ds = np.einsum("bd,bdh->bh", dr, s), dr[..., None] * q[:, None, :]
    else:
        dq, ds = dr @ s, dr.T @ q
    x = inp["logits"][..., :-1, :]
    soft = np.exp(x - x.max(-1, keepdims=True))
    soft /= soft.sum(-1, keepdims=True)
    onehot = np.zeros_like(soft)
    np.put_along_axis(onehot, inp["ids"][..., 1:, None], 1.0, axis=-1)
    g = out["coef"][..., None, None] * (onehot - soft) * (inp["mask"][..., 1:, None] != 0)
    dlogits = np.zeros_like(inp["logits"])
    dlogits[..., :-1, :] = g
    for key, mine in (("dq", dq), ("ds", ds), ("dlogits", dlogits)):
        assert marginal_ref.scaled_error(mine, out[key]) <= 1e-13, key
    dead = np.isinf(inp["logw"])
    assert np.all(out["d_scores"][dead] == 0) and np.all(out["coef"][dead] == 0) and np.all(out["dlogits"][dead] == 0)


def test_bound_is_continuous_as_alpha_reaches_one():
    """|Lhat(1 - 1e-4) - Lhat(1)| within twice the first-order term 1e-4 * Var(lw) / 2 (variance under the normalised weights)."""
    inp = make(14)
    near, at = run(inp, alpha=1 - 1e-4), run(inp, alpha=1.0)
    w = np.where(np.isfinite(at["ls"]), np.exp(at["ls"]), 0.0)
    lw = np.where(np.isfinite(at["lw"]), at["lw"], 0.0)
    mean = (w * lw).sum(-1)
    var = (w * (lw - mean[:, None]) ** 2).sum(-1)
    assert np.all(var > 0)
    assert np.all(np.abs(near["Lhat"] - at["Lhat"]) <= 2 * 1e-4 * var / 2)
    assert np.all(near["Lhat"] >= at["Lhat"])
    np.testing.assert_allclose(at["Lhat"], mean, rtol=1e-13)


def test_corner_rules():
    inp = make(15)
    base = run(inp, alpha=0.5)
    assert np.isfinite(base["loss"])
    # an excluded section with a finite score keeps its retriever score, gets no gradient, and its tokens and ids are not looked at
    assert np.isfinite(inp["score"][1, 3]) and np.isinf(inp["logw"][1, 3]) and np.isfinite(base["retriever_scores"][1, 3])
    assert base["d_scores"][1, 3] == 0 and base["coef"][1, 3] == 0 and np.all(base["ds"][1, 3] == 0) and np.all(base["dlogits"][1, 3] == 0)
    other = {k: v.copy() for k, v in inp.items()}
    other["ids"][1, 3, 1:] = -7
    other["mask"][1, 3, 1:] = 0
    other["logits"][1, 3] = 5.0
    got = run(other, alpha=0.5)
    assert all(np.array_equal(got[k], base[k], equal_nan=True) for k in ("loss", "dq", "ds", "dlogits", "iw_bound", "elbo", "ess"))
    assert np.array_equal(np.isinf(base["retriever_scores"]), np.isinf(inp["score"]))
    # the same holds when the proposal, not the weight, is -inf
    prop = np.where(np.isinf(inp["score"]), 0.0, inp["score"])
    prop[3, 4] = -np.inf
    got = run(inp, alpha=0.5, log_proposal=prop)
    assert np.isfinite(got["loss"]) and got["d_scores"][3, 4] == 0 and got["coef"][3, 4] == 0
    # an empty live set: NaN loss, the other rows' gradients stay finite
    empty = {k: v.copy() for k, v in inp.items()}
    empty["logw"][3] = -np.inf
    got = run(empty, alpha=0.5)
    assert np.isnan(got["loss"]) and np.isnan(got["Lhat"][3]) and np.isfinite(got["Lhat"][:3]).all() and np.isfinite(got["dq"][:3]).all()
    # a NaN weight or proposal of a section that is not padded: NaN; of a padded one: not looked at
    for key in ("logw", "score"):
        bad = {k: v.copy() for k, v in inp.items()}
        bad[key][1, 5] = np.nan
        assert np.isnan(run(bad, alpha=0.5)["loss"]), key
    bad = {k: v.copy() for k, v in inp.items()}
    bad["logw"][0, -1] = np.nan
    assert run(bad, alpha=0.5)["loss"] == base["loss"]
    assert np.isfinite(run(inp, alpha=0.5, temperature=0.0)["loss"])  # no 0 * -inf from a padded score
    # n = 0 on a live section: NaN in both reductions; a live target outside [0, V-2] as well
    for reduction in ("mean", "sum"):
        none = {k: v.copy() for k, v in inp.items()}
        none["mask"][1, 5, 1:] = 0
        assert np.isnan(run(none, alpha=0.5, token_reduction=reduction)["loss"])
    V = inp["logits"].shape[-1]
    for bad_id in (V - 1, -1, V + 5):
        bad = {k: v.copy() for k, v in inp.items()}
        bad["ids"][1, 5, 1], bad["mask"][1, 5, 1] = bad_id, 1
        out = run(bad, alpha=0.5)
        assert np.isnan(out["loss"]) and np.isfinite(out["retriever_scores"][1]).all()


def test_float32_evaluation_is_close_to_float64():
    """The float32 evaluation that sets the GPU tests' tolerance is the same function: 1e-5 apart at most, alpha -> 1 included."""
    inp = make(16)
    for alpha in (0.0, 1 - 1e-4, 1.0):
        a, b = run(inp, alpha=alpha), run(inp, alpha=alpha, dtype=torch.float32)
        for key in ("loss", "dq", "ds", "dlogits", "iw_bound", "elbo", "ess"):
            assert marginal_ref.scaled_error(b[key], a[key]) <= 1e-5, (alpha, key)


def test_header_declares_the_entry_point_and_the_signature_carries_it():
    from vod_amd import _native, gradients

    header = (ROOT / "include" / "vodhip.h").read_text()
    assert re.search(r"\bint vodhip_vod_forward\s*\(", header)
    decl = header[header.index("int vodhip_vod_forward"):]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    res, args = _native.SIGNATURES["vodhip_vod_forward"]
    assert len(args) == 25 == decl.count(",") + 1
    assert hasattr(gradients, "VodGradients")
    g = gradients.VodGradients()
    assert (g.alpha, g.temperature, g.token_reduction) == (0.0, 1.0, "mean")
    with pytest.raises(ValueError):
        gradients.VodGradients(token_reduction="max")
