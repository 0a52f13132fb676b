"""The sampler's proposal without a GPU: the new entry points in the library, the header and the ctypes table; the float64 restatement
(tests/proposal_ref.py) against the reference's own numbers (tests/golden/proposal.npz) and against the identities that pin what the
feature is for - under full enumeration the joint weights ARE log_softmax(score) and both ways of feeding the VOD objective
(tests/vod_ref.py) give the marginal likelihood (tests/marginal_ref.py), which the per-stratum weights alone do not."""
import ctypes
import json
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import marginal_ref
import proposal_ref

torch = pytest.importorskip("torch")
import vod_ref  # noqa: E402

ROOT = pathlib.Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
NEW_SYMBOLS = {"vodhip_priority_sample_proposal": 18, "vodhip_priority_sample_merged_proposal": 32, "vodhip_collate_proposal": 2}
NEW_POINTERS = ("out_log_proposal", "out_log_mass_pos", "out_log_mass_neg", "out_joint_log_weights", "flat_log_proposal",
                "flat_joint_log_weights")


# ---- 1. the C-ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_header_declares_them():
    from vod_amd import _native

    lib = _native.load_library()  # raises when a symbol of the table is missing
    header = (ROOT / "include" / "vodhip.h").read_text()
    for name, n_args in NEW_SYMBOLS.items():
        assert hasattr(lib, name), name
        assert re.search(rf"\bint {name}\s*\(", header), name
        decl = header[header.index(f"int {name}"):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        res, args = _native.SIGNATURES[name]
        assert len(args) == n_args == decl.count(",") + 1, name
    assert "Replaces:" in header[header.index("emitting the sampler's PROPOSAL"):header.index("int vodhip_priority_sample_proposal")]


def test_header_is_c99_and_the_new_struct_extends_the_old_one(tmp_path):
    from vod_amd import _native

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", str(ROOT / "include" / "vodhip.h")], check=True)
    prog = tmp_path / "layout.c"
    prog.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "vodhip.h"\nint main(void) {\n'
        '  printf("%zu %zu %zu %zu\\n", offsetof(vodhip_collate_proposal_args_t, base), sizeof(vodhip_collate_proposal_args_t),\n'
        '         sizeof(vodhip_collate_args_t), sizeof(float*));\n'
        + "".join(f'  printf("%zu\\n", offsetof(vodhip_collate_proposal_args_t, {f}));\n' for f in NEW_POINTERS)
        + "  return 0;\n}\n"
    )
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", str(prog), "-I", str(ROOT / "include"), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    off_base, size_new, size_old, size_ptr = got[:4]
    assert off_base == 0
    assert size_new >= size_old + 6 * size_ptr
    assert size_old == ctypes.sizeof(_native.CollateArgs) and size_new == ctypes.sizeof(_native.CollateProposalArgs)
    assert _native.CollateProposalArgs.base.offset == 0
    assert got[4:] == [getattr(_native.CollateProposalArgs, f).offset for f in NEW_POINTERS]


# ---- 2. the restatement against the reference's numbers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN / "proposal.npz")
    return g, json.loads(str(g["params_json"]))


def _against_fixture(tag, g, prefix, want, e_ref):
    np.testing.assert_array_equal(g[f"{prefix}__out_samples"], want["samples"])
    np.testing.assert_array_equal(g[f"{prefix}__out_labels"], want["labels"])
    for key, unit in e_ref.items():
        e = proposal_ref.scaled_error(g[f"{prefix}__out_{key}"], want[key])
        print(f"PROPERR {tag} {key} err={e:.3e} gate={4 * unit:.3e}")
        assert e <= 4 * unit, (tag, key, e)


def test_restatement_agrees_with_the_reference_fixture(golden):
    g, params = golden
    assert 20 <= len(params["labeled"]) + len(params["single"]) <= 48 and all(c[1] <= 300 for c in params["labeled"])
    for c, (nq, width, _, _, k_pos, k_tot, temp, support, _) in enumerate(params["labeled"]):
        p = f"labeled_{c}"
        want = proposal_ref.sample(g[f"{p}__scores"], g[f"{p}__labels"], g[f"{p}__noise"], k_pos, k_tot, temperature=temp, max_support=support)
        _against_fixture(p, g, p, want, params["e_ref"])
    for c, (width, _, k, temp, support, _) in enumerate(params["single"]):
        p = f"single_{c}"
        want = proposal_ref.sample_row(g[f"{p}__scores"], np.zeros(width, bool), g[f"{p}__noise"], 0, k, temperature=temp,
                                       max_support=support, normalized=False)
        _against_fixture(p, g, p, want, params["e_ref"])


# ---- 3. identities, in float64 -----------------------------------------------------------------------------------------------------
B, W, H, L, V = 4, 9, 6, 5, 13


def _rows(seed=31):
    """Rows with both strata non-empty and unequal masses, one -inf score inside a stratum that keeps finite members."""
    rng = np.random.default_rng(seed)
    scores = (rng.normal(size=(B, W)) * 2).astype(np.float32)
    labels = np.zeros((B, W), bool)
    labels[:, [1, 4, 6]] = True
    scores[0, 2] = scores[2, 4] = -np.inf
    noise = rng.exponential(size=(B, W)).astype(np.float32)
    return scores, labels, noise


def _enumerated(scores, labels, noise, **kw):
    return proposal_ref.sample(scores, labels, noise, W, W, temperature=1.0, **kw)  # k_total >= width, k_positive >= #positives


def _log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def test_full_enumeration_joint_weights_are_the_log_softmax_of_the_scores():
    scores, labels, noise = _rows()
    out = _enumerated(scores, labels, noise)
    assert (out["samples"] >= 0).all()
    want = np.take_along_axis(_log_softmax64(scores), out["samples"], axis=1)
    fin = np.isfinite(want)
    assert fin.sum() == B * W - 2 and np.array_equal(np.isneginf(out["joint"]), ~fin)
    assert np.abs(out["joint"][fin] - want[fin]).max() <= 1e-12


def _lm_inputs(out, scores, seed=32):
    rng = np.random.default_rng(seed)
    mask = (rng.random(size=(B, W, L)) >= 0.25).astype(np.int64)
    mask[..., 1] = 1
    return {"q": rng.normal(size=(B, H)), "s": rng.normal(size=(B, W, H)), "score": np.take_along_axis(scores, out["samples"], axis=1),
            "logits": rng.normal(size=(B, W, L, V)) * 2, "ids": rng.integers(0, V - 1, size=(B, W, L)), "mask": mask}


def _vod_loss(inp, logw, log_proposal=None):
    return vod_ref.vod(inp["q"], inp["s"], inp["score"], logw, inp["logits"], inp["ids"], inp["mask"], alpha=0.0, temperature=1.0,
                       log_proposal=log_proposal)


def test_full_enumeration_both_feeding_modes_give_the_marginal_likelihood_and_the_bare_stratum_weights_do_not():
    scores, labels, noise = _rows()
    out = _enumerated(scores, labels, noise)
    inp = _lm_inputs(out, scores)
    want = marginal_ref.marginal(inp["q"], inp["s"], inp["score"], inp["logits"], inp["ids"], inp["mask"])
    stratum = _vod_loss(inp, out["log_weights"], log_proposal=out["log_p"])
    joint = _vod_loss(inp, out["joint"])
    for got in (stratum, joint):
        for key in ("loss", "retriever_scores", "dq", "ds", "dlogits"):
            assert marginal_ref.scaled_error(got[key], want[key]) <= 1e-12, key
    # (b) what the feature repairs: the collate's output so far - per-stratum weights, no proposal - is NOT the marginal likelihood on
    # rows whose two strata are non-empty and of unequal mass
    assert np.isfinite(out["log_mass"]).all() and np.abs(out["log_mass"][:, 0] - out["log_mass"][:, 1]).min() > 0.05
    bare = _vod_loss(inp, out["log_weights"])
    assert abs(bare["loss"] - want["loss"]) > 1e-3 * abs(want["loss"])
    assert np.abs(bare["Lhat"] - stratum["Lhat"]).min() > 1e-6  # every row is off, not one


def test_joint_weights_and_enumerated_strata_sum_to_one():
    scores, labels, noise = _rows()
    rng = np.random.default_rng(33)
    wide = (rng.normal(size=(3, 150)) * 3).astype(np.float32)
    wl, wn = rng.uniform(size=wide.shape) < 0.3, rng.exponential(size=wide.shape).astype(np.float32)
    for out in (_enumerated(scores, labels, noise), proposal_ref.sample(wide, wl, wn, 8, 32), proposal_ref.sample(wide, wl, wn, 8, 32, temperature=0.5),
                proposal_ref.sample(wide, wl, wn, 8, 32, max_support=40, keep_top=True)):
        assert np.abs(np.exp(out["joint"]).sum(-1) - 1).max() <= 1e-12          # (c)
    out = _enumerated(scores, labels, noise)
    for cls in (True, False):                                                    # (d)
        assert np.abs(np.where(out["labels"] == cls, np.exp(out["log_p"]), 0).sum(-1) - 1).max() <= 1e-12


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_a_row_constant_moves_the_masses_only(temperature):
    rng = np.random.default_rng(34)
    scores = (rng.integers(-64, 65, size=(3, 80)) / 8.0).astype(np.float32)  # multiples of 1/8: score + 4 is exact in float32
    labels, noise = rng.uniform(size=scores.shape) < 0.3, rng.exponential(size=scores.shape).astype(np.float32)
    a = proposal_ref.sample(scores, labels, noise, 4, 16, temperature=temperature)
    b = proposal_ref.sample(scores + np.float32(4), labels, noise, 4, 16, temperature=temperature)
    np.testing.assert_array_equal(a["samples"], b["samples"])
    for key in ("log_p", "joint", "log_weights"):
        assert np.abs(a[key] - b[key]).max() <= 1e-12, key
    assert np.abs(b["log_mass"] - a["log_mass"] - temperature * 4).max() <= 1e-12


def test_pads_empty_strata_and_strata_without_mass():
    scores = np.array([[0.5, -np.inf, 1.0, -np.inf], [-np.inf, 0.25, np.nan, 2.0]], np.float32)
    labels = np.array([[0, 1, 0, 1], [0, 0, 0, 0]], bool)  # row 0: the positives are all -inf; row 1: no positives, a NaN score
    noise = np.ones_like(scores)
    out = proposal_ref.sample(scores, labels, noise, 2, 6)
    assert np.array_equal(out["samples"][:, 4:], np.full((2, 2), -1))
    assert np.isneginf(out["log_p"][:, 4:]).all() and np.isneginf(out["joint"][:, 4:]).all()
    assert np.isneginf(out["log_mass"][:, 0]).all() and np.isfinite(out["log_mass"][:, 1]).all()
    assert not np.isnan(out["joint"]).any()
    assert np.isneginf(out["joint"][0, :2]).all() and np.isnan(out["log_p"][0, :2]).all()  # -inf - (-inf), as the weight formula reads it
    assert np.abs(np.exp(out["joint"]).sum(-1) - 1).max() <= 1e-12


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------------------
def _sections(proposal):
    from vod_amd.core.collate import DeviceSampledSections

    z = torch.zeros((2, 3))
    extra = {"log_proposal": z - 1, "log_mass": torch.zeros((2, 2)), "joint_log_weights": z - 2} if proposal else {}
    return DeviceSampledSections(indices=torch.zeros((2, 3), dtype=torch.int64), scores=z, labels=z > 0, log_weights=z - 3, lse_pos=z[:, 0],
                                 lse_neg=z[:, 0], max_sampling_id=z[:, 0], raw_scores={"dense": z}, **extra)


def test_to_dict_keeps_its_keys_and_the_two_modes_need_the_proposal():
    base = {"p_idx", "p_score", "p_label", "p_log_weight", "p_lse_pos", "p_lse_neg", "p_dense"}
    for s in (_sections(False), _sections(True)):
        assert set(s.to_dict("p_")) == set(s.to_dict("p_", weights=None)) == base
        assert set(s.to_dict("p_", relevances=torch.zeros(2, 3))) == base | {"p_relevance"}
    for mode in ("stratum", "joint"):
        with pytest.raises(ValueError, match="proposal=True"):
            _sections(False).to_dict("p_", weights=mode)
    with pytest.raises(ValueError):
        _sections(True).to_dict("p_", weights="both")
    s = _sections(True)
    d = s.to_dict("p_", weights="stratum")
    assert set(d) == base | {"p_log_proposal", "p_log_mass_pos", "p_log_mass_neg"}
    assert d["p_log_weight"] is s.log_weights and d["p_log_proposal"] is s.log_proposal
    d = s.to_dict("p_", weights="joint")
    assert set(d) == base | {"p_log_mass_pos", "p_log_mass_neg"} and d["p_log_weight"] is s.joint_log_weights


def test_numpy_drop_ins_carry_the_optional_fields():
    import dataclasses
    import inspect

    from vod_amd.core import collate, in_batch_negatives, sample

    names = {f.name: f.default for f in dataclasses.fields(sample.PrioritySampledSections)}
    assert names["log_proposal"] is None and names["log_mass"] is None and names["joint_log_weights"] is None
    for fn in (sample.sample_search_results, in_batch_negatives.flatten_samples, collate.sample_merged_on_device, collate.flatten_on_device,
               collate.collate_on_device):
        assert inspect.signature(fn).parameters["proposal"].default is False, fn.__name__
