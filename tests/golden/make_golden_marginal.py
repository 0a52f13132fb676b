"""Generate tests/golden/marginal_likelihood.npz by RUNNING the reference's MarginalLikelihoodGradients (build container only):

    python tests/golden/make_golden_marginal.py

The fixture is data: seeded float32 inputs, what the reference computed for them (loss, retriever_scores and - through autograd with
an upstream gradient of 1 - the gradients of the query encodings, the section encodings and the LM logits), and the generator's
parameters (`params_json`).  Reference code exercised (paths relative to the reference's src/):
  vod_models/vod_gradients/marginal_likelihood.py:9-66   MarginalLikelihoodGradients.__call__, _compute_lm_logprobs
  vod_models/vod_gradients/retrieval.py:186-203          _compute_retriever_scores
`params_json["e_ref"][case][output]` = max |reference - restatement| / max |restatement| against the float64 restatement of
tests/marginal_ref.py: what the reference's own float32 arithmetic costs on that case, the unit of the tests' tolerances.

Every input is a multiple of 1/8 (of 1/64 for the encodings): exact in float32, and mostly exact in the 16-bit formats the GPU
tests round them to.  Cases (B, D, L, V, H):
  tiny_3d / tiny_2d   1,1,2,7,8      one position, one section
  mid_3d / mid_2d     3,5,17,264,8   trailing pads of every length, a hole inside a mask, a padded section, a row with one live
                                     section, -inf logits off and on the target, logits of magnitude 1e4
  wide_2d             4,70,3,40,520  in-batch sections: D beyond one 64-wide GEMM tile, H >= 512 (split-K)
  oddv_3d             2,2,3,2049,8   odd V: rows off the 16-byte grid
  tailv_2d            2,2,3,4104,8   aligned V that is no multiple of a 256-lane sweep
"""
from __future__ import annotations

import importlib
import json
import pathlib
import sys
import types
import warnings

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))  # tests/: the float64 restatement
import _ref_shim  # noqa: E402

warnings.filterwarnings("ignore")
_ref_shim.install()
import torch  # noqa: E402

import marginal_ref  # noqa: E402

CASES = {  # name: (B, D, L, V, H, sections_3d, seed)
    "tiny_3d": (1, 1, 2, 7, 8, True, 5101),
    "tiny_2d": (1, 1, 2, 7, 8, False, 5102),
    "mid_3d": (3, 5, 17, 264, 8, True, 5103),
    "mid_2d": (3, 5, 17, 264, 8, False, 5104),
    "wide_2d": (4, 70, 3, 40, 520, False, 5105),
    "oddv_3d": (2, 2, 3, 2049, 8, True, 5106),
    "tailv_2d": (2, 2, 3, 4104, 8, False, 5107),
}
E_REF_CEILING = 1e-5  # float32 against float64 on these sizes; a wrong restatement is off by 1e-3 or more
OUTPUTS = ("loss", "retriever_scores", "dq", "ds", "dlogits")


def make_inputs(name: str) -> dict[str, np.ndarray]:
    B, D, L, V, H, three_d, seed = CASES[name]
    rng = np.random.default_rng(seed)
    q = (rng.integers(-64, 65, size=(B, H)) / 64.0).astype(np.float32)
    s = (rng.integers(-64, 65, size=((B, D, H) if three_d else (D, H))) / 64.0).astype(np.float32)
    if H > 64:
        q, s = q / 4, s / 4  # keep the scores of the H = 520 case O(1)
    logits = (rng.integers(-40, 41, size=(B, D, L, V)) / 8.0).astype(np.float32)
    ids = rng.integers(0, V - 1, size=(B, D, L)).astype(np.int64)
    mask = np.ones((B, D, L), dtype=np.int64)
    score = rng.normal(size=(B, D)).astype(np.float32)
    if name.startswith("mid"):
        for b in range(B):
            for d in range(D):
                mask[b, d, L - (b * D + d):] = 0 if (b * D + d) else 1   # trailing pads of 1..14 tokens (the first pair keeps them all)
        mask[1, 2, 5:8] = 0                       # a hole in the middle
        mask[0, 4, 1:] = 0
        mask[0, 4, 9] = 1                         # one live position behind a long hole
        score[0, 2] = -np.inf                     # a padded section
        score[1, :] = -np.inf
        score[1, 3] = 0.25                        # a row with one live section
        logits[0, 0, 3, (ids[0, 0, 4] + 1) % (V - 1)] = -np.inf   # -inf off the target
        logits[0, 1, 2, 8:40] = -np.inf
        logits[0, 1, 2, ids[0, 1, 3]] = 1.0
        logits[2, 1, 4, ids[2, 1, 5]] = -np.inf   # -inf ON the target: the section carries zero posterior
        logits[2, 3] += 1.0e4                     # magnitude 1e4 (still multiples of 1/8 in float32)
        logits[2, 0, :4] -= 1.0e4
    elif name == "wide_2d":
        mask[:, 1::3, 2] = 0                      # trailing pad
        mask[:, 2::3, 1] = 0                      # a hole: only t = 1 is live
        score[:, 5::7] = -np.inf
        score[3, :] = -np.inf
        score[3, 69] = 1.0                        # one live section, in the second GEMM tile
        logits[1, 64, 0, (ids[1, 64, 1] + 3) % (V - 1)] = -np.inf
    elif name in ("oddv_3d", "tailv_2d"):
        mask[1, 0, 2] = 0
        mask[0, 1, 1] = 0
        score[1, 1] = -np.inf
        logits[0, 0, 1, V - 1] = -np.inf          # the last column: normalised over, never a target
        logits[1, 0, 0, 5:V - 3] = -np.inf
        logits[1, 0, 0, ids[1, 0, 1]] = 0.5
        logits[0, 0, 0] *= 250.0                  # |logits| up to 1250: a sharp row
    return {"q": q, "s": s, "score": score, "logits": logits, "ids": ids, "mask": mask}


def run_reference(inp: dict[str, np.ndarray]) -> dict[str, np.ndarray]:
    mod = importlib.import_module("vod_models.vod_gradients.marginal_likelihood")
    q = torch.from_numpy(inp["q"]).requires_grad_()
    s = torch.from_numpy(inp["s"]).requires_grad_()
    lg = torch.from_numpy(inp["logits"]).requires_grad_()
    batch = types.SimpleNamespace(section__score=torch.from_numpy(inp["score"]), lm__input_ids=torch.from_numpy(inp["ids"]),
                                  lm__attention_mask=torch.from_numpy(inp["mask"]))
    out = mod.MarginalLikelihoodGradients()(batch=batch, query_encoding=q, section_encoding=s, lm_logits=lg)
    loss, scores = (out["loss"], out["retriever_scores"]) if isinstance(out, dict) else (out.loss, out.retriever_scores)
    dq, ds, dlg = torch.autograd.grad(loss, [q, s, lg])
    return {"loss": loss.detach().numpy(), "retriever_scores": scores.detach().numpy(), "dq": dq.numpy(), "ds": ds.numpy(),
            "dlogits": dlg.numpy()}


def main() -> None:
    arrays: dict[str, np.ndarray] = {}
    e_ref: dict[str, dict[str, float]] = {}
    for name in CASES:
        inp = make_inputs(name)
        ref = run_reference(inp)
        want = marginal_ref.marginal(inp["q"], inp["s"], inp["score"], inp["logits"], inp["ids"], inp["mask"])
        e_ref[name] = {}
        for key in OUTPUTS:
            assert ref[key].dtype == np.float32, (name, key, ref[key].dtype)
            if key == "retriever_scores":
                assert np.isfinite(ref[key]).sum() == (~np.isinf(inp["score"])).sum(), (name, key)
            else:
                assert np.isfinite(ref[key]).all(), (name, key)  # every case of the fixture is meant to be finite
            e_ref[name][key] = marginal_ref.scaled_error(ref[key], want[key])
            assert e_ref[name][key] <= E_REF_CEILING, (name, key, e_ref[name][key])  # the restatement IS the reference's arithmetic
            arrays[f"{name}__ref_{key}"] = ref[key]
        for key, val in inp.items():
            arrays[f"{name}__{key}"] = val.astype(np.uint8) if key == "mask" else (val.astype(np.int32) if key == "ids" else val)
    params = {"cases": {k: list(v[:5]) + [bool(v[5]), v[6]] for k, v in CASES.items()}, "case_fields": ["B", "D", "L", "V", "H", "sections_3d", "seed"],
              "outputs": list(OUTPUTS), "grad_out": 1.0, "e_ref": e_ref,
              "fn": "vod_models.vod_gradients.marginal_likelihood.MarginalLikelihoodGradients + torch.autograd.grad"}
    arrays["params_json"] = np.array(json.dumps(params, sort_keys=True))
    path = HERE / "marginal_likelihood.npz"
    np.savez_compressed(path, **arrays)
    size = path.stat().st_size
    assert size < 1_000_000, size
    print(f"{path.name}: {len(arrays)} arrays, {size / 1024:.1f} KiB")
    print(json.dumps(e_ref, indent=1))


if __name__ == "__main__":
    main()
