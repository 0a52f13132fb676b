"""Generate tests/golden/pooler.npz by RUNNING the reference's VodPooler on CPU float32 with autograd (build container only):

    python tests/golden/make_golden_pooler.py

The fixture is data: seeded inputs, what the reference computed for them (y and, for the loss sum(y * grad), the gradients of the hidden
states, of log_scaler and of the projection), the reference's state-dict keys, and the generator's parameters (`params_json`).
Reference code exercised (relative to the reference's src/): vod_models/vod_encoder/modeling.py:63-181 (Aggregator, MeanAgg, ClsAgg,
VodPooler) with vod_models/vod_encoder/configuration.py (VodPoolerConfig).  Only two empty package shells are fabricated here
(vod_models, vod_models.vod_encoder); product code and GPU tests never import this file.

Every value of hidden, of the projection weight and bias is a multiple of 1/64 and every value of the upstream gradient a multiple of
1/8, all with |x| <= 1: each partial sum over L is exact in float32 IN ANY ORDER, for inputs rounded to fp16 / bf16 too.
Mask mode "masked": the reference is run a second time on hidden * mask; its y is the masked-mode y and its d hidden * mask the
masked-mode gradient (mean aggregator; `cls` ignores the mask, so both modes are the reference on the unchanged hidden).
`params_json["e_ref"][case][cfg][mode][output]` = max |reference - restatement| / max |restatement| against the float64 restatement of
tests/pooler_ref.py: what the reference's own float32 arithmetic costs, the unit of the tests' tolerances.  The reference's d hidden
is non-finite in exactly the fully masked rows of the mean-aggregator runs (`params_json["nonfinite_rows"]`: one row of `mid`); there
the restatement's zeros are the expectation.

Cases (N, L, H):
  tiny   1,1,8      smallest shape
  mid    5,17,72    trailing pads of several lengths, a hole inside a mask, a row with one live token, one fully masked row
  oddh   3,5,67     rows off the 16-byte grid in 16-bit
  wideh  2,3,1032   H beyond one 256-lane x 4 sweep
  longl  2,300,64   many L-chunks
"""
from __future__ import annotations

import io
import json
import pathlib
import sys
import types
import warnings
import zipfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))  # tests/: the float64 restatement
REF_SRC = pathlib.Path("/root/reference/src")

warnings.filterwarnings("ignore")
import torch  # noqa: E402

import pooler_ref  # noqa: E402

CASES = {  # name: (N, L, H, seed)
    "tiny": (1, 1, 8, 6101),
    "mid": (5, 17, 72, 6102),
    "oddh": (3, 5, 67, 6103),
    "wideh": (2, 3, 1032, 6104),
    "longl": (2, 300, 64, 6105),
}
CONFIGS = {
    "mean_l2_s100": {"agg_method": "mean", "output_norm": "l2", "scaler": 100.0},
    "mean_none": {"agg_method": "mean"},
    "mean_tanh": {"agg_method": "mean", "output_activation": "tanh"},
    "mean_l1": {"agg_method": "mean", "output_norm": "l1", "scaler": 4.0},
    "cls_none": {"agg_method": "cls"},
    "cls_l2": {"agg_method": "cls", "output_norm": "l2"},
    "proj": {"agg_method": "mean", "projection_size": 24, "output_activation": "gelu", "output_norm": "l2", "scaler": 100.0,
             "learn_scaler": True},
}
PROJ_CASES = ("tiny", "mid", "oddh")  # the projection's K stays <= 72
MODES = ("reference", "masked")
E_REF_CEILING = 1e-5  # float32 against float64 on these sizes (measured: below 1e-6); a wrong restatement is off by 1e-3 or more
P = 24


def configs_of(case: str) -> list[str]:
    return [c for c in CONFIGS if c != "proj" or case in PROJ_CASES]


def full_config(cfg: str) -> dict:
    return {"projection_size": None, "output_activation": None, "output_norm": None, "agg_method": "mean", "scaler": 1.0,
            "learn_scaler": False, **CONFIGS[cfg]}


def make_inputs(name: str) -> dict[str, np.ndarray]:
    N, L, H, seed = CASES[name]
    rng = np.random.default_rng(seed)
    hidden = (rng.integers(-64, 65, size=(N, L, H)) / 64.0).astype(np.float32)
    grad_h = (rng.integers(-8, 9, size=(N, H)) / 8.0).astype(np.float32)   # upstream gradient of the paths without a projection
    grad_p = (rng.integers(-8, 9, size=(N, P)) / 8.0).astype(np.float32)   # ... and behind the projection
    weight = (rng.integers(-64, 65, size=(P, H)) / 64.0).astype(np.float32)
    bias = (rng.integers(-64, 65, size=(P,)) / 64.0).astype(np.float32)
    mask = np.ones((N, L), dtype=np.uint8)
    if name == "mid":
        mask[1, 12:] = 0      # trailing pads of 5 and 9 tokens
        mask[2, 8:] = 0
        mask[2, 3:5] = 0      # a hole inside the mask
        mask[3, :] = 0
        mask[3, 6] = 1        # a single live token, not the first
        mask[4, :] = 0        # a fully masked row
    elif name == "oddh":
        mask[1, 3:] = 0
        mask[2, 4:] = 0
    elif name == "wideh":
        mask[1, 2:] = 0
    elif name == "longl":
        mask[1, 137:] = 0
        mask[1, 40:45] = 0
    return {"hidden": hidden, "mask": mask, "grad_h": grad_h, "grad_p": grad_p, "weight": weight, "bias": bias}


def import_reference():
    if not REF_SRC.exists():
        raise RuntimeError("the reference checkout is not available: this fixture can only be regenerated in the build container")
    for name, path in (("vod_models", REF_SRC / "vod_models"), ("vod_models.vod_encoder", REF_SRC / "vod_models" / "vod_encoder")):
        mod = types.ModuleType(name)  # an empty package shell: the package's __init__ is never executed
        mod.__path__ = [str(path)]  # type: ignore[attr-defined]
        mod.__package__ = name
        sys.modules[name] = mod
    import importlib

    return importlib.import_module("vod_models.vod_encoder.modeling")


def run_reference(modeling, cfg: str, inp: dict[str, np.ndarray], hidden: np.ndarray) -> tuple[dict[str, np.ndarray], list[str]]:
    conf = full_config(cfg)
    H = hidden.shape[-1]
    pooler = modeling.VodPooler(dict(conf), H)
    keys = list(pooler.state_dict().keys())
    if conf["projection_size"]:
        with torch.no_grad():
            pooler.projection.weight.copy_(torch.from_numpy(inp["weight"]))
            pooler.projection.bias.copy_(torch.from_numpy(inp["bias"]))
    pooler.log_scaler.requires_grad_(True)  # its gradient is recorded for every config
    x = torch.from_numpy(hidden.copy()).requires_grad_()
    y = pooler(x, attention_mask=torch.from_numpy(inp["mask"].astype(np.int64)))
    g = torch.from_numpy(inp["grad_p"] if conf["projection_size"] else inp["grad_h"])
    wrt = [x, pooler.log_scaler] + ([pooler.projection.weight, pooler.projection.bias] if conf["projection_size"] else [])
    grads = torch.autograd.grad((y * g).sum(), wrt)
    out = {"y": y.detach().numpy(), "d_hidden": grads[0].numpy(), "d_log_scaler": grads[1].numpy().reshape(()),
           "log_scaler": pooler.log_scaler.detach().numpy().reshape(())}
    if conf["projection_size"]:
        out["dW"], out["db"] = grads[2].numpy(), grads[3].numpy()
    return out, keys


def restate(cfg: str, inp: dict[str, np.ndarray], mode: str, log_scaler: float) -> dict[str, np.ndarray]:
    conf = full_config(cfg)
    proj = bool(conf["projection_size"])
    return pooler_ref.pool(inp["hidden"], inp["mask"], agg=conf["agg_method"], mode=mode, activation=conf["output_activation"],
                           norm=conf["output_norm"], log_scaler=log_scaler, weight=inp["weight"] if proj else None,
                           bias=inp["bias"] if proj else None, grad=inp["grad_p"] if proj else inp["grad_h"])


def write_npz(path: pathlib.Path, arrays: dict[str, np.ndarray]) -> None:
    """A compressed .npz with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main() -> None:
    torch.manual_seed(0)
    torch.set_num_threads(1)
    modeling = import_reference()
    arrays: dict[str, np.ndarray] = {}
    e_ref: dict = {}
    nonfinite_rows: dict[str, list[int]] = {}
    state_keys: dict[str, list[str]] = {}
    log_scalers: dict[str, float] = {}
    worst = 0.0
    for name in CASES:
        inp = make_inputs(name)
        live = inp["mask"] != 0
        dead = [int(r) for r in np.flatnonzero(~live.any(-1))]
        nonfinite_rows[name] = dead
        e_ref[name] = {}
        for key, val in inp.items():
            arrays[f"{name}__{key}"] = val
        for cfg in configs_of(name):
            conf = full_config(cfg)
            e_ref[name][cfg] = {}
            for mode in MODES:
                # the cls aggregator ignores the mask, so the mask mode does not touch it: both modes are the reference on `hidden`
                zero_pads = mode == "masked" and conf["agg_method"] == "mean"
                hidden = inp["hidden"] * live[..., None].astype(np.float32) if zero_pads else inp["hidden"]
                ref, keys = run_reference(modeling, cfg, inp, hidden)
                state_keys[cfg] = keys
                log_scalers[cfg] = float(ref.pop("log_scaler"))
                # the reference's d hidden is non-finite in EXACTLY the fully masked rows of the mean runs (0 / 0 in its backward)
                bad = ~np.isfinite(ref["d_hidden"])
                expect_bad = np.zeros_like(bad)
                if conf["agg_method"] == "mean":
                    expect_bad[dead] = True
                assert np.array_equal(bad, expect_bad), (name, cfg, mode, sorted(set(np.argwhere(bad)[:, 0].tolist())), dead)
                assert all(np.isfinite(v).all() for k, v in ref.items() if k != "d_hidden"), (name, cfg, mode)
                if zero_pads:
                    ref["d_hidden"] = ref["d_hidden"] * live[..., None].astype(np.float32)  # d hidden * mask, as it is (NaN * 0 = NaN)
                want = restate(cfg, inp, mode, log_scalers[cfg])
                e_ref[name][cfg][mode] = {}
                for out_key, val in ref.items():
                    assert val.dtype == np.float32, (name, cfg, out_key, val.dtype)
                    arrays[f"{name}__{cfg}__{mode}__ref_{out_key}"] = val
                    cmp = val.copy()
                    if out_key == "d_hidden" and conf["agg_method"] == "mean":
                        cmp[dead] = 0.0  # the recorded rows: the restatement's zeros are the expectation
                    assert np.isfinite(cmp).all(), (name, cfg, mode, out_key)
                    e = pooler_ref.scaled_error(cmp, want[out_key])
                    assert e <= E_REF_CEILING, (name, cfg, mode, out_key, e)  # the restatement IS the reference's arithmetic
                    e_ref[name][cfg][mode][out_key] = e
                    worst = max(worst, e)
    params = {"cases": {k: list(v) for k, v in CASES.items()}, "case_fields": ["N", "L", "H", "seed"],
              "configs": {k: full_config(k) for k in CONFIGS}, "proj_cases": list(PROJ_CASES), "modes": list(MODES),
              "projection_size": P, "log_scaler": log_scalers, "state_dict_keys": state_keys, "nonfinite_rows": nonfinite_rows,
              "e_ref": e_ref, "e_ref_ceiling": E_REF_CEILING,
              "fn": "vod_models.vod_encoder.modeling.VodPooler + torch.autograd.grad of sum(y * grad)"}
    arrays["params_json"] = np.array(json.dumps(params, sort_keys=True))
    path = HERE / "pooler.npz"
    write_npz(path, arrays)
    size = path.stat().st_size
    assert size < 1_000_000, size
    print(f"{path.name}: {len(arrays)} arrays, {size / 1024:.1f} KiB, worst e_ref {worst:.2e}")


if __name__ == "__main__":
    main()
