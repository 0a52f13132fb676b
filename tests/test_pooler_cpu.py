"""The pooling head without a GPU: the float64 restatement (tests/pooler_ref.py) against what the reference computed
(tests/golden/pooler.npz) and against finite differences, the mask-mode identity, the construction rules of `VodPooler` and the new
entry points in the header and the ctypes table."""
import functools
import json
import pathlib
import re

import numpy as np
import pytest

import pooler_ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
E_REF_CEILING = 1e-5  # also asserted by tests/golden/make_golden_pooler.py when it writes the fixture
CASES = ["tiny", "mid", "oddh", "wideh", "longl"]
CONFIGS = ["mean_l2_s100", "mean_none", "mean_tanh", "mean_l1", "cls_none", "cls_l2", "proj"]
MODES = ["reference", "masked"]
NEW_SYMBOLS = {"vodhip_pool_workspace_floats": 4, "vodhip_pool_forward": 20, "vodhip_pool_backward": 19,
               "vodhip_pool_finish_forward": 10, "vodhip_pool_finish_backward": 13}


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(ROOT / "tests" / "golden" / "pooler.npz")
    return z, json.loads(str(z["params_json"]))


def pairs():
    _, params = fixture()
    return [(c, k) for c in CASES for k in CONFIGS if k != "proj" or c in params["proj_cases"]]


def restate(z, params, case, cfg, mode, hidden=None, log_scaler=None):
    conf = params["configs"][cfg]
    proj = conf["projection_size"] is not None
    return pooler_ref.pool(
        z[f"{case}__hidden"] if hidden is None else hidden, z[f"{case}__mask"], agg=conf["agg_method"], mode=mode,
        activation=conf["output_activation"], norm=conf["output_norm"],
        log_scaler=params["log_scaler"][cfg] if log_scaler is None else log_scaler,
        weight=z[f"{case}__weight"] if proj else None, bias=z[f"{case}__bias"] if proj else None,
        grad=z[f"{case}__grad_p"] if proj else z[f"{case}__grad_h"])


def test_fixture_holds_the_cases_and_only_data():
    z, params = fixture()
    assert (ROOT / "tests" / "golden" / "pooler.npz").stat().st_size < 1_000_000
    assert {k: v[:3] for k, v in params["cases"].items()} == {"tiny": [1, 1, 8], "mid": [5, 17, 72], "oddh": [3, 5, 67],
                                                              "wideh": [2, 3, 1032], "longl": [2, 300, 64]}
    assert sorted(params["configs"]) == sorted(CONFIGS) and params["proj_cases"] == ["tiny", "mid", "oddh"]
    assert params["nonfinite_rows"] == {"tiny": [], "mid": [4], "oddh": [], "wideh": [], "longl": []}
    for key in z.files:
        assert z[key].dtype.kind in "fiuU", (key, z[key].dtype)  # numbers and the parameter string: no pickled objects
    m = z["mid__mask"].astype(np.int64)
    assert (m.sum(-1) == 0).sum() == 1 and (m.sum(-1) == 1).any() and (m.sum(-1) == m.shape[1]).any()
    assert (np.diff(m, axis=-1) == 1).any(), "a hole: 0 followed by 1"
    for case in CASES:  # multiples of 1/64 (1/8 for the gradients) within [-1, 1]: sums over L are exact in float32 in any order
        for key, q in (("hidden", 64), ("weight", 64), ("bias", 64), ("grad_h", 8), ("grad_p", 8)):
            v = z[f"{case}__{key}"].astype(np.float64)
            assert np.array_equal(v * q, np.round(v * q)) and np.abs(v).max() <= 1.0, (case, key)


@pytest.mark.parametrize("case,cfg", pairs())
@pytest.mark.parametrize("mode", MODES)
def test_restatement_meets_the_reference(case, cfg, mode):
    """(a) every reference output of the fixture; only the recorded fully masked rows of d hidden are left out (zeros expected)."""
    z, params = fixture()
    want = restate(z, params, case, cfg, mode)
    dead = params["nonfinite_rows"][case]
    outputs = ["y", "d_hidden", "d_log_scaler"] + (["dW", "db"] if cfg == "proj" else [])
    for key in outputs:
        ref = z[f"{case}__{cfg}__{mode}__ref_{key}"]
        assert ref.dtype == np.float32
        got = ref.astype(np.float64)
        if key == "d_hidden" and params["configs"][cfg]["agg_method"] == "mean" and dead:
            assert not np.isfinite(got[dead]).any() and np.all(want[key][dead] == 0)
            got[dead] = 0.0
        e = pooler_ref.scaled_error(got, want[key])
        stored = params["e_ref"][case][cfg][mode][key]
        assert stored <= E_REF_CEILING and e <= E_REF_CEILING, (case, cfg, mode, key, e, stored)
        assert e <= max(4 * stored, 1e-12), (case, cfg, mode, key, e, stored)


@pytest.mark.parametrize("case,cfg", [p for p in pairs() if p[0] in ("tiny", "mid")])
@pytest.mark.parametrize("mode", MODES)
def test_restatement_backward_matches_finite_differences(case, cfg, mode):
    """(b) central differences in float64 of L = sum(y * grad) along random directions of hidden, and along log_scaler, W and b."""
    z, params = fixture()
    conf = params["configs"][cfg]
    proj = conf["projection_size"] is not None
    g = (z[f"{case}__grad_p"] if proj else z[f"{case}__grad_h"]).astype(np.float64)
    hidden, ls = z[f"{case}__hidden"].astype(np.float64), params["log_scaler"][cfg]
    base = restate(z, params, case, cfg, mode)
    rng = np.random.default_rng(11)
    eps = 1e-6

    def loss(h=hidden, s=ls, w=None, b=None):
        kw = dict(agg=conf["agg_method"], mode=mode, activation=conf["output_activation"], norm=conf["output_norm"], log_scaler=s)
        if proj:
            kw.update(weight=z[f"{case}__weight"].astype(np.float64) if w is None else w,
                      bias=z[f"{case}__bias"].astype(np.float64) if b is None else b)
        return float((pooler_ref.pool(h, z[f"{case}__mask"], **kw)["y"] * g).sum())

    def check(numeric, analytic, what):
        assert abs(numeric - analytic) <= 1e-6 * max(1.0, abs(analytic)), (case, cfg, mode, what, numeric, analytic)

    for _ in range(3):
        d = rng.standard_normal(hidden.shape)
        check((loss(h=hidden + eps * d) - loss(h=hidden - eps * d)) / (2 * eps), float((base["d_hidden"] * d).sum()), "d_hidden")
    check((loss(s=ls + eps) - loss(s=ls - eps)) / (2 * eps), float(base["d_log_scaler"]), "d_log_scaler")
    if proj:
        w, b = z[f"{case}__weight"].astype(np.float64), z[f"{case}__bias"].astype(np.float64)
        dw, db = rng.standard_normal(w.shape), rng.standard_normal(b.shape)
        check((loss(w=w + eps * dw) - loss(w=w - eps * dw)) / (2 * eps), float((base["dW"] * dw).sum()), "dW")
        check((loss(b=b + eps * db) - loss(b=b - eps * db)) / (2 * eps), float((base["db"] * db).sum()), "db")


@pytest.mark.parametrize("case,cfg", [p for p in pairs() if p[1].startswith("mean") or p[1] == "proj"])
def test_masked_mode_is_reference_mode_on_zeroed_pads(case, cfg):
    """(c) masked(x) == reference(x * mask); the gradients agree on live positions and masked mode has zeros on padded ones."""
    z, params = fixture()
    live = z[f"{case}__mask"] != 0
    masked = restate(z, params, case, cfg, "masked")
    zeroed = restate(z, params, case, cfg, "reference", hidden=z[f"{case}__hidden"] * live[..., None])
    assert np.array_equal(masked["y"], zeroed["y"])
    assert np.array_equal(masked["d_hidden"][live], zeroed["d_hidden"][live])
    assert np.all(masked["d_hidden"][~live] == 0)
    poisoned = np.where(live[..., None], z[f"{case}__hidden"], np.nan)
    assert np.array_equal(restate(z, params, case, cfg, "masked", hidden=poisoned)["y"], masked["y"])


def test_fully_masked_row_is_zero_output_and_zero_gradient():
    z, params = fixture()
    for cfg in ("mean_l2_s100", "mean_none", "mean_tanh", "mean_l1"):
        for mode in MODES:
            out = restate(z, params, "mid", cfg, mode)
            assert np.all(out["y"][4] == 0) and np.all(out["d_hidden"][4] == 0)
            assert all(np.isfinite(v).all() for v in out.values())


def test_vodpooler_construction_and_state_dict():
    """(d) state-dict parity with the reference, the refused aggregators, and no CPU path."""
    torch = pytest.importorskip("torch")
    from vod_amd import _native
    from vod_amd.pooler import VodPooler

    z, params = fixture()
    for cfg, conf in params["configs"].items():
        pooler = VodPooler(dict(conf), 72)
        assert list(pooler.state_dict().keys()) == params["state_dict_keys"][cfg], cfg
        assert pooler.log_scaler.requires_grad is bool(conf["learn_scaler"])
        assert float(pooler.log_scaler.detach()) == params["log_scaler"][cfg]
    assert params["state_dict_keys"]["mean_none"] == ["log_scaler", "aggregator._dtype_marker"]
    assert params["state_dict_keys"]["proj"] == ["log_scaler", "aggregator._dtype_marker", "projection.weight", "projection.bias"]
    pooler = VodPooler(dict(params["configs"]["proj"]), 72)
    state = {"log_scaler": torch.tensor(1.5), "aggregator._dtype_marker": torch.zeros(1),
             "projection.weight": torch.from_numpy(z["mid__weight"]), "projection.bias": torch.from_numpy(z["mid__bias"])}
    pooler.load_state_dict(state, strict=True)
    assert torch.equal(pooler.projection.weight.detach(), state["projection.weight"]) and float(pooler.log_scaler.detach()) == 1.5
    assert pooler.output_vector_size == 24 and pooler.get_encoding_shape() == (24,)

    class Config:  # an object with the six fields works like a dict
        projection_size, output_activation, output_norm, agg_method, scaler, learn_scaler = None, "tanh", "l1", "cls", 4.0, True

    assert VodPooler(Config(), 8).log_scaler.requires_grad
    with pytest.raises(ValueError, match=r"\[N, 1, 1\]"):
        VodPooler({"agg_method": "max"}, 8)
    with pytest.raises(ValueError, match="not a pooling"):
        VodPooler({"agg_method": "none"}, 8)
    with pytest.raises(ValueError, match="output_activation"):
        VodPooler({"output_activation": "swish"}, 8)
    with pytest.raises(ValueError, match="mask_mode"):
        VodPooler({}, 8, mask_mode="fixed")
    with pytest.raises(_native.NativeLibraryError, match="no CPU path"):
        VodPooler({}, 8)(torch.zeros(2, 3, 8), attention_mask=torch.ones(2, 3, dtype=torch.int64))


def test_header_declares_the_entry_points_and_signatures_carry_them():
    """(e)"""
    from vod_amd import _native

    header = (ROOT / "include" / "vodhip.h").read_text()
    for name, n_args in NEW_SYMBOLS.items():
        assert re.search(rf"\bint(64_t)? {name}\s*\(", header), name
        _, args = _native.SIGNATURES[name]
        assert len(args) == n_args, name
    for macro in ("VODHIP_POOL_AGG_CLS", "VODHIP_POOL_MASK_MASKED", "VODHIP_POOL_ACT_GELU", "VODHIP_POOL_NORM_L1"):
        assert re.search(rf"#define {macro}\b", header), macro
