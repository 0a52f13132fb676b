"""Generate tests/golden/proposal.npz by RUNNING the reference's priority sampler on seeded rows with explicit noise (build container only):

    python tests/golden/make_golden_proposal.py

The fixture is data: seeded inputs, what the reference returned for them, and the two quantities it forms and discards, taken from its
own helpers.  Reference code exercised (relative to the reference's src/vod_dataloaders/core): `_labeled_priority_sampling_2d_` and
`_priority_sampling_1d` (sample.py:160-352) for samples / log-weights / labels / lse; `mul_1d_`, `masked_fill_1d_`, `max_1d`,
`_logsumexp_1d` and `log_softmax_1d` (numpy_ops.py:162-224) applied to the SAME strata the sampler splits the row into, for
  log_mass_S = max_1d(a) + _logsumexp_1d(a - max_1d(a))   with a = the stratum's scores after mul_1d_ and the truncation's masked_fill_1d_
  log_p      = log_softmax_1d(a), indexed by the returned samples
  joint      = log_weight + log_mass_S - logaddexp(log_mass_pos, log_mass_neg), in float64 on the reference's float32 values.
The import shim `_ref_shim.py` is used unchanged (numba's decorators become identities: the reference's loops run as written, in float32).

Every case keeps at least as many finite members in a stratum as the sampler draws from it, so no sample is taken among -inf keys
(numpy's order among equal keys is unspecified; tests/test_sampling_gpu.py makes the same exclusion) - asserted below.

`params_json["e_ref"][output]` = max over the cases of max |fixture - restatement| / max(1, max |restatement|) against the float64
restatement of tests/proposal_ref.py (lse is ~0: below 1 the error is absolute): what the reference's own float32, sequentially summed
arithmetic costs.  Measured: log_weights 9.2e-07, log_p 9.1e-08, log_mass 7.2e-08, joint 9.2e-07, lse 4.2e-07 (E_REF_CEILING asserts
they stay below 5e-6; a wrong restatement is off by 1e-2 or more).  tests/test_proposal_cpu.py gates at 4 x the recorded value per
output; samples and labels are exact.

Cases: `labeled` rows go through `_labeled_priority_sampling_2d_`, `single` rows through `_priority_sampling_1d` (one stratum,
unnormalised weights: the restatement with no positive label and normalized=False).
"""
from __future__ import annotations

import io
import json
import pathlib
import sys
import warnings
import zipfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))         # _ref_shim
sys.path.insert(0, str(HERE.parent))  # tests/: the float64 restatement

warnings.filterwarnings("ignore")

import proposal_ref  # noqa: E402

E_REF_CEILING = 5e-6
# labeled: (nq, width, P(positive), P(-inf), k_positive, k_total, temperature, max_support, seed)
LABELED = [
    (2, 1, 0.0, 0.0, 1, 1, 1.0, -1, 7101),        # one candidate
    (2, 2, 0.5, 0.0, 1, 2, 1.0, -1, 7102),
    (3, 17, 0.3, 0.0, 2, 8, 1.0, -1, 7103),
    (3, 17, 0.3, 0.0, 17, 32, 1.0, -1, 7104),     # full enumeration, pads
    (3, 63, 0.2, 0.1, 4, 16, 1.0, -1, 7105),
    (3, 64, 0.2, 0.1, 4, 16, 0.5, -1, 7106),
    (3, 65, 0.0, 0.1, 4, 16, 1.0, -1, 7107),      # no positives
    (3, 40, 1.0, 0.0, 4, 16, 1.0, -1, 7108),      # no negatives: k_positive grows
    (3, 128, 0.5, 0.1, 8, 32, 1.0, -1, 7109),
    (3, 130, 0.8, 0.1, 4, 64, 1.0, -1, 7110),     # fewer finite negatives than k_total - k_positive
    (2, 256, 0.1, 0.05, 8, 32, 1.0, -1, 7111),
    (2, 257, 0.1, 0.05, 8, 32, 0.5, -1, 7112),
    (2, 300, 0.4, 0.0, 8, 32, 1.0, 40, 7113),     # support truncation: the reference REMOVES the best 40 of each stratum
    (2, 300, 0.4, 0.0, 8, 32, 0.5, 100, 7114),
    (2, 300, 0.1, 0.1, 8, 32, 0.0, -1, 7115),     # temperature 0: deterministic top-k
    (2, 100, 0.2, 0.0, 4, 4, 1.0, -1, 7116),      # k_total = k_positive
]
# single: (width, P(-inf), k, temperature, max_support, seed)
SINGLE = [
    (1, 0.0, 1, 1.0, -1, 7201),
    (5, 0.0, 8, 1.0, -1, 7202),                   # k beyond the row
    (64, 0.1, 8, 1.0, -1, 7203),
    (65, 0.1, 8, 0.5, -1, 7204),
    (300, 0.05, 32, 1.0, -1, 7205),
    (300, 0.0, 32, 1.0, 50, 7206),
    (200, 0.1, 16, 0.0, -1, 7207),
]


def labeled_inputs(case):
    nq, width, p_pos, p_inf, _, _, _, _, seed = case
    rng = np.random.default_rng(seed)
    scores = (rng.normal(size=(nq, width)) * 3).astype(np.float32)
    scores[rng.uniform(size=scores.shape) < p_inf] = -np.inf
    labels = rng.uniform(size=scores.shape) < p_pos
    noise = rng.exponential(size=scores.shape).astype(np.float32)
    return scores, labels, noise


def single_inputs(case):
    width, p_inf, _, _, _, seed = case
    rng = np.random.default_rng(seed)
    scores = (rng.normal(size=(width,)) * 3).astype(np.float32)
    scores[rng.uniform(size=scores.shape) < p_inf] = -np.inf
    if np.isinf(scores).all():
        scores[0] = 0.0
    noise = rng.exponential(size=scores.shape).astype(np.float32)
    return scores, noise


def stratum_terms(npo, scores, temperature, max_support):
    """(log_p [m], log_mass) of one stratum from the reference's helpers, as `_priority_sampling_1d` forms them (sample.py:170-180)."""
    dt = scores.dtype
    a = scores.copy()
    npo.mul_1d_(a, dt.type(temperature if temperature > 0 else 1.0))
    if max_support > 0 and len(a) > max_support:
        threshold = np.sort(a)[-max_support]
        npo.masked_fill_1d_(a >= threshold, a, dt.type(-np.inf))
    npo.masked_fill_1d_(np.isnan(a), a, dt.type(-np.inf))
    mx = npo.max_1d(a)
    shifted = a.copy()
    npo.add_1d_(shifted, -mx)
    log_mass = dt.type(mx + npo._logsumexp_1d(shifted))
    return npo.log_softmax_1d(a), log_mass


def joint_of(logw, cls, log_mass):
    mp, mn = np.float64(log_mass[0]), np.float64(log_mass[1])
    tot = np.logaddexp(mp, mn)
    out = np.full(logw.shape, -np.inf)
    for j in range(len(logw)):
        mc = (mp, mn)[cls[j]]
        if cls[j] >= 0 and mc > -np.inf:
            out[j] = np.float64(logw[j]) + mc - tot
    return out


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
    import _ref_shim

    ref = _ref_shim.install()
    smp, npo = ref["sample"], ref["numpy_ops"]
    arrays: dict[str, np.ndarray] = {}
    e_ref = {k: 0.0 for k in ("log_weights", "log_p", "log_mass", "joint", "lse")}

    def record(tag, got, want):
        assert np.array_equal(got["samples"], want["samples"]) and np.array_equal(got["labels"], want["labels"]), tag
        for key in e_ref:
            e = proposal_ref.scaled_error(got[key], want[key])
            assert e <= E_REF_CEILING, (tag, key, e)
            e_ref[key] = max(e_ref[key], e)

    for c, case in enumerate(LABELED):
        nq, width, _, _, k_pos, k_tot, temp, support, _ = case
        scores, labels, noise = labeled_inputs(case)
        out = {"samples": np.full((nq, k_tot), -1, np.int64), "log_weights": np.full((nq, k_tot), -np.inf, np.float32),
               "labels": np.zeros((nq, k_tot), np.bool_), "lse": np.zeros((nq, 2), np.float32)}
        smp._labeled_priority_sampling_2d_(scores, labels, noise, k_pos, k_tot, out["samples"], out["log_weights"], out["labels"],
                                           out["lse"], True, temp, support)
        live = out["samples"] >= 0
        assert np.isfinite(out["log_weights"][live]).all(), (c, "a sample among -inf keys")
        out["log_p"] = np.full((nq, k_tot), -np.inf, np.float32)
        out["log_mass"] = np.zeros((nq, 2), np.float32)
        out["joint"] = np.full((nq, k_tot), -np.inf, np.float64)
        for r in range(nq):
            cls_of = np.where(live[r], np.where(out["labels"][r], 0, 1), -1)
            for cls, members in enumerate((np.flatnonzero(labels[r]), np.flatnonzero(~labels[r]))):
                log_p, out["log_mass"][r, cls] = stratum_terms(npo, scores[r][members], temp, support)
                where = {int(col): i for i, col in enumerate(members)}
                for j in np.flatnonzero(cls_of == cls):
                    out["log_p"][r, j] = log_p[where[int(out["samples"][r, j])]]
            out["joint"][r] = joint_of(out["log_weights"][r], cls_of, out["log_mass"][r])
        record(("labeled", c), out, proposal_ref.sample(scores, labels, noise, k_pos, k_tot, temperature=temp, max_support=support))
        for key, val in {"scores": scores, "labels": labels, "noise": noise, **{f"out_{k}": v for k, v in out.items()}}.items():
            arrays[f"labeled_{c}__{key}"] = val

    for c, case in enumerate(SINGLE):
        width, _, k, temp, support, _ = case
        scores, noise = single_inputs(case)
        ids, logw, lse = smp._priority_sampling_1d(scores, noise, k, temp, support)
        assert np.isfinite(logw).all(), (c, "a sample among -inf keys")
        log_p, log_mass = stratum_terms(npo, scores, temp, support)
        n = len(ids)
        out = {"samples": np.full(k, -1, np.int64), "labels": np.zeros(k, np.bool_), "log_weights": np.full(k, -np.inf, np.float32),
               "log_p": np.full(k, -np.inf, np.float32), "lse": np.array([-np.inf, lse], np.float32),
               "log_mass": np.array([-np.inf, log_mass], np.float32)}
        out["samples"][:n], out["log_weights"][:n], out["log_p"][:n] = ids, logw, log_p[ids]
        out["joint"] = joint_of(out["log_weights"], np.where(out["samples"] >= 0, 1, -1), out["log_mass"])
        want = proposal_ref.sample_row(scores, np.zeros(width, bool), noise, 0, k, temperature=temp, max_support=support, normalized=False)
        record(("single", c), out, want)
        for key, val in {"scores": scores, "noise": noise, **{f"out_{k_}": v for k_, v in out.items()}}.items():
            arrays[f"single_{c}__{key}"] = val

    params = {"labeled": [list(c) for c in LABELED], "single": [list(c) for c in SINGLE],
              "labeled_fields": ["nq", "width", "p_positive", "p_inf", "k_positive", "k_total", "temperature", "max_support", "seed"],
              "single_fields": ["width", "p_inf", "k", "temperature", "max_support", "seed"],
              "e_ref": e_ref, "e_ref_ceiling": E_REF_CEILING,
              "fn": "vod_dataloaders.core.sample._labeled_priority_sampling_2d_ / _priority_sampling_1d + numpy_ops helpers"}
    arrays["params_json"] = np.array(json.dumps(params, sort_keys=True))
    path = HERE / "proposal.npz"
    write_npz(path, arrays)
    size = path.stat().st_size
    assert size < 200_000, size
    print(f"{path.name}: {len(arrays)} arrays, {size / 1024:.1f} KiB, e_ref " + ", ".join(f"{k} {v:.1e}" for k, v in e_ref.items()))


if __name__ == "__main__":
    main()
