"""GPU tests of the collate-side kernels (vod_amd/csrc/kernels_sample.hip) at the limits include/vodhip.h documents.

  1. `flatten_inbatch_kernel` through `flatten_on_device` and the raw `vodhip_flatten_inbatch`, at every sort-size edge (U = 1023 / 1024 /
     1025, 2049 / 4096 / 4097: the 4096-key network), at the largest shapes its LDS holds (7 x 1024, 8 x 1000), and at the corner the LDS
     does not hold: 8 x 1024 is refused by the C entry points before a launch and `flatten_samples` takes the `vodhip_gather_by_id`
     path for it (tests/test_collate_plan_cpu.py has the arithmetic).  Ids: a mix with 1 and -1 present, all equal, all distinct,
     and ids that differ only above bit 32.
  2. `gather_by_id_kernel` directly (`gather_by_id_tensors`) and through the two `flatten_samples` shapes that must take it.
  3. `priority_sample_kernel` with k_total above its 256 threads, up to the 4096 the header admits, against tests/proposal_ref.py
     with the gate and the `_compare` of tests/test_proposal_gpu.py (each case prints its `PROPERR` lines: run with `-s`).
  4. exactly tied priority keys and a support threshold inside a run of equal scores: the smaller column wins.

Everything in 1. and 2. is a copy or an integer operation: every comparison against `oracle.sampling.flatten_samples` /
`oracle.hybrid.gather_values` is exact, bit for bit, NaN positions included.  Each reference is computed once and never modified.
"""
import ctypes
import functools

import numpy as np
import pytest

import proposal_ref

torch = pytest.importorskip("torch")
import test_proposal_gpu as tp  # noqa: E402  (its `_sample` / `_compare` / gate are reused, not restated)

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _assert_same_bits(got, want, msg):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (msg, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _stream():
    from vod_amd import _native

    return _native.current_stream_ptr(torch.device("cuda", torch.cuda.current_device()))


def _last_error():
    from vod_amd import _native

    return _native.load_library().vodhip_last_error().decode()


def _values(rng, shape):
    """float32 with NaN, -inf and -0.0 sprinkled in: a gather is a copy, so every bit pattern must come through."""
    v = rng.standard_normal(shape).astype(np.float32)
    r = rng.random(shape)
    v[r < 0.05] = np.nan
    v[(r >= 0.05) & (r < 0.10)] = -np.inf
    v[(r >= 0.10) & (r < 0.13)] = -0.0
    return v


# ---- 1. the one-launch flattening ---------------------------------------------------------------------------------------------------
FLAT_SHAPES = [(1, 1023), (1, 1024), (5, 205),    # U = 1023 / 1024 / 1025: the edge between the 1024- and the 2048-key sort
               (3, 683), (4, 1024), (17, 241),    # U = 2049 / 4096 / 4097: the 4096-key network (4 keys per thread) and its upper edge
               (7, 1024),                         # the largest per-row count of a batch of more than 4096 ids that fits
               (8, 1000)]                         # 162,616 bytes of LDS: within 1.3 KB of the workgroup's 163,840
ID_KINDS = ("mixed", "equal", "distinct", "high")
RAW = tuple(f"r{i}" for i in range(6))            # scores + log-weights + 6 raw arrays = the 8 value arrays one launch carries


def _ids(rng, B, n, kind):
    U = B * n
    if kind == "mixed":   # duplicates inside and across rows; 1 (the padding value) and -1 (the sampler's pad) are present
        ids = rng.integers(-1, max(U // 2, 3), size=(B, n)).astype(np.int64)
        ids.reshape(-1)[rng.choice(U, size=2, replace=False)] = (1, -1)
        return ids
    if kind == "equal":
        return np.full((B, n), 7, np.int64)
    if kind == "distinct":  # -1, 0, 1, ..., U - 2: nothing to pad
        return (rng.permutation(U).astype(np.int64) - 1).reshape(B, n)
    hi = rng.integers(-(U // 4) - 1, U // 4 + 2, size=(B, n)).astype(np.int64)  # the low 32 bits are the same everywhere, both signs
    return 5 + (hi << 32)


@functools.lru_cache(maxsize=None)
def _flat_case(B, n, kind):
    """(ids, labels, the 8 value arrays by name, the oracle's flattening with padding), read-only."""
    from oracle import sampling as osmp

    rng = np.random.default_rng(9100 + 7919 * B + 13 * n + ID_KINDS.index(kind))
    ids = _ids(rng, B, n, kind)
    labels = rng.random((B, n)) < 0.3
    vals = {name: _values(rng, (B, n)) for name in ("scores", "log_weights", *RAW)}
    ref = osmp.flatten_samples(ids, vals["scores"], labels, vals["log_weights"], {k: vals[k] for k in RAW}, padding=True)
    want = {"indices": ref["indices"], "labels": ref["labels"], "scores": ref["scores"], "log_weights": ref["log_weights"], **ref["raw"],
            "n_unique": len(np.unique(ids))}
    for a in (ids, labels, *vals.values(), *[v for v in want.values() if isinstance(v, np.ndarray)]):
        a.setflags(write=False)
    return ids, labels, vals, want


def _device_sections(ids, labels, vals):
    from vod_amd.core.collate import DeviceSampledSections

    zero = torch.zeros((ids.shape[0],), device="cuda")
    return DeviceSampledSections(indices=tp._t(ids), scores=tp._t(vals["scores"]), labels=tp._t(labels), log_weights=tp._t(vals["log_weights"]),
                                 lse_pos=zero, lse_neg=zero, max_sampling_id=zero, raw_scores={k: tp._t(vals[k]) for k in RAW})


def _raw_flatten(ids, values, labels, with_count=True):
    """One call of `vodhip_flatten_inbatch`; every output is pre-filled so that a slot nobody wrote shows.  -> (status, outputs on the host)"""
    from vod_amd import _native

    lib = _native.load_library()
    B, n = ids.shape
    U = B * n
    d_ids, d_vals = tp._t(ids), [tp._t(v) for v in values]
    outs = [torch.full((B, U), 7.0, device="cuda") for _ in values]
    uq = torch.full((U,), -7, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_lab = None if labels is None else tp._t(labels.astype(np.uint8))
    o_lab = None if labels is None else torch.full((B, U), 7, dtype=torch.uint8, device="cuda")
    nv = len(values)
    status = lib.vodhip_flatten_inbatch(d_ids.data_ptr(), B, n, nv, _ptrs(d_vals), (ctypes.c_float * nv)(*[float("nan")] * nv), _ptrs(outs),
                                        None if labels is None else d_lab.data_ptr(), None if labels is None else o_lab.data_ptr(),
                                        uq.data_ptr(), cnt.data_ptr() if with_count else None, _stream())
    torch.cuda.synchronize()
    return status, {"outs": [o.cpu().numpy() for o in outs], "indices": uq.cpu().numpy(), "n_unique": int(cnt.item()),
                    "labels": None if labels is None else o_lab.cpu().numpy()}


def _untouched(out):
    return (all((o == 7.0).all() for o in out["outs"]) and (out["indices"] == -7).all() and out["n_unique"] == -7
            and (out["labels"] is None or (out["labels"] == 7).all()))


@pytest.mark.parametrize("kind", ID_KINDS)
@pytest.mark.parametrize("B,n", FLAT_SHAPES)
def test_flatten_on_device_is_the_oracles_flattening(B, n, kind):
    """8 value arrays and the labels in one launch; ids list, distinct count, every value array and the labels, bit for bit."""
    from vod_amd.core.collate import flatten_on_device

    ids, labels, vals, want = _flat_case(B, n, kind)
    flat = flatten_on_device(_device_sections(ids, labels, vals))
    assert int(flat.n_unique.item()) == want["n_unique"]
    _assert_same_bits(flat.indices.cpu().numpy(), want["indices"], "indices")
    _assert_same_bits(flat.labels.cpu().numpy(), want["labels"], "labels")
    _assert_same_bits(flat.scores.cpu().numpy(), want["scores"], "scores")
    _assert_same_bits(flat.log_weights.cpu().numpy(), want["log_weights"], "log_weights")
    for k in RAW:
        _assert_same_bits(flat.raw_scores[k].cpu().numpy(), want[k], k)
    if kind == "equal":
        assert want["n_unique"] == 1 and (want["indices"][1:] == 1).all()
    if kind == "distinct":
        assert want["n_unique"] == B * n


@pytest.mark.parametrize("B,n", FLAT_SHAPES)
def test_raw_flatten_entry_point_without_labels_and_without_the_count(B, n):
    """`vodhip_flatten_inbatch` itself with 3 value arrays, `labels` and `out_n_unique` NULL: the same lists, and the staging of fewer
    arrays than the 8 the LDS is carved for."""
    ids, _, vals, want = _flat_case(B, n, "mixed")
    names = ("scores", "r0", "r5")
    status, out = _raw_flatten(ids, [vals[k] for k in names], None, with_count=False)
    assert status == 0, _last_error()
    _assert_same_bits(out["indices"], want["indices"], "indices")
    for k, got in zip(names, out["outs"]):
        _assert_same_bits(got, want[k], k)
    assert out["n_unique"] == -7


def _corner_inputs():
    rng = np.random.default_rng(9200)
    ids = _ids(rng, 8, 1024, "mixed")
    labels = rng.random(ids.shape) < 0.3
    vals = {name: _values(rng, ids.shape) for name in ("scores", "log_weights", "dense", "sparse")}
    return ids, labels, vals


@pytest.mark.parametrize("B,n,word", [(8, 1024, "1012"), (8, 1013, "1012"), (1, 1025, "1024 per row"), (9, 1024, "8192")])
def test_shapes_the_flattening_does_not_hold_are_refused_and_the_next_call_works(B, n, word):
    """8 x 1013 ... 1024 need more LDS than a workgroup has (collate_plan.h); 1025 ids per row and 9216 ids are past the two size bounds.
    The C entry point refuses each before a launch: a negative status, a message that names the bound, every output as it was."""
    from vod_amd import _native
    from vod_amd.core.collate import flatten_on_device

    rng = np.random.default_rng(9300 + B + n)
    ids = rng.integers(-1, 5000, size=(B, n)).astype(np.int64)
    labels = rng.random((B, n)) < 0.3
    vals = [_values(rng, (B, n)) for _ in range(8)]
    status, out = _raw_flatten(ids, vals, labels)
    assert status < 0 and _untouched(out)
    assert word in _last_error(), _last_error()
    assert _native.load_library().vodhip_flatten_inbatch_admits(B, n) == 0
    with pytest.raises(_native.NativeLibraryError, match=word):
        flatten_on_device(_device_sections(ids, labels, dict(zip(("scores", "log_weights", *RAW), vals))))
    ids2, labels2, vals2, want = _flat_case(5, 205, "mixed")  # the next call works
    status, out = _raw_flatten(ids2, [vals2["scores"]], labels2)
    assert status == 0, _last_error()
    _assert_same_bits(out["indices"], want["indices"], "indices")
    _assert_same_bits(out["outs"][0], want["scores"], "scores")
    _assert_same_bits(out["labels"] != 0, want["labels"], "labels")
    assert out["n_unique"] == want["n_unique"]


def _sampled(ids, labels, vals, raw_names):
    from vod_amd import types as vt
    from vod_amd.core.sample import PrioritySampledSections

    z = np.zeros(ids.shape[0])
    return PrioritySampledSections(batch=vt.RetrievalBatch(indices=ids, scores=vals["scores"], labels=labels), log_weights=vals["log_weights"],
                                   max_sampling_id=z, lse_pos=z, lse_neg=z, raw_scores={k: vals[k] for k in raw_names})


def _check_flatten_samples(ids, labels, vals, raw_names, padding):
    from oracle import sampling as osmp
    from vod_amd.core.in_batch_negatives import flatten_samples

    out = flatten_samples(_sampled(ids, labels, vals, raw_names), padding=padding)
    ref = osmp.flatten_samples(ids, vals["scores"], labels, vals["log_weights"], {k: vals[k] for k in raw_names}, padding=padding)
    _assert_same_bits(out.batch.indices, ref["indices"], "indices")
    _assert_same_bits(out.batch.labels, ref["labels"], "labels")
    _assert_same_bits(out.batch.scores, ref["scores"], "scores")
    _assert_same_bits(out.log_weights, ref["log_weights"], "log_weights")
    for k in raw_names:
        _assert_same_bits(out.raw_scores[k], ref["raw"][k], k)


def _forbid_the_one_launch_path(monkeypatch):
    from vod_amd.core import in_batch_negatives

    def refuse(*a, **kw):
        raise AssertionError("this batch must not take the one-launch flattening")

    monkeypatch.setattr(in_batch_negatives, "_flatten_one_launch", refuse)


@pytest.mark.parametrize("padding", [True, False])
def test_flatten_samples_takes_the_gather_path_at_the_corner(padding, monkeypatch):
    """8 x 1024: `flatten_samples` gives the oracle's result through `torch.unique` + `vodhip_gather_by_id`."""
    _forbid_the_one_launch_path(monkeypatch)
    ids, labels, vals = _corner_inputs()
    _check_flatten_samples(ids, labels, vals, ("dense", "sparse"), padding)


def test_collate_on_device_refuses_the_corner_before_any_launch(monkeypatch):
    """`collate_on_device` raises on its own guard; with that guard answered "yes" the C entry point refuses, before the merge."""
    from vod_amd import _native
    from vod_amd.core import collate

    l_idx, l_lbl, engines, weights, noise = tp._collate_inputs(8, 4, (40, 30), 200, 9400)
    kw = dict(total=1024, max_pos_sections=4, in_batch_negatives=True)
    with pytest.raises(ValueError, match="1012"):
        collate.collate_on_device(l_idx, l_lbl, engines, weights, noise, **kw)
    lib = _native.load_library()

    class Yes:
        def __getattr__(self, name):
            return getattr(lib, name)

        def vodhip_flatten_inbatch_admits(self, n_rows, n_keys):
            return 1

    with monkeypatch.context() as m:
        m.setattr(collate._native, "load_library", lambda: Yes())
        with pytest.raises(_native.NativeLibraryError, match="1012"):
            collate.collate_on_device(l_idx, l_lbl, engines, weights, noise, **kw)
    out = collate.collate_on_device(l_idx, l_lbl, engines, weights, noise, total=1000, max_pos_sections=4, in_batch_negatives=True)  # 8 x 1000 fits
    assert out.scores.shape == (8, 8000) and int(out.n_unique.item()) > 1


# ---- 2. gather by id ----------------------------------------------------------------------------------------------------------------
GATHER_ROWS = 3
FILLS = (float("nan"), 0.0, float("-inf"))


@functools.lru_cache(maxsize=None)
def _gather_case(n_queries, n_keys, n_values):
    """Keys drawn with replacement from a pool (duplicates: the first occurrence wins), queries from a pool twice as large (absent ids),
    fills NaN / 0 / -inf in turn.  -> (queries, keys, values, fills, oracle outputs)"""
    from oracle.hybrid import gather_values

    rng = np.random.default_rng(9500 + 31 * n_queries + n_keys)
    pool = max(2, n_keys // 2)
    keys = rng.integers(-1, pool, size=(GATHER_ROWS, n_keys)).astype(np.int64)
    queries = rng.integers(-1, 2 * pool, size=(n_queries,)).astype(np.int64)
    values = [_values(rng, (GATHER_ROWS, n_keys)) for _ in range(n_values)]
    fills = [FILLS[(v + n_keys + n_queries) % 3] for v in range(n_values)]
    uq = np.broadcast_to(queries, (GATHER_ROWS, n_queries))
    want = [gather_values(uq, keys, v, fill_value=f) for v, f in zip(values, fills)]
    return queries, keys, values, fills, want


@pytest.mark.parametrize("n_queries", [1, 255, 256, 257, 9000])
@pytest.mark.parametrize("n_keys", [0, 1, 255, 256, 257, 4096])
def test_gather_by_id_matches_the_oracle(n_keys, n_queries):
    """One thread per query id, 256 per row: 255 / 256 / 257 ids are one block's edge, 9000 is 36 strides; 0 keys is all fill."""
    from vod_amd.core.in_batch_negatives import gather_by_id_tensors

    for n_values in (1, 8):
        queries, keys, values, fills, want = _gather_case(n_queries, n_keys, n_values)
        got = gather_by_id_tensors(tp._t(queries), tp._t(keys), [tp._t(v) for v in values], fills)
        for v in range(n_values):
            _assert_same_bits(got[v].cpu().numpy(), want[v], f"values={n_values} array {v} fill {fills[v]}")
        if n_keys <= 1:
            hit = (queries[None, :] == keys[:, :1]) if n_keys else np.zeros((GATHER_ROWS, n_queries), bool)
            fill_bits = _bits(np.float32(fills[0]).reshape(1))[0]
            assert (_bits(got[0].cpu().numpy())[~hit] == fill_bits).all()


def test_gather_by_id_first_occurrence_wins_and_absent_ids_take_each_fill():
    from vod_amd.core.in_batch_negatives import gather_by_id_tensors

    keys = np.array([[5, 5, 9, 5, 9, -1, -1], [9, 9, 9, 9, 9, 9, 9]], np.int64)
    queries = np.array([9, 5, -1, 4, 5 + (1 << 32), 9], np.int64)
    vals = np.arange(14, dtype=np.float32).reshape(2, 7) + 100
    got = gather_by_id_tensors(tp._t(queries), tp._t(keys), [tp._t(vals)] * 3, list(FILLS))
    for g, fill in zip(got, FILLS):
        want = np.array([[102, 100, 105, fill, fill, 102], [107, fill, fill, fill, fill, 107]], np.float32)
        _assert_same_bits(g.cpu().numpy(), want, f"fill {fill}")


def test_gather_by_id_refuses_more_than_4096_keys_and_the_next_call_works():
    from vod_amd import _native
    from vod_amd.core.in_batch_negatives import gather_by_id_tensors

    lib = _native.load_library()
    keys = torch.zeros((2, 4097), dtype=torch.int64, device="cuda")
    vals = torch.zeros((2, 4097), device="cuda")
    q = torch.zeros((16,), dtype=torch.int64, device="cuda")
    out = torch.full((2, 16), 7.0, device="cuda")
    status = lib.vodhip_gather_by_id(q.data_ptr(), 16, keys.data_ptr(), 2, 4097, 1, _ptrs([vals]), (ctypes.c_float * 1)(0.0), _ptrs([out]), _stream())
    torch.cuda.synchronize()
    assert status < 0 and bool((out == 7).all()) and "4096" in _last_error()
    with pytest.raises(_native.NativeLibraryError, match="4096"):
        gather_by_id_tensors(q, keys, [vals], [0.0])
    with pytest.raises(ValueError, match="between 1 and 8"):
        gather_by_id_tensors(q, keys[:, :8], [vals[:, :8]] * 9, [0.0] * 9)
    queries, keys_ok, values, fills, want = _gather_case(257, 255, 1)
    got = gather_by_id_tensors(tp._t(queries), tp._t(keys_ok), [tp._t(values[0])], fills)
    _assert_same_bits(got[0].cpu().numpy(), want[0], "next call")


@pytest.mark.parametrize("padding", [True, False])
@pytest.mark.parametrize("B,n,n_raw", [(64, 130, 1),   # 8320 ids: past the one-launch flattening's 8192
                                       (4, 8, 6)])     # scores, labels, log-weights + 6 raw = 9 value arrays: a second gather launch
def test_flatten_samples_through_gather_by_id(B, n, n_raw, padding, monkeypatch):
    _forbid_the_one_launch_path(monkeypatch)
    rng = np.random.default_rng(9600 + B)
    ids = rng.integers(-1, B * n // 3, size=(B, n)).astype(np.int64)
    ids[0, 0], ids[-1, -1] = 1, -1
    labels = rng.random((B, n)) < 0.3
    raw_names = RAW[:n_raw]
    vals = {name: _values(rng, (B, n)) for name in ("scores", "log_weights", *raw_names)}
    _check_flatten_samples(ids, labels, vals, raw_names, padding)


# ---- 3. the sampler with k_total above its 256 threads --------------------------------------------------------------------------------
LARGE_K = [(4096, 257), (4096, 1024), (4096, 4096), (300, 4096), (1000, 1000)]
OLD_KEYS = ("samples", "log_weights", "labels", "lse")


def _large_k_case(tag, width, k_tot, mode, temperature, **kw):
    """old entry point, proposal entry point with every new pointer NULL, and with all of them set: the same old bytes; the proposal
    run against the restatement."""
    scores, labels, noise = tp._rows(width, mode, seed=6, nq=2)
    k_pos = max(1, k_tot // 4)
    null = tp._sample(scores, labels, noise, k_pos, k_tot, temperature=temperature, entry="null", **kw)
    new = tp._sample(scores, labels, noise, k_pos, k_tot, temperature=temperature, entry="proposal", **kw)
    old = tp._sample(scores, labels, noise, k_pos, k_tot, temperature=temperature, entry="old", **kw)
    for key in OLD_KEYS:
        assert tp._same_bytes(old[key], null[key]) and tp._same_bytes(old[key], new[key]), key
    assert all(bool((null[k] == 7).all()) for k in ("log_p", "log_mass", "joint"))
    want = tp._compare(tag, tp._host(new), scores, labels, noise, k_pos, k_tot, temperature=temperature, **kw)
    assert (want["samples"] < 0).any() == (k_tot > width)
    return want


def test_each_instantiation_is_granted_its_lds_at_the_largest_shape():
    """Width 4096 with 4096 samples: 114,784 bytes without the proposal outputs, 131,176 with them - above the 64 KiB a kernel gets
    unasked, and above every grant an earlier test of the suite obtained (k_total <= 128).  `priority_sample_kernel<false>` runs
    first, then `<true>`: each must obtain its own."""
    want = _large_k_case("grant-w4096-k4096", 4096, 4096, "half", 1.0)
    assert (want["samples"] >= 0).all() and want["labels"].sum() > 256 and (~want["labels"]).sum() > 256


@pytest.mark.parametrize("temperature", [1.0, 0.0])
@pytest.mark.parametrize("mode", ["half", "nopos"])
@pytest.mark.parametrize("width,k_tot", LARGE_K)
def test_large_k_total_matches_the_restatement(width, k_tot, mode, temperature):
    """More samples than threads: the selection loops take up to 16 strides and wsel / isel / sel_all / wall hold up to 4096 entries."""
    want = _large_k_case(f"w{width}-k{k_tot}-{mode}-T{temperature:g}", width, k_tot, mode, temperature)
    if mode == "nopos":
        assert not want["labels"].any() and ((want["samples"] >= 0).sum(1) == min(width, k_tot)).all()


@pytest.mark.parametrize("keep_top", [False, True])
def test_large_k_total_with_a_truncated_support(keep_top):
    """Each stratum of a 4096-wide "half" row has ~2048 members: max_support 1500 truncates both, and 1024 samples are drawn."""
    scores, labels, _ = tp._rows(4096, "half", seed=6, nq=2)
    assert (labels.sum(1) > 1500).all() and ((~labels).sum(1) > 1500).all()
    _large_k_case(f"w4096-k1024-support1500-{'keep' if keep_top else 'ref'}", 4096, 1024, "half", 1.0, max_support=1500, keep_top=keep_top)


# ---- 4. exactly tied keys -----------------------------------------------------------------------------------------------------------
MIN_GAP = 1e-3   # distinct keys are at least this far apart in float64: ~1000 times what float32 exp / log can move a key of size <= 20


@functools.lru_cache(maxsize=None)
def _tie_rows(width, mode, p_inf, seed, nq=4):
    """Integer scores in [-4, 4] and noise in {0.5, 1, 2}: few distinct keys, so many exact ties - what merged rows look like, where a
    section an engine did not return carries that engine's minimum score.  Two keys of a stratum differ by d_score - d_j * ln 2 with
    integers |d_score| <= 8, |d_j| <= 2: zero or at least 0.3."""
    rng = np.random.default_rng(9700 + 17 * width + seed)
    scores = rng.integers(-4, 5, size=(nq, width)).astype(np.float32)
    scores[rng.uniform(size=scores.shape) < p_inf] = -np.inf
    labels = rng.uniform(size=scores.shape) < {"mixed": 0.08, "half": 0.5, "nopos": 0.0}[mode]
    if mode == "mixed":
        labels[:, 0], labels[:, 1] = True, False
    noise = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=scores.shape)
    for a in (scores, labels, noise):
        a.setflags(write=False)
    return scores, labels, noise


def _keys64(score, noise, temperature, max_support=-1, keep_top=False):
    """The float64 priority keys of one stratum (the formulas of tests/proposal_ref.py)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        log_p, _ = proposal_ref._log_softmax(proposal_ref._scaled(score, temperature, max_support, keep_top, np.float64), np.float64)
        return log_p - np.log(noise.astype(np.float64)) if temperature > 0 else log_p


def _tie_report(scores, labels, noise, want, temperature, **kw):
    """On the float64 restatement alone -> (smallest gap between two DISTINCT keys of a stratum, number of strata with two equal keys
    among the slots 0 ... k: the selected ones and the threshold's)."""
    gap, tied = np.inf, 0
    for r in range(scores.shape[0]):
        for cls in (True, False):
            members = np.flatnonzero(labels[r] == cls)
            key = _keys64(scores[r][members], noise[r][members], temperature, **kw)
            key = np.sort(key[~np.isnan(key)])[::-1]  # (a stratum without mass has NaN keys only: its order is the column order)
            n_sel = int(((want["samples"][r] >= 0) & (want["labels"][r] == cls)).sum())
            head = key[: n_sel + 1]
            with np.errstate(invalid="ignore"):
                d = -np.diff(key)  # (-inf) - (-inf) = NaN: equal
                dh = -np.diff(head)
            tied += bool(len(dh) and (np.isnan(dh) | (dh == 0)).any())
            d = d[~np.isnan(d) & (d != 0)]
            if len(d):
                gap = min(gap, d.min())
    return gap, tied


# seeds chosen on the CPU so that every case below has a tie among its selected slots or at slot k (asserted in the test)
TIE_SEEDS = {(40, "half", 0.8, 1.0, 4): 1}


@pytest.mark.parametrize("k_tot", [4, 32])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("p_inf", [0.0, 0.8])
@pytest.mark.parametrize("mode", ["mixed", "half"])
@pytest.mark.parametrize("width", [40, 65, 300, 1000])
def test_exactly_tied_keys_go_to_the_smaller_column(width, mode, p_inf, temperature, k_tot):
    """One-wave path (a class of <= 64 members) and LDS path: among equal keys the smaller column is selected first, and the
    threshold at slot k is the next one.  `samples` is the restatement's (a stable argsort) in EVERY slot, -inf weights included."""
    seed = TIE_SEEDS.get((width, mode, p_inf, temperature, k_tot), 0)
    scores, labels, noise = _tie_rows(width, mode, p_inf, seed)
    k_pos = 2 if k_tot == 4 else 8
    want = proposal_ref.sample(scores, labels, noise, k_pos, k_tot, temperature=temperature)
    gap, tied = _tie_report(scores, labels, noise, want, temperature)
    assert gap >= MIN_GAP, f"two distinct keys {gap:.3e} apart: device rounding could reorder them"
    assert tied >= 1, "no tie among the selected slots or at slot k: the case would not exercise the rule"
    got = tp._host(tp._sample(scores, labels, noise, k_pos, k_tot, temperature=temperature))
    np.testing.assert_array_equal(got["samples"], want["samples"])
    tp._compare(f"ties-w{width}-{mode}-inf{p_inf:g}-T{temperature:g}-k{k_tot}", got, scores, labels, noise, k_pos, k_tot, temperature=temperature)


RUN_SEEDS = {300: 0, 1000: 1, 65: 0}  # chosen on the CPU for the property the test asserts first


@pytest.mark.parametrize("keep_top", [False, True])
@pytest.mark.parametrize("width,mode,max_support,k_tot", [(300, "nopos", 40, 64), (1000, "half", 100, 32), (65, "half", 10, 16)])
def test_support_threshold_inside_a_run_of_equal_scores(width, mode, max_support, k_tot, keep_top):
    """The max_support-th largest score of a stratum lies inside a run of equal scores.  The reference mode masks everything >= it,
    the whole run; `keep_top` masks everything below it and so KEEPS the whole run: more than max_support entries stay."""
    scores, labels, noise = _tie_rows(width, mode, 0.0, RUN_SEEDS[width])
    for r in range(scores.shape[0]):  # in every row the run of the threshold's value reaches past rank max_support among the negatives
        s = np.sort(scores[r][~labels[r]])[::-1]
        assert len(s) > max_support and s[max_support] == s[max_support - 1] > s[-1]
    kw = dict(temperature=1.0, max_support=max_support, keep_top=keep_top)
    want = proposal_ref.sample(scores, labels, noise, 4, k_tot, **kw)
    gap, _ = _tie_report(scores, labels, noise, want, 1.0, max_support=max_support, keep_top=keep_top)
    assert gap >= MIN_GAP
    got = tp._host(tp._sample(scores, labels, noise, 4, k_tot, **kw))
    np.testing.assert_array_equal(got["samples"], want["samples"])
    tp._compare(f"run-w{width}-{mode}-support{max_support}-{'keep' if keep_top else 'ref'}", got, scores, labels, noise, 4, k_tot, **kw)
    if keep_top:  # log_mass is the log-sum-exp over the kept support: the WHOLE run of the threshold's value, not max_support entries
        for r in range(scores.shape[0]):
            neg = np.sort(scores[r][~labels[r]].astype(np.float64))[::-1]
            kept = neg[neg >= neg[max_support - 1]]
            assert len(kept) > max_support
            mass, cut = np.log(np.exp(kept).sum()), np.log(np.exp(neg[:max_support]).sum())
            assert abs(got["log_mass"][r, 1] - mass) <= 1e-4 < mass - cut
