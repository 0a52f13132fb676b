"""Listed section ids (`ids` of SearchClient.search) above the kernels: the restatement's own edge cases, the routing inside
`Endpoints`, the section-id map, the wire format of the client and the dense lookup of the hybrid search - none of it needs a GPU
(tests/test_score_ids_gpu.py and tests/test_score_ids_server_gpu.py run the kernels and the real server)."""
import pickle

import numpy as np
import pytest

import score_ids_ref as R
from vod_amd import io as vio
from vod_amd import types as vt


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_restatement_aligned_form_edge_cases():
    x = np.array([[1, 0], [0, 2], [3, 3], [np.nan, 1]], dtype=np.float32)
    q = np.array([[1, 1], [2, -1]], dtype=np.float32)
    ids = np.array([[0, -1, 2, 4, 2, 1 << 33], [3, 1, 1, 0, -5, 2]], dtype=np.int64)
    got = R.score_ids_aligned(q, x, ids)
    ninf = -np.inf
    np.testing.assert_array_equal(got[0], [1, ninf, 6, ninf, 6, ninf])  # empty, id = ntotal, beyond 2^32: absent; a duplicate scores twice
    assert np.isnan(got[1, 0]) and got[1, 1:].tolist() == [-2, -2, 2, ninf, 3]
    # id_base: ids below it and at id_base + ntotal are absent
    got = R.score_ids_aligned(q[:1], x[:3], np.array([[999, 1000, 1002, 1003]]), id_base=1000)
    np.testing.assert_array_equal(got, [[ninf, 1, 6, ninf]])
    # labels: a foreign label hides the row, all -1 is unrestricted, an unknown label (-2) restricts to nothing
    lab = np.array([0, 1, 0, 1], dtype=np.int32)
    ql = np.array([[1, -1], [-1, -1], [-2, -1]], dtype=np.int32)
    got = R.score_ids_aligned(np.ones((3, 2), np.float32), x[:3], np.array([[0, 1, 2]] * 3), row_labels=lab[:3], q_labels=ql)
    np.testing.assert_array_equal(got, [[ninf, 2, ninf], [1, 2, 6], [ninf, ninf, ninf]])


def test_restatement_topk_form_edge_cases():
    ninf = -np.inf
    aligned = np.array([[5.0, ninf, 7.0, 5.0, 7.0, np.nan, 5.0], [ninf] * 7], dtype=np.float64)
    ids = np.array([[9, -1, 4, 2, 4, 8, 9], [-1] * 7], dtype=np.int64)
    s, i = R.score_ids_topk(aligned, ids, 5)
    np.testing.assert_array_equal(i, [[4, 2, 9, -1, -1], [-1] * 5])  # a listed id counts once; equal scores by id; NaN never enters
    np.testing.assert_array_equal(s, [[7, 5, 5, ninf, ninf], [ninf] * 5])
    s, i = R.score_ids_topk(aligned, ids, 2)
    np.testing.assert_array_equal(i, [[4, 2], [-1, -1]])
    np.testing.assert_array_equal(R.es_labels(s), [[1, 1], [0, 0]])


# ---- Endpoints -----------------------------------------------------------------------------------------------------------------
class _ListedEngine:
    """records what reaches `search_listed`; a scan (`search`) must never run for a listed request"""

    ntotal = 100

    def __init__(self, section_rows=None):
        self.section_rows = section_rows
        self.calls = []

    def search(self, q, k):
        raise AssertionError("a listed request went to the scan path")

    def encode_subset(self, subset_ids):
        return np.array([[{"a": 0, "b": 1}.get(s[0], -2) if s else -1] for s in subset_ids], dtype=np.int32)

    def search_listed(self, q, k, rows, subset=None):
        self.calls.append((np.array(q), k, np.array(rows), None if subset is None else np.array(subset)))
        return R.score_ids_topk(np.where(rows >= 0, rows.astype(np.float64), -np.inf), rows, k)  # score of row r = r


def _fast_search(endpoints, q, **extra):
    import json

    status, _, payload, _ = endpoints.handle("POST", "/fast-search", {}, bytes(vio.json_body_with_arrays({"vectors": q}, extra)))
    doc = json.loads(bytes(payload))
    if status != 200:
        return status, doc
    return status, (vio.deserialize_np_array(doc["scores"]), vio.deserialize_np_array(doc["indices"]))


def test_endpoints_route_listed_requests_to_the_engine_not_the_batcher():
    from vod_amd.search.server import Endpoints

    engine = _ListedEngine()
    ep = Endpoints(engine)
    q = np.ones((4, 8), dtype=np.float32)
    status, (s, i) = _fast_search(ep, q, top_k=3, ids=[["7", "5", "7", "9"], [], ["nope", "-3", "1.5", "12"], ["2"]])
    assert status == 200 and ep.batcher is None and not ep._generic  # no batcher was built, let alone used
    (got_q, k, rows, subset), = engine.calls
    np.testing.assert_array_equal(got_q, q)
    assert k == 3 and subset is None and rows.dtype == np.int64
    # ragged lists are padded with -1; `[]` lists nothing; unknown / unparsable / negative ids match nothing
    np.testing.assert_array_equal(rows, [[7, 5, 7, 9], [-1, -1, -1, -1], [-1, -1, -1, 12], [2, -1, -1, -1]])
    np.testing.assert_array_equal(i, [[9, 7, 5], [-1, -1, -1], [12, -1, -1], [2, -1, -1]])
    assert np.isneginf(s[1]).all() and s.dtype == np.float32 and i.dtype == np.int64
    # a batch whose lists are all empty is still a listed request: nobody is a hit
    status, (s, i) = _fast_search(ep, q[:2], top_k=2, ids=[[], []])
    assert status == 200 and (i == -1).all() and engine.calls[-1][2].shape == (2, 1)
    # ids AND subset_ids: both reach the engine
    status, _ = _fast_search(ep, q[:2], top_k=2, ids=[["1"], ["2"]], subset_ids=[["b"], ["zzz"]])
    assert status == 200
    np.testing.assert_array_equal(engine.calls[-1][3], [[1], [-2]])
    ep.close()


def test_endpoints_listed_request_errors_are_http_500_with_detail():
    from vod_amd.search.server import Endpoints, GroupHipEngine

    ep = Endpoints(_ListedEngine())
    q = np.ones((3, 8), dtype=np.float32)
    status, doc = _fast_search(ep, q, top_k=2, ids=[["1"], ["2"]])
    assert status == 500 and "`ids` must have one list per query" in doc["detail"]
    status, doc = _fast_search(ep, q, top_k=2, ids="7")
    assert status == 422  # not a list of lists: the pydantic model refuses the document

    class _ScanOnly:
        ntotal = 5

        def search(self, q, k):
            raise AssertionError("not reached")

    status, doc = _fast_search(Endpoints(_ScanOnly()), q, top_k=2, ids=[["1"]] * 3)
    assert status == 500 and "this engine cannot score listed ids" in doc["detail"]
    group = GroupHipEngine.__new__(GroupHipEngine)  # the multi-process group: a clear error, no GPU needed to say it
    with pytest.raises(ValueError, match="this engine cannot score listed ids"):
        group.search_listed(q, 2, np.zeros((3, 1), np.int64))


def test_section_id_map(tmp_path):
    from vod_amd.search.server import Endpoints, encode_listed_ids, load_section_rows

    np.save(tmp_path / "ids.npy", np.array(["s-10", "s-11", "7", "s-13"]))
    rows = load_section_rows(tmp_path / "ids.npy", 4)
    assert rows == {"s-10": 0, "s-11": 1, "7": 2, "s-13": 3}
    np.testing.assert_array_equal(encode_listed_ids([["s-13", "7", "3"], []], rows), [[3, 2, -1], [-1, -1, -1]])  # "3" is no section id
    np.testing.assert_array_equal(encode_listed_ids([["s-13", "7", "3"]], None), [[-1, 7, 3]])  # without a map: decimal row numbers
    with pytest.raises(ValueError, match="4 section ids for 5 vectors"):
        load_section_rows(tmp_path / "ids.npy", 5)
    np.save(tmp_path / "dup.npy", np.array(["a", "b", "a", "c", "b"]))
    with pytest.raises(ValueError, match="section ids must be unique, 2 are not"):
        load_section_rows(tmp_path / "dup.npy", 5)
    engine = _ListedEngine(rows)
    status, (_, i) = _fast_search(Endpoints(engine), np.ones((1, 8), np.float32), top_k=4, ids=[["7", "s-10", "8"]])
    assert status == 200 and i.tolist() == [[2, 0, -1, -1]]


def test_native_front_hands_listed_requests_to_the_endpoints():
    """libvodhip's HTTP front answers the plain hot document itself; one that carries `ids` is not plain: it reaches `Endpoints`"""
    import ctypes

    from vod_amd import _native
    from vod_amd.search.client import HipMipsClient
    from vod_amd.search.native import NativeHttpFront
    from vod_amd.search.server import Endpoints

    lib = _native.load_library()
    q = np.ones((2, 8), dtype=np.float32)
    vb, ve, tk = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    plain = bytes(vio.json_body_with_arrays({"vectors": q}, {"top_k": 4}))
    listed = bytes(vio.json_body_with_arrays({"vectors": q}, {"top_k": 4, "ids": [["1"], []]}))
    assert lib.vodhip_wire_parse_fast_search(plain, len(plain), ctypes.byref(vb), ctypes.byref(ve), ctypes.byref(tk)) == 0
    assert lib.vodhip_wire_parse_fast_search(listed, len(listed), ctypes.byref(vb), ctypes.byref(ve), ctypes.byref(tk)) == 1

    class _Engine(_ListedEngine):
        def search(self, q, k):
            return np.zeros((len(q), k), np.float32), np.tile(np.arange(k, dtype=np.int64), (len(q), 1))

    engine = _Engine()
    endpoints = Endpoints(engine)
    endpoints.batcher = endpoints._batcher_for(8)
    front = NativeHttpFront(endpoints.batcher, endpoints)
    port = front.listen("127.0.0.1", 0, None)
    front.start()
    try:
        client = HipMipsClient(host="http://127.0.0.1", port=port, forward_ids=True)
        res = client.search(vector=q, ids=[[5, 3, 5], []], top_k=4)  # (section ids of any type travel as strings)
        np.testing.assert_array_equal(res.indices, [[5, 3, -1, -1], [-1] * 4])
        np.testing.assert_array_equal(res.labels, [[1, 1, 0, 0], [0] * 4])
        np.testing.assert_array_equal(engine.calls[-1][2], [[5, 3, 5], [-1, -1, -1]])
        before = front.get_stat("requests_native")
        assert front.get_stat("requests_fallback") == 1
        plain_res = client.search(vector=q, top_k=4)  # no `ids`: the same connection, the native hot path, no labels
        assert plain_res.labels is None and plain_res.indices.tolist() == [[0, 1, 2, 3]] * 2 and len(engine.calls) == 1
        assert front.get_stat("requests_native") == before + 1 and front.get_stat("requests_fallback") == 1
    finally:
        front.close()
        endpoints.close()


# ---- the client ----------------------------------------------------------------------------------------------------------------
def _capture(client, monkeypatch, scores, indices):
    sent = []

    def post(path, body, content_type, timeout):
        sent.append((path, bytes(body)))
        return 200, {}, bytes(vio.json_body_with_arrays({"scores": scores, "indices": indices}))

    monkeypatch.setattr(client, "_post", post)
    return sent


def test_client_forward_ids_wire_format_and_labels(monkeypatch):
    from vod_amd.search.client import HipMipsClient

    q = np.arange(16, dtype=np.float32).reshape(2, 8)
    scores = np.array([[3.0, -np.inf], [-np.inf, -np.inf]], dtype=np.float32)
    indices = np.array([[12, -1], [-1, -1]], dtype=np.int64)
    ids = [["s12", "s9"], []]
    today = bytes(vio.json_body_with_arrays({"vectors": q}, {"top_k": 2}))
    # off (the default): `ids` is dropped as the reference's faiss client drops it - the bytes on the wire are today's
    off = HipMipsClient(port=1, native=False)
    assert off.forward_ids is False
    sent = _capture(off, monkeypatch, scores, indices)
    res = off.search(vector=q, ids=ids, top_k=2)
    assert sent == [("/fast-search", today)] and res.labels is None
    # on: the document carries `ids`, the result the Elasticsearch client's labels; without `ids` nothing changes
    on = HipMipsClient(port=1, native=False, forward_ids=True)
    sent = _capture(on, monkeypatch, scores, indices)
    res = on.search(vector=q, ids=ids, top_k=2)
    import json

    doc = json.loads(sent[0][1])
    assert doc["ids"] == ids and doc["top_k"] == 2 and set(doc) == {"vectors", "top_k", "ids"}
    np.testing.assert_array_equal(res.labels, [[1, 0], [0, 0]])
    assert res.labels.dtype == np.int64
    np.testing.assert_array_equal(res.indices, indices)
    res = on.search(vector=q, top_k=2)
    assert sent[1] == ("/fast-search", today) and res.labels is None
    # a listed request never takes the binary or the native transport (neither carries the field)
    for kw in ({"binary": True}, {"native": True}):
        c = HipMipsClient(port=1, forward_ids=True, **kw)
        sent = _capture(c, monkeypatch, scores, indices)
        c.search(vector=q, ids=ids, top_k=2)
        assert sent[0][0] == "/fast-search" and json.loads(sent[0][1])["ids"] == ids


def test_client_pickles_with_and_without_the_new_attribute():
    from vod_amd.search.client import HipMipsClient

    c = pickle.loads(pickle.dumps(HipMipsClient(port=5, forward_ids=True)))
    assert c.forward_ids is True and c.port == 5
    state = HipMipsClient(port=5).__getstate__()
    state.pop("forward_ids")  # a pickle written before the attribute existed
    old = HipMipsClient.__new__(HipMipsClient)
    old.__setstate__(state)
    assert old.forward_ids is False and old.forward_subset_ids is False


def test_master_passes_the_id_files_to_the_server(tmp_path):
    from vod_amd.search.client import HipMipsMaster

    cmd = HipMipsMaster(tmp_path / "v.npy", port=7001, skip_setup=True, section_ids_path=tmp_path / "s.npy")._make_cmd()
    assert cmd[cmd.index("--section-ids-path") + 1] == str(tmp_path / "s.npy") and "--subset-ids-path" not in cmd
    assert "--section-ids-path" not in HipMipsMaster(tmp_path / "v.npy", port=7001, skip_setup=True)._make_cmd()


# ---- the hybrid search's lookup on the dense engine -----------------------------------------------------------------------------
def test_hybrid_search_looks_the_gold_sections_up_on_the_dense_client(monkeypatch):
    """`async_hybrid_search` prepends a lookup request (`text = ""`, `ids = section_ids`) to `clients[lookup_engine_name]`; with a
    client that honours `ids` that engine may be the dense one.  The merge kernel is replaced by a stand-in that keeps what this test
    is about - which result is the lookup's and that its labels lead the merged batch (tests/test_score_ids_server_gpu.py runs the
    real merge end to end)."""
    from vod_amd.core import merge as vmerge
    from vod_amd.core import search as vsearch

    seen = []

    class _Dense:
        def search(self, *, vector, text=None, subset_ids=None, ids=None, shard=None, top_k=3):
            seen.append({"text": text, "ids": ids})
            if ids is None:  # the scan: rows 0 .. top_k-1
                return vt.RetrievalBatch(scores=np.tile(np.arange(top_k, 0, -1, dtype=np.float32), (len(vector), 1)),
                                         indices=np.tile(np.arange(top_k, dtype=np.int64), (len(vector), 1)), labels=None, meta={})
            rows = np.array([[int(s) for s in r] + [-1] * (top_k - len(r)) for r in ids], dtype=np.int64)
            scores = np.where(rows >= 0, 1.0, -np.inf).astype(np.float32)
            return vt.RetrievalBatch(scores=scores, indices=rows, labels=R.es_labels(scores), meta={})

        async def async_search(self, **kw):
            return self.search(**kw)

    def fake_merge(lookup_idx, lookup_lbl, engines, weights, device=0):
        (name, (idx, scr)), = engines.items()
        return (np.concatenate([lookup_idx, idx], 1), np.concatenate([np.zeros_like(lookup_idx, dtype=np.float32), scr], 1),
                np.concatenate([lookup_lbl, np.full_like(idx, -1)], 1), {name: scr})

    monkeypatch.setattr(vmerge, "merge_hybrid", fake_merge)
    merged, raw = vsearch.async_hybrid_search(text=["q0", "q1"], shards=["s", "s"], vector=np.zeros((2, 4), np.float32),
                                              section_ids=[["41", "7"], []], top_k=3, clients={"dense": _Dense()},
                                              weights={"dense": 1.0}, lookup_engine_name="dense")
    assert seen[0] == {"text": ["", ""], "ids": [["41", "7"], []]} and seen[1] == {"text": ["q0", "q1"], "ids": None}
    np.testing.assert_array_equal(merged.indices[:, :3], [[41, 7, -1], [-1, -1, -1]])
    np.testing.assert_array_equal(merged.labels[:, :3], [[1, 1, 0], [0, 0, 0]])  # the gold labels, from the dense engine
    assert set(raw) == {"dense"}
