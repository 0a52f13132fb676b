"""`--metric l2` end to end: the real server process behind libvodhip's native HTTP front on a 3000 x 64 vector file; `HipMipsClient.search`
returns the ids and squared distances of the float64 restatement (tests/l2_ref.py) through the native hot path - the front and the
batcher call `vodhip_index_search` and know nothing of the metric - and a request that lists `ids` is answered HTTP 500 with the
library's message."""
import numpy as np
import pytest

import l2_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_server_serves_l2_through_the_native_front(tmp_path, monkeypatch):
    import requests

    from vod_amd import store
    from vod_amd.search.client import HipMipsClient, HipMipsMaster

    monkeypatch.chdir(tmp_path)  # the master writes its logs into the cwd
    rng = np.random.default_rng(17)
    n, d, nq, k = 3000, 64, 9, 12
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    q[0] = x[41]  # a stored row: distance 0
    store.save_vectors(tmp_path / "v.npy", x, dtype=np.float16)
    rd, ri = R.l2_topk(q, x, k, R.F16)
    with HipMipsMaster(tmp_path / "v.npy", port=-1, logging_level="warning", metric="l2") as m:
        assert "--metric" in m._make_cmd()
        stats = lambda: requests.get(f"{m.host}:{m.port}/stats", timeout=30).json()  # noqa: E731
        before = stats()
        res = m.get_client().search(vector=q, top_k=k)
        np.testing.assert_array_equal(res.indices, ri)
        np.testing.assert_array_equal(np.asarray(res.scores, dtype=np.float64), rd)
        assert res.scores[0, 0] == 0.0 and res.indices[0, 0] == 41
        after = stats()
        assert after["requests_native"] == before["requests_native"] + 1 and after["requests_fallback"] == before["requests_fallback"]
        # listed ids: refused by the library, HTTP 500 with its message
        c = HipMipsClient(host=m.host, port=m.port, forward_ids=True)
        with pytest.raises(requests.exceptions.HTTPError, match="500"):
            c.search(vector=q, ids=[["1", "2"]] * nq, top_k=k)
        from vod_amd import io as vio

        reply = requests.post(f"{m.host}:{m.port}/fast-search", timeout=30,
                              json={"vectors": vio.serialize_np_array(q), "top_k": k, "ids": [["1", "2"]] * nq})
        assert reply.status_code == 500 and "listed ids are not supported on an L2 index" in reply.json()["detail"]
        np.testing.assert_array_equal(m.get_client().search(vector=q, top_k=k).indices, ri)  # and the server keeps serving
