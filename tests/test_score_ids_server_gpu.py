"""Listed section ids end to end: the real server process behind libvodhip's native HTTP front (the default), started with
`--section-ids-path` and `--subset-ids-path` on a 5000 x 64 store, queried by a `forward_ids=True` client - hits and labels against
the restatement of tests/score_ids_ref.py - and the hybrid search with its gold-section lookup on the dense engine."""
import numpy as np
import pytest

import score_ids_ref as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_server_honours_ids_and_the_dense_engine_serves_the_lookup(tmp_path, monkeypatch):
    import requests

    from oracle.flat_ip import flat_ip_topk
    from vod_amd import store
    from vod_amd.core import search as vsearch
    from vod_amd.search.client import HipMipsClient, HipMipsMaster

    monkeypatch.chdir(tmp_path)  # the master writes its logs into the cwd
    rng = np.random.default_rng(7)
    n, d, nq, k = 5000, 64, 8, 6
    x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    q = rng.integers(-8, 9, size=(nq, d)).astype(np.float32)
    sections = np.array([f"sec-{(r * 7919) % n}" for r in range(n)])  # unique, and not the row number
    row_of = {s: r for r, s in enumerate(sections)}
    subsets = np.array([f"doc{r % 4}" for r in range(n)])
    store.save_vectors(tmp_path / "v.npy", x, dtype=np.float16)
    np.save(tmp_path / "sections.npy", sections)
    np.save(tmp_path / "subsets.npy", subsets)

    listed_rows = [rng.choice(n, size=20, replace=False).tolist() for _ in range(nq)]
    ids = [[str(sections[r]) for r in rows] for rows in listed_rows]
    ids[1] = []                                    # lists nothing: no hit
    ids[2] = ["sec-none", "12", ids[2][0]]         # unknown ids ("12" is a row number, not a section id) match nothing
    ids[3] = ids[3][:3] * 2                        # a listed id counts once
    ids[4] = ids[4][:2]                            # fewer ids than top_k: pads
    rows = np.full((nq, 20), -1, dtype=np.int64)
    for i, names in enumerate(ids):
        rows[i, : len(names)] = [row_of.get(s, -1) for s in names]

    with HipMipsMaster(tmp_path / "v.npy", port=-1, logging_level="warning", section_ids_path=tmp_path / "sections.npy",
                       subset_ids_path=tmp_path / "subsets.npy") as m:
        c = HipMipsClient(host=m.host, port=m.port, forward_ids=True, forward_subset_ids=True)
        res = c.search(vector=q, ids=ids, top_k=k)
        aligned = R.score_ids_aligned(q, x, rows)
        rs, ri = R.score_ids_topk(aligned, rows, k)
        np.testing.assert_array_equal(res.indices, ri)
        np.testing.assert_array_equal(res.scores.astype(np.float64), rs)
        np.testing.assert_array_equal(res.labels, R.es_labels(rs))
        assert (res.indices[1] == -1).all() and (res.labels[1] == 0).all() and np.isneginf(res.scores[1]).all()
        assert res.indices[2].tolist() == [rows[2, 2]] + [-1] * (k - 1)
        assert (res.indices[3] >= 0).sum() == 3 and (res.indices[4] >= 0).sum() == 2
        # ids AND subset_ids
        subset_ids = [["doc1", "doc3"] if i % 2 else [] for i in range(nq)]
        subset_ids[6] = ["nope"]
        both = c.search(vector=q, ids=ids, subset_ids=subset_ids, top_k=k)
        vocab = {f"doc{j}": j for j in range(4)}
        q_labels = np.array([[vocab.get(s, -2) for s in names] + [-1] * (2 - len(names)) for names in subset_ids], dtype=np.int32)
        row_labels = (np.arange(n) % 4).astype(np.int32)
        bs, bi = R.score_ids_topk(R.score_ids_aligned(q, x, rows, row_labels=row_labels, q_labels=q_labels), rows, k)
        np.testing.assert_array_equal(both.indices, bi)
        np.testing.assert_array_equal(both.scores.astype(np.float64), bs)
        assert (both.indices[6] == -1).all() and not np.array_equal(bi, ri)
        # a plain request on the same connection: the native hot path, unchanged
        stats = lambda: requests.get(f"{m.host}:{m.port}/stats", timeout=30).json()  # noqa: E731
        before = stats()
        plain = c.search(vector=q, top_k=k)
        ps, pi = flat_ip_topk(q, x, k)
        np.testing.assert_array_equal(plain.indices, pi)
        np.testing.assert_array_equal(plain.scores, ps)
        assert plain.labels is None
        after = stats()
        assert after["requests_native"] == before["requests_native"] + 1 and after["requests_fallback"] == before["requests_fallback"]
        assert before["requests_fallback"] >= 2  # the two listed requests above went to the host's handler
        # a client that does not forward `ids` gets today's answer
        np.testing.assert_array_equal(m.get_client().search(vector=q, ids=ids, top_k=k).indices, pi)
        # the gold-section lookup of the hybrid search on the dense engine: no other engine needed
        gold = [[str(sections[r]) for r in rows_i[:2]] for rows_i in listed_rows]
        merged, raw = vsearch.async_hybrid_search(text=["q"] * nq, shards=["s"] * nq, vector=q, section_ids=gold, top_k=k,
                                                  clients={"dense": c}, weights={"dense": 1.0}, lookup_engine_name="dense")
        assert set(raw) == {"dense"}
        for i in range(nq):
            want = {row_of[s] for s in gold[i]}
            got = {int(r) for r, lab in zip(merged.indices[i], merged.labels[i]) if lab > 0}
            assert got == want, (i, got, want)  # exactly the gold sections carry a positive label in the merged batch
            assert set(pi[i].tolist()) <= set(merged.indices[i].tolist())  # next to the dense engine's own hits
