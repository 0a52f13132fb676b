"""The survivor rings of the 8-phase FILTER kernel (kernels_mips_8phase.hip): each wave stores the 32 sums of a query block that holds
a survivor to a ring in the workspace and turns them into candidates after its last tile.  A block that no longer fits into the ring
takes the in-loop path.  Either way the candidate lists receive the same (key, query) multiset, so results are bit-identical to the
oracle on integer-valued data (every partial sum exact in fp32) and do not depend on the ring size ("survivor_ring").
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _index(x, **params):
    from vod_amd.index import HipFlatIndex

    ix = HipFlatIndex(x.shape[1], len(x), dtype=torch.float16, device=0)
    ix.add(x)
    # every FILTER stage on the 8-phase kernel, however short (auto: stages of less than one tile per CU run the 128x128 kernel)
    ix.set_param("small_chunk_tiles", 0)
    for k, v in params.items():
        ix.set_param(k, v)
    return ix


def _int_data(seed, n, d, nq):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 9, size=(nq, d)).astype(np.float16), rng.integers(-8, 9, size=(n, d)).astype(np.float16)


def _clustered_int(seed, n, d, nq, n_clusters=64):
    """rows sorted by topic cluster, queries aimed at the LAST clusters: many survivors in few tiles, i.e. in few waves' rings"""
    rng = np.random.default_rng(seed)
    centers = rng.integers(-6, 7, size=(n_clusters, d))
    lab = np.sort(rng.integers(0, n_clusters, size=n))
    x = np.clip(centers[lab] + rng.integers(-2, 3, size=(n, d)), -8, 8).astype(np.float16)
    ql = rng.integers(n_clusters - 4, n_clusters, size=nq)
    q = np.clip(centers[ql] + rng.integers(-2, 3, size=(nq, d)), -8, 8).astype(np.float16)
    return q, x


def _search(ix, q, k):
    s, i = ix.search(torch.from_numpy(q).cuda(), k)
    return s.cpu().numpy(), i.cpu().numpy()


def _oracle(q, x, k):
    from oracle.flat_ip import flat_ip_topk

    return flat_ip_topk(q, x, k)


@pytest.mark.parametrize("nq", [256, 1024])  # one and four query tiles
def test_auto_kernel_bit_exact_with_the_ring(nq):
    q, x = _int_data(11, 120_000, 96, nq)
    k = 50
    with _index(x) as ix:
        s, i = _search(ix, q, k)
        assert ix.get_stat("last_survivor_ring") > 0  # the search planned rings: its FILTER stages run the 8-phase kernel
    rs, ri = _oracle(q, x, k)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)


@pytest.mark.parametrize("ring", [1, 4])
def test_full_rings_fall_back_bit_identically(ring):
    q, x = _int_data(12, 120_000, 96, 1024)
    k = 100
    with _index(x) as ix:
        s0, i0 = _search(ix, q, k)
        ix.set_param("survivor_ring", ring)
        s1, i1 = _search(ix, q, k)
        assert ix.get_stat("last_survivor_ring") == ring
        assert ix.get_stat("last_ring_fallbacks") > 0  # the rings filled up: blocks went through the in-loop path
    np.testing.assert_array_equal(i1, i0)
    np.testing.assert_array_equal(s1, s0)
    rs, ri = _oracle(q, x, k)
    np.testing.assert_array_equal(i0, ri)
    np.testing.assert_array_equal(s0, rs)


@pytest.mark.parametrize("ring", [0, 4])
def test_clustered_rows_fill_single_waves(ring):
    q, x = _clustered_int(13, 150_000, 64, 512)
    k = 100
    with _index(x, survivor_ring=ring, tile_order=1) as ix:  # row order: a late cluster's tiles all in the last stage
        s, i = _search(ix, q, k)
    rs, ri = _oracle(q, x, k)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)


@pytest.mark.parametrize("nq", [256, 1024])
def test_repeated_auto_searches_are_bit_identical(nq):
    rng = np.random.default_rng(14)
    x = rng.standard_normal((200_000, 128)).astype(np.float16)
    q = rng.standard_normal((nq, 128)).astype(np.float16)
    with _index(x, small_chunk_tiles=256) as ix:  # the library's defaults
        ref = _search(ix, q, 100)
        for _ in range(3):
            s, i = _search(ix, q, 100)
            np.testing.assert_array_equal(i, ref[1])
            np.testing.assert_array_equal(s, ref[0])
            # every block with survivors went through the rings and their drain (the planned size holds i.i.d. data)
            assert ix.get_stat("last_survivor_ring") > 0 and ix.get_stat("last_ring_fallbacks") == 0


def test_ring_absent_every_block_takes_the_in_loop_path():
    # survivor_ring forced to 1 on a batch whose blocks mostly hold several hit lanes: almost nothing fits, the result is the same
    rng = np.random.default_rng(15)
    x = rng.standard_normal((200_000, 128)).astype(np.float16)
    q = rng.standard_normal((1024, 128)).astype(np.float16)
    with _index(x) as ix:
        ref = _search(ix, q, 100)
        assert ix.get_stat("last_ring_fallbacks") == 0
        ix.set_param("survivor_ring", 1)
        s, i = _search(ix, q, 100)
        assert ix.get_stat("last_ring_fallbacks") > 0
    np.testing.assert_array_equal(i, ref[1])
    np.testing.assert_array_equal(s, ref[0])
