"""`sum_ids` / `listed_scores`, the parts that need no GPU:

* the float64 restatement (tests/sum_ids_ref.py) on hand-made inputs: presence, the zero-weight skip, NaN / inf weights and rows;
* its derived bound holds for float32 sums of the same terms taken in several orders and chunkings (the kernel's among them), each
  product fused into its add - and is not met by a sum that drops a term;
* ragged ids and weights are padded with -1 and 0;
* the autograd wiring of `listed_scores` through a NumPy stand-in index: forward = `score_ids`, backward = `sum_ids(ids, g)`, NaN
  upstream gradients at -inf slots give a finite gradient, dtype and device of the gradient, once-differentiable;
* both new symbols are listed in `_native.SIGNATURES` with the argument counts of the header and exported by the library (the header
  itself is enumerated by tests/test_host_logic.py and compiled as C99 by tests/test_c_abi.py).
"""
import ctypes

import numpy as np
import pytest

import score_ids_ref as S
import sum_ids_ref as R


# ---- the restatement -----------------------------------------------------------------------------------------------------------
def test_restatement_presence_zero_weights_and_non_finite_values():
    x = np.array([[1, 2], [3, 4], [np.nan, 5], [7, 8]], dtype=np.float32)
    nan, inf = np.nan, np.inf
    ids = np.array([[0, 1, -1, 4, 1 << 33, 1], [2, 3, 3, -1, -1, -1], [2, 0, -1, -1, -1, -1], [-1, 9, 4, -3, -1, -1]], dtype=np.int64)
    w = np.array([[2, -1, nan, inf, -inf, 0.5], [0.0, 1, 1, nan, 0, 0], [-0.0, 3, inf, 0, 0, 0], [nan, inf, 1, 1, 0, 0]], dtype=np.float32)
    out, bound = R.sum_ids(x, ids, w)
    # absent slots carry NaN / inf weights and add nothing; a duplicate adds once per slot; a zero weight (either sign) skips a NaN row
    np.testing.assert_array_equal(out, [[2 - 3 + 1.5, 4 - 4 + 2], [14, 16], [3, 6], [0, 0]])
    assert np.isfinite(bound).all() and (bound[3] == 0).all() and (bound[:3] > 0).all()
    # a non-zero weight on the NaN row: exactly its NaN column; a NaN weight on a present slot: the whole row, of that query only
    out, _ = R.sum_ids(x, np.array([[2, 0], [0, 1]]), np.array([[1.0, 1.0], [nan, 1.0]]))
    assert np.isnan(out[0, 0]) and out[0, 1] == 7 and np.isnan(out[1]).all()
    # id_base and labels: the rule of score_ids
    out, _ = R.sum_ids(x[:2], np.array([[999, 1000, 1001, 1002]]), np.ones((1, 4)), id_base=1000)
    np.testing.assert_array_equal(out, [[4, 6]])
    lab = np.array([0, 1, 0, 1], dtype=np.int32)
    ql = np.array([[1, -1], [-1, -1], [-2, -1]], dtype=np.int32)
    out, _ = R.sum_ids(x, np.array([[0, 1, 3]] * 3), np.ones((3, 3)), row_labels=lab, q_labels=ql)
    np.testing.assert_array_equal(out, [[10, 12], [11, 14], [0, 0]])
    keep = R.contributing(np.array([[0, 1, 3]] * 3), np.ones((3, 3)), 4, 0, lab, ql)
    np.testing.assert_array_equal(keep, np.isfinite(S.score_ids_aligned(np.ones((3, 2)), np.nan_to_num(x), np.array([[0, 1, 3]] * 3), 0, lab, ql)))


def _fused_sum(terms64, order_chunks):
    """float32 sum of exact float64 products `terms64` [n, d]: inside a run acc = fl32(acc + term) - the product fused into its add -
    and the runs' sums added as float32 in the tree `order_chunks` describes (a list of runs or nested lists of them)"""
    def run(node):
        if isinstance(node, np.ndarray):
            acc = np.zeros(terms64.shape[1], dtype=np.float32)
            for j in node:
                acc = (acc.astype(np.float64) + terms64[j]).astype(np.float32)
            return acc
        acc = run(node[0])
        for child in node[1:]:
            acc = acc + run(child)  # float32 + float32
        return acc
    return run(order_chunks)


@pytest.mark.parametrize("kind", ["gauss", "softmax", "cancelling"])
def test_bound_holds_for_float32_sums_in_any_order_and_chunking(kind):
    rng = np.random.default_rng(5)
    n, d = 1000, 48
    x = rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
    if kind == "gauss":
        w = rng.standard_normal(n).astype(np.float32)
    elif kind == "softmax":
        z = rng.standard_normal(n) * 4
        w = (np.exp(z - z.max()) / np.exp(z - z.max()).sum()).astype(np.float32)
    else:  # pairs that cancel to rounding level: the bound is on sum |terms|, not on |sum|
        w = rng.standard_normal(n).astype(np.float32)
        x[1::2], w[1::2] = x[0::2], -w[0::2] * np.float32(1 + 2.0 ** -12)
    ids = np.arange(n, dtype=np.int64)[None]
    ref, bound = R.sum_ids(x, ids, w[None])
    terms = w.astype(np.float64)[:, None] * x.astype(np.float64)  # exact: 24 + 11 significant bits
    idx = np.arange(n)
    kernel = [[c[i : i + 8] for i in range(0, len(c), 8)] for c in (idx[s : s + 32] for s in range(0, n, 32))]
    orders = {
        "forward": idx, "backward": idx[::-1].copy(), "shuffled": rng.permutation(n),
        "runs of 8, chunks of 32 (the kernel)": kernel,
        "chunks of 512": [idx[s : s + 512] for s in range(0, n, 512)],
        "chunks of 7": [idx[s : s + 7] for s in range(0, n, 7)],
        "halves of halves": [[idx[:250], idx[250:500]], [idx[500:750], idx[750:]]],
    }
    worst = 0.0
    for name, order in orders.items():
        got = _fused_sum(terms, order).astype(np.float64)
        frac = (np.abs(got - ref[0]) / bound[0]).max()
        worst = max(worst, frac)
        assert frac <= 1.0, (name, frac)
    print(f"{kind}: largest fraction of the bound over {len(orders)} orders = {worst:.3f}")
    # the bound is small enough to see a mistake: a sum that loses its heaviest slot is outside it somewhere
    lost = _fused_sum(terms, np.setdiff1d(idx, [np.argmax(np.abs(w))])).astype(np.float64)
    assert (np.abs(lost - ref[0]) > bound[0]).any()
    assert (R.cast_bound(ref, bound, "bfloat16") > R.cast_bound(ref, bound, "float16")).all()
    np.testing.assert_array_equal(R.cast_bound(ref, bound, "float32"), bound)


# ---- ragged lists ----------------------------------------------------------------------------------------------------------------
def test_ragged_ids_and_weights_are_padded_with_minus_one_and_zero():
    from vod_amd.index import pad_listed_ids, pad_listed_weights

    ids = pad_listed_ids([[5, 7, 9], [], [3]])
    w = pad_listed_weights([[0.5, 2, -1], [], [4]], ids.shape)
    np.testing.assert_array_equal(ids, [[5, 7, 9], [-1, -1, -1], [3, -1, -1]])
    np.testing.assert_array_equal(w, [[0.5, 2, -1], [0, 0, 0], [4, 0, 0]])
    assert w.dtype == np.float32 and w.flags.c_contiguous
    assert pad_listed_weights([[], []], (2, 1)).tolist() == [[0.0], [0.0]]  # a batch of empty lists is still a list
    a = np.arange(6, dtype=np.float64).reshape(2, 3)
    assert pad_listed_weights(a, (2, 3)).dtype == np.float32
    for bad, shape in (([[1.0, 2.0]], (1, 1)), ([[1.0]], (2, 1)), (np.zeros((2, 2)), (2, 3))):
        with pytest.raises(ValueError, match="expected weights of shape"):
            pad_listed_weights(bad, shape)


# ---- the autograd wiring ---------------------------------------------------------------------------------------------------------
class _NumpyIndex:
    """what `_ListedScores` needs, in NumPy: `score_ids` and `sum_ids` of the two restatements over float32 rows"""

    def __init__(self, x):
        self.x = x
        self.calls = []

    def score_ids(self, queries, ids, *, subset=None, id_base=0):
        assert not queries.requires_grad
        self.calls.append(("score_ids", subset, id_base))
        return S.score_ids_aligned(queries.float().numpy(), self.x, np.asarray(ids), id_base).astype(np.float32)

    def sum_ids(self, ids, weights, *, subset=None, id_base=0):
        self.calls.append(("sum_ids", subset, id_base))
        return R.sum_ids(self.x, np.asarray(ids), weights.numpy(), id_base)[0].astype(np.float32)


@pytest.mark.parametrize("qdt", ["float32", "float16", "bfloat16"])
def test_listed_scores_autograd_wiring_through_a_numpy_index(qdt):
    torch = pytest.importorskip("torch")
    from vod_amd.index import _ListedScores, listed_scores_backward

    rng = np.random.default_rng(9)
    x = rng.integers(-8, 9, size=(50, 16)).astype(np.float32)
    ids = rng.integers(0, 50, size=(4, 7)).astype(np.int64) + 100
    ids[0, 2], ids[1, :], ids[2, 5] = -1, -1, 150  # an empty slot, an empty list, id = id_base + ntotal
    index = _NumpyIndex(x)
    dt = getattr(torch, qdt)
    q = torch.from_numpy(rng.integers(-4, 5, size=(4, 16)).astype(np.float32)).to(dt).requires_grad_()
    kw = {"subset": None, "id_base": 100}
    scores = _ListedScores.apply(q, index, torch.from_numpy(ids), kw)
    ref = S.score_ids_aligned(q.detach().float().numpy(), x, ids, 100)
    assert scores.dtype == torch.float32 and scores.requires_grad
    np.testing.assert_array_equal(scores.detach().numpy().astype(np.float64), ref)  # the bits of score_ids, -inf where absent
    assert np.isneginf(ref[1]).all() and np.isneginf(ref[0, 2]) and np.isneginf(ref[2, 5])
    # an upstream gradient that is NaN exactly at the -inf slots (what d/ds of a softmax over -inf scores produces)
    g = rng.integers(-4, 5, size=ids.shape).astype(np.float32) / 8
    g[np.isneginf(ref)] = np.nan
    scores.backward(torch.from_numpy(g))
    want = R.sum_ids(x, ids, g, 100)[0]
    assert q.grad.dtype == dt and q.grad.device == q.device and q.grad.shape == q.shape
    assert torch.isfinite(q.grad).all() and (q.grad[1] == 0).all()
    np.testing.assert_array_equal(q.grad.float().numpy().astype(np.float64), torch.from_numpy(want).to(dt).double().numpy())
    assert index.calls == [("score_ids", None, 100), ("sum_ids", None, 100)]
    # the plain function is the whole backward
    again = listed_scores_backward(index, ids, torch.from_numpy(g), dt, q.device, **kw)
    assert torch.equal(again, q.grad)
    # through a loss, against torch's own autograd over the materialised gather (integers: exact in every dtype involved)
    q2 = q.detach().clone().float().requires_grad_()
    live = torch.from_numpy(np.isfinite(ref))
    dense = (torch.from_numpy(x)[torch.from_numpy(np.clip(ids - 100, 0, 49))] @ q2[:, :, None])[:, :, 0]
    (torch.where(live, dense, torch.zeros(())) ** 2).sum().backward()
    q3 = q.detach().clone().float().requires_grad_()
    s3 = _ListedScores.apply(q3, index, torch.from_numpy(ids), kw)
    (torch.where(live, s3, torch.zeros(())) ** 2).sum().backward()
    assert torch.equal(q3.grad, q2.grad)


def test_listed_scores_is_once_differentiable_and_leaves_the_other_arguments_alone():
    torch = pytest.importorskip("torch")
    from vod_amd.index import _ListedScores

    x = np.eye(4, dtype=np.float32)
    q = torch.ones(2, 4, requires_grad=True)
    ids = torch.tensor([[0, 1], [2, 3]])
    s = _ListedScores.apply(q, _NumpyIndex(x), ids, {"subset": None, "id_base": 0})
    (g,) = torch.autograd.grad((s ** 2).sum() / 2, q, create_graph=True)  # (the upstream gradient, s itself, depends on q)
    np.testing.assert_array_equal(g.detach().numpy(), [[1, 1, 0, 0], [0, 0, 1, 1]])
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    with torch.no_grad():
        assert not _ListedScores.apply(q, _NumpyIndex(x), ids, {"subset": None, "id_base": 0}).requires_grad


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_listed_and_exported():
    from vod_amd import _native

    flat_res, flat_args = _native.SIGNATURES["vodhip_index_sum_ids"]
    node_res, node_args = _native.SIGNATURES["vodhip_node_index_sum_ids"]
    assert flat_res is ctypes.c_int32 or flat_res is ctypes.c_int
    assert len(flat_args) == 10 and len(node_args) == 10 and node_res is flat_res
    lib = _native.load_library()
    for name in ("vodhip_index_sum_ids", "vodhip_node_index_sum_ids"):
        assert getattr(lib, name) is not None
    # refusals that need no device: a NULL handle
    assert lib.vodhip_index_sum_ids(None, None, None, 0, 1, 0, None, 0, None, None) < 0
    assert b"index is NULL" in lib.vodhip_last_error()
    assert lib.vodhip_node_index_sum_ids(None, None, None, 0, 1, None, 0, 0, None, None) < 0
