"""The fused retrieval loss (vod_amd/csrc/kernels_retrieval.hip) at its tile, split-K, dtype, padding and alignment edges.

Every case runs `RetrievalGradients` forward and backward (upstream gradient 2.5) and is compared, output by output, with the float64
oracle on the same (already rounded) inputs.  The case tables and the branch each row is there for live in `retrieval_edge_cases.py`;
tests/test_retrieval_edge_cases_cpu.py proves on the CPU that every branch is hit by an fp32 row and by a 16-bit row.

Comparators
  * `retriever_scores`: a-priori, elementwise `|got - fp64| <= H * 2^-24 * (|q| . |s|^T)` - any correct fp32 accumulation of H products
    satisfies it in any order, with or without FMA; a dropped element or K tile does not.  Padded positions must be -inf exactly.
  * loss, every diagnostic, dq, ds: `|got - fp64| <= F * dev32` (F per output class, below), floored at 4 float32 ulps of the output's largest magnitude, where
    `dev32 = max |float32 oracle - float64 oracle|` on the same inputs: the reference arithmetic's own float32 error is the unit.
    16-bit runs add half an ulp of the format to dq and ds, which are cast back (2^-11 / 2^-8 relative, 2^-25 absolute below the fp16
    normal range).
  * the only elements left out are those where the float64 oracle itself is NaN / inf; there the positions must match exactly, and
    the oracle must be finite in at least 95 % of every compared array (asserted; the all-rows-padded case is NaN by design).

F: measured once over every case and output of this module on an MI355X (profiles/r09_h5_error.txt holds the complete table), per
output class, each the next power of two at or above twice the largest `err / dev32` among outputs whose error exceeds the floor:
  * dq, ds (arrays; fp32 rows - in the 16-bit rows the cast back dominates and says nothing about F): largest ratio 4.6
    -> F_GRAD = 16.  The plain entry point's dLoss/dScores uses it too.
  * loss and the diagnostics (one number each, so dev32 is a single sample of the float32 oracle's error): largest ratio 46.8,
    kl_score of the 3-D 5 x 255 x 65 bf16 case - its error of 1.949e-6 sits AT the floor of 1.944e-6, its dev32 happens to be 4.2e-8;
    the next ratios are 24, 17, 15 and 12 -> F_SCALAR = 128.  It binds the scalars only: the gradients' bound does not see it.
The a-priori score bound is used up to 0.995 at H = 1 (one product, one rounding: the bound is exactly half an ulp) and below 0.1
from H = 63 on.
"""
import numpy as np
import pytest

import retrieval_edge_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F_SCALAR = 128.0  # loss and the diagnostics: one number each
F_GRAD = 16.0     # dq, ds (and dLoss/dScores of the plain entry point): arrays
ULP32 = 2.0 ** -23
HALF_ULP = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -8}
TDT = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _dev(a, dtype=None):
    return torch.tensor(a, device="cuda") if dtype is None else torch.tensor(a, device="cuda", dtype=dtype)


def _run(x, dtype="float32", aux=False, q=None, s=None):
    """Forward + backward on the GPU -> dict of float64 NumPy outputs (gradients of loss * UPSTREAM)."""
    from vod_amd.gradients import RetrievalGradients

    qt = _dev(x["q"], TDT[dtype]).requires_grad_() if q is None else q
    st = _dev(x["s"], TDT[dtype]).requires_grad_() if s is None else s
    batch = {"section__score": _dev(x["score"]), "section__relevance": _dev(x["relevance"]),
             "section__sparse": _dev(x["sparse"]), "section__dense": _dev(x["dense"])}
    out = RetrievalGradients(**(rc.AUX if aux else {}))(batch=batch, query_encoding=qt, section_encoding=st)
    (out.loss * rc.UPSTREAM).backward()
    assert out.loss.dtype == torch.float32 and qt.grad.dtype == TDT[dtype] and st.grad.dtype == TDT[dtype]
    got = {k: v.detach().double().cpu().numpy() for k, v in out.diagnostics.items()}
    got.update(loss=out.loss.detach().double().cpu().numpy(), retriever_scores=out.retriever_scores.double().cpu().numpy(),
               dq=qt.grad.double().cpu().numpy(), ds=st.grad.double().cpu().numpy())
    return got, out


def _compare(tag, got, x, r64, r32, dtype="float32", min_share=0.95, keys=None):
    """Print one line per output (error, dev32, ratio; for the scores the slack of the a-priori bound), then assert."""
    want, w32 = rc.compared_outputs(r64), rc.compared_outputs(r32)
    if keys is not None:  # (the plain entry point has no backward)
        want, w32 = {k: want[k] for k in keys}, {k: w32[k] for k in keys}
    assert set(got) == set(want), (sorted(got), sorted(want))
    three_d = x["s"].ndim == 3
    H = x["q"].shape[1]
    aq, as_ = np.abs(x["q"].astype(np.float64)), np.abs(x["s"].astype(np.float64))
    failures = []
    for key in sorted(want):
        w, g, w3 = np.asarray(want[key]), np.asarray(got[key]), np.asarray(w32[key], dtype=np.float64)
        assert g.shape == w.shape, key
        fin = np.isfinite(w)
        assert fin.mean() >= min_share, (key, fin.mean())
        # where the oracle is NaN / inf, so is the kernel, with the same sign
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isposinf(g), np.isposinf(w)) and \
            np.array_equal(np.isneginf(g), np.isneginf(w)), f"{tag} {key}: NaN / inf positions differ"
        if not fin.any():
            print(f"H5ERR {tag} {key} err=nan dev32=nan ratio=nan (no finite element by design)")
            continue
        err = np.abs(np.where(fin, g - np.where(fin, w, 0.0), 0.0))
        if key == "retriever_scores":
            bound = H * 2.0 ** -24 * (np.einsum("bh,bdh->bd", aq, as_) if three_d else aq @ as_.T)
            slack = float(np.max(np.where(fin & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)))
            print(f"H5ERR {tag} {key} err={err.max():.3e} apriori_bound_used={slack:.4f}")
            if not np.all(err[fin] <= bound[fin]):
                failures.append(f"{key}: {int((err > bound)[fin].sum())} elements beyond H * 2^-24 * |q|.|s|^T (worst {slack:.2f} x)")
            continue
        dev32 = float(np.max(np.abs(np.where(fin & np.isfinite(w3), w3 - np.where(fin, w, 0.0), 0.0))))
        floor = 4 * ULP32 * float(np.abs(w[fin]).max())
        bound = np.full(w.shape, max((F_GRAD if key in ("dq", "ds") else F_SCALAR) * dev32, floor))
        if dtype != "float32" and key in ("dq", "ds"):
            bound = bound + HALF_ULP[dtype] * np.abs(np.where(fin, w, 0.0)) + (2.0 ** -25 if dtype == "float16" else 0.0)
        e = float(err.max())
        print(f"H5ERR {tag} {key} err={e:.3e} dev32={dev32:.3e} ratio={e / dev32 if dev32 > 0 else float('inf') if e > 0 else 0.0:.3f} "
              f"floor={floor:.3e} over_floor={int(e > floor)}")
        if not np.all(err <= bound):
            failures.append(f"{key}: err {e:.3e} > bound {float(bound.max()):.3e} (dev32 {dev32:.3e})")
    assert not failures, f"{tag}: " + "; ".join(failures)


def _case(B, D, H, three_d=False, dtype="float32", aux=False, **kw):
    x, r64, r32 = rc.reference(B, D, H, three_d, dtype, aux, **kw)
    got, _ = _run(x, dtype, aux)
    tag = f"{'3d' if three_d else '2d'}:{B}x{D}x{H}:{dtype}:{'aux' if aux else 'plain'}" + "".join(f":{k}={v}" for k, v in kw.items())
    _compare(tag, got, x, r64, r32, dtype)


@pytest.mark.parametrize("B,D,H,why", rc.CASES_2D, ids=[f"{b}-{d}-{h}" for b, d, h, _ in rc.CASES_2D])
def test_2d_fp32_case_table(B, D, H, why):
    """Tile edges of M, N and K, the forward and the dq split-K arithmetic, vector / scalar staging - without and with the auxiliary
    terms."""
    for aux in (False, True):
        _case(B, D, H, aux=aux)


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("B,D,H,why", rc.CASES_2D_16BIT, ids=[f"{b}-{d}-{h}" for b, d, h, _ in rc.CASES_2D_16BIT])
def test_2d_16bit_case_table(B, D, H, why, dtype):
    for aux in (False, True):
        _case(B, D, H, dtype=dtype, aux=aux)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("B,D,H,why", rc.CASES_3D, ids=[f"{b}-{d}-{h}" for b, d, h, _ in rc.CASES_3D])
def test_3d_case_table(B, D, H, why, dtype):
    for aux in (False, True):
        _case(B, D, H, three_d=True, dtype=dtype, aux=aux)


@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
@pytest.mark.parametrize("edge", ["padrow", "onelive", "tie"])
def test_row_edges_at_a_split_shape(edge, three_d, aux):
    """The edge fixtures' rows again where the contraction is split: a fully padded row, a row with one live column, exactly tied
    positives (the self-supervision arg-max must take the first; its gradient differs by the one-hot otherwise)."""
    B, D, H = (64, 32, 768) if three_d else (64, 2048, 768)
    _case(B, D, H, three_d=three_d, aux=aux, edge=edge)
    if edge == "tie":
        x, r64, _ = rc.reference(B, D, H, three_d, "float32", aux, edge=edge)
        r = B // 3
        pos = np.flatnonzero(x["relevance"][r] > 0)
        assert len(pos) == 2 and r64["retriever_scores"][r, pos[0]] == r64["retriever_scores"][r, pos[1]]
        got, _ = _run(x, aux=aux)
        assert got["retriever_scores"][r, pos[0]] == got["retriever_scores"][r, pos[1]], "identical encodings must score identically"


@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
def test_d_equals_one_at_a_split_width(three_d, aux):
    _case(64, 1, 768, three_d=three_d, aux=aux)


@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
def test_every_row_padded_is_nan_exactly_where_the_oracle_is(three_d, aux):
    B, D, H = (64, 32, 768) if three_d else (64, 2048, 768)
    x, r64, r32 = rc.reference(B, D, H, three_d, "float32", aux, edge="allpad")
    assert np.isnan(r64["loss"]) and np.isnan(r64["dq"]).all() and np.isneginf(r64["retriever_scores"]).all()
    got, _ = _run(x, aux=aux)
    _compare(f"{'3d' if three_d else '2d'}:allpad:{'aux' if aux else 'plain'}", got, x, r64, r32, min_share=0.0)


@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
def test_every_row_without_positives(three_d):
    """n_positives falls back to the live count in every row (with the self-supervision term the reference's loss is NaN by design)."""
    B, D, H = (64, 32, 768) if three_d else (64, 2048, 768)
    _case(B, D, H, three_d=three_d, edge="nopos")


@pytest.mark.parametrize("aux", [False, True], ids=["plain", "aux"])
@pytest.mark.parametrize("three_d", [False, True], ids=["2d", "3d"])
def test_large_logits_need_the_max_subtraction(three_d, aux):
    B, D, H = (64, 32, 768) if three_d else (64, 2048, 768)
    x, r64, _ = rc.reference(B, D, H, three_d, "float32", aux, q_scale=20.0)
    sc = r64["retriever_scores"]
    assert 60 < np.abs(sc[np.isfinite(sc)]).max() < 700  # exp(logit) overflows float32 without the subtraction, fp64 stays finite
    _case(B, D, H, three_d=three_d, aux=aux, q_scale=20.0)


def test_sixteen_bit_at_the_3d_training_shape_with_row_edges():
    for dtype in ("float16", "bfloat16"):
        _case(64, 32, 768, three_d=True, dtype=dtype, aux=True, edge="padrow")


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------------


def _bytes(x, aux=True, dtype="float32"):
    got, _ = _run(x, dtype, aux)
    torch.cuda.synchronize()
    return {k: v.tobytes() for k, v in got.items()}


def test_a_split_shape_run_twice_gives_identical_bytes():
    x, _, _ = rc.reference(64, 2048, 768, False, "float32", True)
    assert _bytes(x) == _bytes(x)


def test_scratch_reuse_across_shapes_leaves_no_trace():
    """(64, 512, 512) and (64, 512, 520) share one scratch key (its size does not depend on H); the second has an empty slab, which must
    be written as zeros over the first's partial sums - and the first, run again, must not see the second's."""
    from vod_amd import gradients

    a, _, _ = rc.reference(64, 512, 512, False, "float32", True)
    b, b64, b32 = rc.reference(64, 512, 520, False, "float32", True)
    first = _bytes(a)
    n_keys = len(gradients._scratch)
    got_b, _ = _run(b, aux=True)
    assert len(gradients._scratch) == n_keys, "the two shapes must share one scratch buffer"
    _compare("2d:64x512x520:after-64x512x512", got_b, b, b64, b32)
    assert _bytes(a) == first


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("three_d,D,H", [(False, 512, 512), (True, 32, 768)], ids=["2d", "3d"])
def test_graphed_step_in_16_bit_replays_the_eager_step_bit_for_bit(three_d, D, H, dtype):
    from vod_amd.gradients import GraphedRetrievalStep, RetrievalGradients

    B = 64
    grad = RetrievalGradients(**rc.AUX)
    step = GraphedRetrievalStep(grad, batch_size=B, n_sections=D, hidden=H, sections_3d=three_d, dtype=TDT[dtype], device=0)
    for seed in (0, 1):
        x = rc.make_inputs(B, D, H, three_d, dtype, True, seed=seed)
        batch = {f"section__{k}": _dev(x[k]) for k in ("score", "relevance", "sparse", "dense")}
        q, s = _dev(x["q"], TDT[dtype]), _dev(x["s"], TDT[dtype])
        out, dq, ds = step(batch=batch, query_encoding=q, section_encoding=s)
        qe, se = q.clone().requires_grad_(), s.clone().requires_grad_()
        # the captured step accumulates into zeroed `.grad` buffers, and 0 + (-0.0) = +0.0: fp16 gradients that underflow to -0.0 would
        # differ in the sign bit from a backward that merely stores.  The eager step accumulates the same way, so bytes are comparable.
        qe.grad, se.grad = torch.zeros_like(qe), torch.zeros_like(se)
        ref = grad(batch=batch, query_encoding=qe, section_encoding=se)
        ref.loss.backward()
        same = lambda a, b: a.dtype == b.dtype and bool(torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8),  # noqa: E731
                                                                       b.detach().contiguous().reshape(-1).view(torch.uint8)))  # bytes: NaN == NaN
        assert torch.isfinite(ref.loss)
        assert same(out.loss, ref.loss) and same(out.retriever_scores, ref.retriever_scores)
        assert list(out.diagnostics) == list(ref.diagnostics)
        for key in ref.diagnostics:
            assert same(out.diagnostics[key], ref.diagnostics[key]), key
        assert dq.dtype == TDT[dtype] and same(dq, qe.grad) and same(ds, se.grad)


# ---- limits ---------------------------------------------------------------------------------------------------------------------------


def test_more_than_16384_sections_fail_loudly_and_the_next_call_works():
    from vod_amd import _native

    x = rc.make_inputs(1, 16385, 8)
    with pytest.raises(_native.NativeLibraryError, match="16384"):
        _run(x)
    _case(1, 512, 520)


def _plain_forward(x, order, B, D, H):
    """`vodhip_retrieval_forward` with a workspace of 16 floats per row (the kernel writes 8 row words) and the two outputs placed by `order` in one [3, B, D] buffer."""
    from vod_amd import _native

    lib = _native.load_library()
    qt, st, sc, rl = _dev(x["q"]), _dev(x["s"]), _dev(x["score"]), _dev(x["relevance"])
    sp, de = _dev(x["sparse"]), _dev(x["dense"])
    both = torch.full((3, B, D), 7.0, device="cuda")
    small = torch.full((4 + 16 * B,), 7.0, device="cuda")
    scores, d_scores = both[order[0]], both[order[1]]
    rc_ = lib.vodhip_retrieval_forward(qt.data_ptr(), st.data_ptr(), _native.F32, 0, B, D, H, sc.data_ptr(), rl.data_ptr(), sp.data_ptr(),
                                       de.data_ptr(), scores.data_ptr(), d_scores.data_ptr(), small[0:1].data_ptr(), small[1:4].data_ptr(),
                                       small[4:].data_ptr(), _native.current_stream_ptr(qt.device))
    torch.cuda.synchronize()
    return rc_, both, small, scores, d_scores


@pytest.mark.parametrize("B,D,H,order", [(64, 2048, 768, (1, 0)), (64, 2048, 768, (0, 1)), (64, 300, 256, (1, 0)), (65, 513, 520, (1, 0)),
                                         (65, 513, 520, (2, 0))])
def test_plain_entry_point(B, D, H, order):
    """Adjacent outputs are the contraction's two slabs when H >= 512 - in either order (`d_scores` first: slab 0 is d_scores) - and
    the row kernel reads its row of both before it writes them; H < 512 and distant outputs run unsplit.  Scores by the a-priori bound,
    loss / KLs / dLoss/dScores by the dev32 bound."""
    x, r64, r32 = rc.reference(B, D, H)
    status, _both, small, scores, d_scores = _plain_forward(x, order, B, D, H)
    assert status == 0
    got = {"loss": small[0], "kl_score": small[1], "kl_sparse": small[2], "kl_dense": small[3], "retriever_scores": scores}
    got = {k: v.double().cpu().numpy() for k, v in got.items()}
    _compare(f"plain:{B}x{D}x{H}:order{order}", got, x, r64, r32, keys=list(got))
    dev32 = np.abs(r32["d_scores"] - r64["d_scores"]).max()
    err = np.abs(d_scores.double().cpu().numpy() - r64["d_scores"]).max()
    print(f"H5ERR plain:{B}x{D}x{H}:order{order} d_scores err={err:.3e} dev32={dev32:.3e} ratio={err / dev32:.3f}")
    assert err <= max(F_GRAD * dev32, 4 * ULP32 * np.abs(r64["d_scores"]).max())


def test_plain_entry_point_refuses_rows_beyond_the_lds_and_the_next_call_works():
    from vod_amd import _native

    B, D, H = 1, 4, 40960  # (H + D + 4) floats of LDS > 160 KB
    x = rc.make_inputs(B, D, H)
    status, both, small, _, _ = _plain_forward(x, (0, 1), B, D, H)
    assert status != 0
    with pytest.raises(_native.NativeLibraryError):
        _native.check(status)
    assert bool((both == 7.0).all()) and bool((small == 7.0).all()), "a refused call must leave its outputs untouched"
    test_plain_entry_point(65, 513, 520, (1, 0))


# ---- base-address alignment -----------------------------------------------------------------------------------------------------------


def _view_into(arr, dtype, offset_elems):
    """A contiguous view of `arr`'s shape that starts `offset_elems` elements into a larger storage."""
    buf = torch.zeros(arr.size + offset_elems, device="cuda", dtype=TDT[dtype])
    view = buf[offset_elems:].view(arr.shape)
    view.copy_(_dev(arr, TDT[dtype]))
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset_elems * buf.element_size()
    return view.requires_grad_()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("three_d,B,D,H", [(False, 64, 128, 128), (False, 65, 513, 516), (True, 5, 64, 64)])
def test_a_contiguous_view_one_element_into_its_storage(three_d, B, D, H, dtype):
    """Aligned pitch, misaligned base: `is_contiguous()` is true, so the wrapper passes the pointer on; `vec_ok` looks at the base
    address (16 B for f32, 8 B for 16 bit) and such an operand takes the scalar path."""
    x, r64, r32 = rc.reference(B, D, H, three_d, dtype, True)
    q, s = _view_into(x["q"], dtype, 1), _view_into(x["s"], dtype, 1)
    assert q.data_ptr() % (16 if dtype == "float32" else 8) != 0 and s.data_ptr() % (16 if dtype == "float32" else 8) != 0
    got, _ = _run(x, dtype, True, q=q, s=s)
    _compare(f"{'3d' if three_d else '2d'}:{B}x{D}x{H}:{dtype}:misaligned-base", got, x, r64, r32, dtype)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_a_view_at_a_row_offset_and_a_non_contiguous_query(dtype):
    """`s` = rows 3.. of a larger matrix (contiguous, still 16 B aligned: the vector path); `q` = the transpose of an [H, B] leaf, which
    the wrapper copies - its gradient must arrive transposed at the leaf."""
    B, D, H = 64, 128, 128
    x, r64, r32 = rc.reference(B, D, H, False, dtype, True)
    s = _view_into(x["s"], dtype, 3 * H)
    assert s.data_ptr() % 16 == 0
    q_leaf = _dev(np.ascontiguousarray(x["q"].T), TDT[dtype]).requires_grad_()
    q = q_leaf.t()
    assert not q.is_contiguous()
    from vod_amd.gradients import RetrievalGradients

    batch = {f"section__{k}": _dev(x[k]) for k in ("score", "relevance", "sparse", "dense")}
    out = RetrievalGradients(**rc.AUX)(batch=batch, query_encoding=q, section_encoding=s)
    (out.loss * rc.UPSTREAM).backward()
    got = {k: v.detach().double().cpu().numpy() for k, v in out.diagnostics.items()}
    got.update(loss=out.loss.detach().double().cpu().numpy(), retriever_scores=out.retriever_scores.double().cpu().numpy(),
               dq=q_leaf.grad.t().double().cpu().numpy(), ds=s.grad.double().cpu().numpy())
    _compare(f"2d:{B}x{D}x{H}:{dtype}:row-offset-view+transposed-q", got, x, r64, r32, dtype)
