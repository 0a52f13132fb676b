"""The hybrid merge kernel (`merge_hybrid_kernel`, vod_amd/csrc/kernels_hybrid.hip) at its own seams, bit for bit against the CPU
oracle (`oracle.hybrid.merge_hybrid`, pinned to the reference by tests/test_oracle_golden.py):

  * `merge_edges.npz`: input classes the reference defines (64-bit ids that differ in the high word only, ids < -1, a -1 inside a
    list, +-inf / NaN scores, zero / negative weights, a repeated lookup id with different labels), reference-generated;
  * exact row widths at the prefix scan's chunk boundary (512 / 513), at every table-size transition, where the LDS cap starts to
    bite (3984 / 3985) and at the ABI's limit (4095 / 4096, the largest LDS footprint), with small and with 64-bit id pools;
  * degenerate rows (one id everywhere, nothing but -1, the same permutation in every segment, all -inf, all NaN);
  * the two forms of the cut-width hand-over to the sampler - per-row cursors and cursor maxima (memset + atomicMax) - on the same
    inputs, and the tall batch (nq > 4096) that takes the maxima form by itself, through `sample_merged_on_device`;
  * C-ABI shapes the Python wrapper never produces (NULL outputs, a wider stride, both cursor outputs, nq = 0, a refused width);
  * run-to-run: the table is built with CAS / atomicMin races whose outcome must not show.

The kernel's contract is bit-exact: every comparison is `array_equal` (NaN == NaN) with dtype and shape checked."""
import ctypes
import json

import numpy as np
import pytest

from conftest import GOLDEN
from test_collate_device_gpu import TOL_RANDOM, _check_sampled
from test_hybrid_gpu import _eq

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MANIFEST = json.loads((GOLDEN / "manifest.json").read_text())
WEIGHTS = (1.0, -1.5, 0.0, 2.0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle(l_idx, l_lbl, engs, weights):
    from oracle.hybrid import merge_hybrid

    with np.errstate(all="ignore"):
        return merge_hybrid((l_idx, np.zeros(l_idx.shape, np.float32), l_lbl), engs, weights)


def _device(l_idx, l_lbl, engs, weights, **kw):
    from vod_amd.core.merge import merge_hybrid_device

    return merge_hybrid_device(_t(l_idx), _t(l_lbl), {n: (_t(i), _t(s)) for n, (i, s) in engs.items()}, weights, **kw)


def _full_stride(case, ref, stride, lbl_in=True):
    """What the kernel leaves at full stride: the oracle's row up to the row's cursor, then pad columns - id -1, score -inf, and (SURVEY
    quirk Q3: the pad id MATCHES the -1 entries of the lists) the label of the lookup's FIRST -1 and every engine's min-subtracted
    score at ITS first -1; -1 / NaN where a list has none.  Restated from the inputs, so that columns beyond the oracle's cut are
    checked too."""
    from oracle.hybrid import subtract_min_score

    l_idx, l_lbl, engs, _ = case
    o_idx, o_scr, o_lbl, o_raw = ref
    nq, w = o_idx.shape
    first_pad = lambda row: int(np.argmax(row == -1)) if (row == -1).any() else -1   # noqa: E731
    idx = np.full((nq, stride), -1, dtype=np.int64)
    scr = np.full((nq, stride), -np.inf, dtype=np.float32)
    lbl = np.full((nq, stride), -1, dtype=np.int64)
    raw = {n: np.full((nq, stride), np.nan, dtype=np.float32) for n in engs}
    with np.errstate(all="ignore"):
        norm = {n: subtract_min_score(s, 0.0) if s.size else s for n, (_, s) in engs.items()}
    for r in range(nq):
        cur = int((o_idx[r] >= 0).sum())
        assert (o_idx[r, :cur] >= 0).all()
        q = first_pad(l_idx[r])
        if lbl_in and q >= 0:
            lbl[r] = l_lbl[r, q]
        for n, (e_idx, _) in engs.items():
            q = first_pad(e_idx[r])
            if q >= 0:
                raw[n][r] = norm[n][r, q]
            raw[n][r, :cur] = o_raw[n][r, :cur]
        idx[r, :cur], scr[r, :cur] = o_idx[r, :cur], o_scr[r, :cur]
        if lbl_in:
            lbl[r, :cur] = o_lbl[r, :cur]
    # where the oracle's own cut holds pad columns, it reports the same values
    for mine, theirs in [(idx, o_idx), (scr, o_scr)] + ([(lbl, o_lbl)] if lbl_in else []) + [(raw[n], o_raw[n]) for n in engs]:
        _eq(mine[:, :w], theirs)
    return idx, scr, lbl, raw


def _check_merged(merged, case, ref):
    """The cut is the oracle's merged batch, bit for bit; every column beyond a row's cursor, up to the stride, is a pad column."""
    o_idx, o_scr, o_lbl, o_raw = ref
    c_idx, c_scr, c_lbl, c_raw = merged.cut()
    _eq(c_idx.cpu().numpy(), o_idx)
    _eq(c_scr.cpu().numpy(), o_scr)
    _eq(c_lbl.cpu().numpy(), o_lbl)
    assert set(c_raw) == set(o_raw)
    for n in o_raw:
        _eq(c_raw[n].cpu().numpy(), o_raw[n])
    idx, scr, lbl, raw = _full_stride(case, ref, merged.stride)
    _eq(merged.indices.cpu().numpy(), idx)
    _eq(merged.scores.cpu().numpy(), scr)
    _eq(merged.labels.cpu().numpy(), lbl)
    for n in raw:
        _eq(merged.raw[n].cpu().numpy(), raw[n])


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference-made fixture
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["one_engine", "two_engines", "four_engines"])
def test_edge_inputs_match_reference_golden(case):
    from vod_amd.core.merge import merge_hybrid

    g = np.load(GOLDEN / "merge_edges.npz")
    w = MANIFEST["merge_edges"]["params"]["cases"][case]
    engines = {n: (g[f"{n}_idx"], g[f"{n}_scr"]) for n in w}
    idx, scr, lbl, raw = merge_hybrid(g["lookup_idx"], g["lookup_lbl"], engines, dict(w))
    _eq(idx, g[f"{case}_out_idx"])
    _eq(scr, g[f"{case}_out_scr"])
    _eq(lbl, g[f"{case}_out_lbl"])
    assert set(raw) == set(w)
    for n in w:
        _eq(raw[n], g[f"{case}_raw_{n}"])


# ---------------------------------------------------------------------------------------------------------------------------------
# exact widths
# ---------------------------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 16, 17, 64, 65, 511, 512, 513, 1024, 1025, 2048, 2049, 3984, 3985, 4095, 4096]
NO_LOOKUP = (1, 17, 513, 4096)   # kl = 0
EMPTY_ENGINE = 65                # (W = 1 has one too: there is nothing to give it)


def _split(W):
    """W over the lookup list and two to four engines of unequal sizes: (kl, [k_e])."""
    n_eng = 2 + WIDTHS.index(W) % 3
    share = [3, 5, 2, 7, 4][: n_eng + (W not in NO_LOOKUP)]
    sizes = [W * s // sum(share) for s in share]
    sizes[int(np.argmax(share))] += W - sum(sizes)
    kl, ks = (0, sizes) if W in NO_LOOKUP else (sizes[0], sizes[1:])
    if W == EMPTY_ENGINE:
        ks = [ks[0], 0, *ks[1:]]
    assert kl + sum(ks) == W and 2 <= len(ks) <= 4
    return kl, ks


def _three_rows(rng, k, pool, lookup):
    """Row 0: no id repeated inside the list; row 1: some repeated; row 2: half of the entries -1, at random positions, half of
    those with a finite score (and, in the lookup, a label) - what the pad columns then report."""
    idx = np.stack([rng.choice(pool, size=k, replace=False) for _ in range(3)]).astype(np.int64).reshape(3, k)
    scr = (rng.normal(size=(3, k)) * 3).astype(np.float32)
    if k >= 2:
        src = rng.integers(0, k, size=max(1, k // 8))
        idx[1, rng.integers(0, k, size=len(src))] = idx[1, src]
    pad = rng.random(k) < 0.5
    idx[2, pad] = -1
    scr[2, pad & (rng.random(k) < 0.5)] = -np.inf
    if not lookup:
        return idx, scr
    return idx, np.where(idx >= 0, rng.integers(1, 4, size=idx.shape), rng.integers(0, 3, size=idx.shape)).astype(np.int64)


def _width_case(W, wide_ids, seed=0):
    kl, ks = _split(W)
    rng = np.random.default_rng(7919 * W + wide_ids + 2 * seed)
    n_pool = max(W // 2, kl, *ks, 1)   # about W / 2: most ids occur in several segments
    j = np.arange(n_pool, dtype=np.int64)
    pool = (j << 33) + j % 3 if wide_ids else j   # 64-bit: many ids share their low word
    l_idx, l_lbl = _three_rows(rng, kl, pool, True)
    engs = {f"e{e}": _three_rows(rng, k, pool, False) for e, k in enumerate(ks)}
    return l_idx, l_lbl, engs, {n: w for n, w in zip(engs, WEIGHTS)}


@pytest.mark.parametrize("wide_ids", [False, True], ids=["pool_half_w", "pool_64bit"])
@pytest.mark.parametrize("W", WIDTHS)
def test_exact_widths(W, wide_ids):
    case = _width_case(W, wide_ids)
    assert case[0].shape[1] + sum(i.shape[1] for i, _ in case[2].values()) == W
    _check_merged(_device(*case), case, _oracle(*case))


# ---------------------------------------------------------------------------------------------------------------------------------
# degenerate rows at W = 385: kl 128, two engines of 128, one of 1
# ---------------------------------------------------------------------------------------------------------------------------------
DEGENERATE = ["same_id", "all_pad", "same_permutation", "all_neg_inf", "all_nan", "ordinary"]


def _degenerate_row(kind, rng):
    sizes = [128, 128, 128, 1]
    idx = [rng.choice(300, size=k, replace=False).astype(np.int64) for k in sizes]
    scr = [(rng.normal(size=k) * 3).astype(np.float32) for k in sizes]
    lbl = rng.integers(1, 4, size=128).astype(np.int64)
    if kind == "same_id":
        idx = [np.full(k, 2**40 + 17, dtype=np.int64) for k in sizes]
    elif kind == "all_pad":   # the scores stay finite: they set the row minima and the pad columns' raw scores
        idx = [np.full(k, -1, dtype=np.int64) for k in sizes]
    elif kind == "same_permutation":
        perm = rng.permutation(128).astype(np.int64) + 1000
        idx = [perm[:k].copy() for k in sizes]
    elif kind == "all_neg_inf":
        scr = [np.full(k, -np.inf, dtype=np.float32) for k in sizes]
    elif kind == "all_nan":
        scr = [np.full(k, np.nan, dtype=np.float32) for k in sizes]
    return idx, scr, lbl


def _degenerate_batch(kinds, seed):
    rng = np.random.default_rng(seed)
    rows = [_degenerate_row(k, rng) for k in kinds]
    l_idx = np.stack([r[0][0] for r in rows])
    l_lbl = np.stack([r[2] for r in rows])
    engs = {f"e{e}": (np.stack([r[0][e + 1] for r in rows]), np.stack([r[1][e + 1] for r in rows])) for e in range(3)}
    return l_idx, l_lbl, engs, {"e0": 1.0, "e1": -1.5, "e2": 2.0}


@pytest.mark.parametrize("kind", DEGENERATE[:-1] + ["one_of_each"])
def test_degenerate_rows(kind):
    kinds = DEGENERATE if kind == "one_of_each" else [kind, kind]
    case = _degenerate_batch(kinds, 31 + len(kind))
    _check_merged(_device(*case), case, _oracle(*case))


# ---------------------------------------------------------------------------------------------------------------------------------
# the cut width's two ways to the sampler: per-row cursors / cursor maxima
# ---------------------------------------------------------------------------------------------------------------------------------
def _random_case(rng, nq, kl, ks, pool, pad_frac=0.3):
    def lst(k):
        idx = np.full((nq, k), -1, dtype=np.int64)
        scr = np.full((nq, k), -np.inf, dtype=np.float32)
        for r in range(nq):
            nv = k if rng.random() > pad_frac else int(rng.integers(0, k + 1))
            idx[r, :nv] = rng.choice(pool, size=nv, replace=pool < nv)
            scr[r, :nv] = (rng.normal(size=nv) * 3).astype(np.float32)
        return idx, scr

    l_idx, _ = lst(kl)
    l_lbl = np.where(l_idx >= 0, rng.integers(0, 3, size=l_idx.shape), 0).astype(np.int64)
    engs = {f"e{e}": lst(k) for e, k in enumerate(ks)}
    return l_idx, l_lbl, engs, {n: w for n, w in zip(engs, WEIGHTS)}


@pytest.mark.parametrize("nq", [3, 64, 300])
def test_cursor_maxima_equal_per_row_cursors(nq):
    case = _random_case(np.random.default_rng(nq), nq, 8, [16, 12, 5, 9], 60)
    ref = _oracle(*case)
    rows = _device(*case, cursors="per_row")
    maxima = _device(*case, cursors="max")
    assert rows.stage_max is None and rows.row_cursor.shape == (nq, 4) and rows.row_cursor.dtype == torch.int32
    assert maxima.row_cursor is None and maxima.stage_max.shape == (4,) and maxima.stage_max.dtype == torch.int32
    _check_merged(rows, case, ref)
    _check_merged(maxima, case, ref)
    assert torch.equal(maxima.stage_max, rows.row_cursor.amax(0))
    assert maxima.width() == rows.width() == ref[0].shape[1] < 8 + 16 + 12 + 5 + 9 + 1   # the cut is a real one
    for a, b in zip(maxima.cut()[:3] + tuple(maxima.cut()[3].values()), rows.cut()[:3] + tuple(rows.cut()[3].values())):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    auto = _device(*case)
    assert auto.stage_max is None and torch.equal(auto.row_cursor, rows.row_cursor)   # the default rule: per row up to 4096 rows


def _tall_case():
    """nq = 4097 (above the 4096-row switch to cursor maxima), kl 3, engines of 4 and 3, ids from a pool of 12.  Ordinary rows end
    their lists with a pad, so their cursors are at most 4 after the first engine and 6 after the second; row 2048 alone sets the
    first maximum (5, then 5: its second engine repeats earlier ids), row 4096 - all ids distinct - alone the last (4, then 7)."""
    nq = 4097
    rng = np.random.default_rng(4097)
    l_idx = rng.integers(0, 12, size=(nq, 3)).astype(np.int64)
    d_idx = rng.integers(0, 12, size=(nq, 4)).astype(np.int64)
    s_idx = rng.integers(0, 12, size=(nq, 3)).astype(np.int64)
    l_idx[:, 2], d_idx[:, 2:], s_idx[:, 2] = -1, -1, -1
    l_idx[2048], d_idx[2048], s_idx[2048] = [0, 1, 2], [3, 0, 4, 3], [4, 1, 0]
    l_idx[4096], d_idx[4096], s_idx[4096] = [5, 6, -1], [7, 8, -1, -1], [9, 10, 11]
    d_scr = np.where(d_idx >= 0, rng.normal(size=d_idx.shape) * 3, -np.inf).astype(np.float32)
    s_scr = np.where(s_idx >= 0, rng.normal(size=s_idx.shape) * 3, -np.inf).astype(np.float32)
    l_lbl = np.where(l_idx >= 0, rng.integers(0, 2, size=l_idx.shape), 0).astype(np.int64)
    noise = rng.exponential(size=(nq, 11)).astype(np.float32)
    return (l_idx, l_lbl, {"dense": (d_idx, d_scr), "sparse": (s_idx, s_scr)}, {"dense": 1.0, "sparse": 0.5}), noise


def test_tall_batch_takes_the_maxima_path_to_the_sampler():
    from oracle import sampling as osmp
    from vod_amd.core.collate import sample_merged_on_device

    case, noise = _tall_case()
    ref = _oracle(*case)
    merged = _device(*case)
    assert merged.row_cursor is None and merged.stage_max is not None   # the auto rule
    assert merged.stage_max.tolist() == [5, 7, 0, 0]
    _check_merged(merged, case, ref)
    m_idx, m_scr, m_lbl, m_raw = ref
    w = m_idx.shape[1]
    assert w == 8   # min(5 + 1, 3 + 4) = 6, then min(7 + 1, 6 + 3): both maxima bind, and they differ
    kw = dict(total=4, max_pos_sections=1)
    want = osmp.sample_search_results(m_idx, m_scr, m_lbl, m_raw, noise[:, :w], 4, 1)
    out = sample_merged_on_device(merged, _t(noise), **kw)
    _check_sampled(out, want, ("dense", "sparse"), TOL_RANDOM)
    given = sample_merged_on_device(merged, _t(noise), width=w, **kw)
    for f in ("indices", "scores", "labels", "log_weights", "lse_pos", "lse_neg", "max_sampling_id", "local_ids"):
        a, b = getattr(out, f), getattr(given, f)
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), f
    for n in ("dense", "sparse"):
        assert torch.equal(out.raw_scores[n].view(torch.int32), given.raw_scores[n].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------------
# C-ABI shapes the Python wrapper never produces
# ---------------------------------------------------------------------------------------------------------------------------------
SENT_I, SENT_F = -770077, -1.25e30


class _Abi:
    """`vodhip_merge_hybrid` as `merge_hybrid_device` calls it, every output pre-filled with a sentinel and one guard row longer."""

    def __init__(self, case, *, extra=1, lbl_in=True, lbl_out=True, raw=None, width=False, rows=False, nq=None, width_buf=None):
        from vod_amd import _native

        l_idx, l_lbl, engs, weights = case
        self.native = _native
        self.names = list(engs)
        self.nq = l_idx.shape[0] if nq is None else nq
        alloc = l_idx.shape[0] + 1
        self.kl = l_idx.shape[1]
        self.ks = [engs[n][0].shape[1] for n in self.names]
        self.W = self.kl + sum(self.ks)
        self.stride = self.W + extra
        self.keep = [_t(l_idx), _t(l_lbl), [_t(engs[n][0]) for n in self.names], [_t(engs[n][1]) for n in self.names]]
        full_i = lambda: torch.full((alloc, self.stride), SENT_I, dtype=torch.int64, device="cuda")     # noqa: E731
        full_f = lambda: torch.full((alloc, self.stride), SENT_F, dtype=torch.float32, device="cuda")   # noqa: E731
        self.idx, self.scr = full_i(), full_f()
        self.lbl = full_i() if lbl_out else None
        raw = [True] * len(self.names) if raw is None else raw
        self.raw = [full_f() if on else None for on in raw]
        self.width = width_buf if width_buf is not None else (torch.full((8,), SENT_I, dtype=torch.int32, device="cuda") if width else None)
        self.rows = torch.full((alloc, 4), SENT_I, dtype=torch.int32, device="cuda") if rows else None
        n_e, VP = len(self.names), ctypes.c_void_p
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        self.args = [
            ptr(self.keep[0]), ptr(self.keep[1]) if lbl_in else None, self.kl, n_e,
            (VP * max(n_e, 1))(*[t.data_ptr() for t in self.keep[2]]), (VP * max(n_e, 1))(*[t.data_ptr() for t in self.keep[3]]),
            (ctypes.c_int * max(n_e, 1))(*self.ks), (ctypes.c_float * max(n_e, 1))(*[float(weights[n]) for n in self.names]), self.nq,
            ptr(self.idx), ptr(self.scr), ptr(self.lbl), (VP * max(n_e, 1))(*[ptr(t) for t in self.raw]), self.stride,
            ptr(self.width), ptr(self.rows), _native.current_stream_ptr(self.idx.device),
        ]

    def call(self):
        status = self.native.load_library().vodhip_merge_hybrid(*self.args)
        torch.cuda.synchronize()
        return status

    def check(self, case, ref, lbl_in=True):
        """Rows [0, nq) carry the oracle's batch, pad columns up to the stride; the rows beyond stay as they were."""
        n = self.nq
        idx, scr, lbl, raw = _full_stride(case, ref, self.stride, lbl_in)
        _eq(self.idx.cpu().numpy()[:n], idx[:n])
        _eq(self.scr.cpu().numpy()[:n], scr[:n])
        if self.lbl is not None:
            _eq(self.lbl.cpu().numpy()[:n], lbl[:n])
        for name, t in zip(self.names, self.raw):
            if t is not None:
                _eq(t.cpu().numpy()[:n], raw[name][:n])
        for t in (self.idx, self.lbl):
            assert t is None or bool((t[n:] == SENT_I).all())
        for t in (self.scr, *self.raw):
            assert t is None or bool((t[n:] == SENT_F).all())


@pytest.fixture(scope="module")
def abi_case():
    case = _random_case(np.random.default_rng(99), 5, 6, [9, 4, 7], 30, pad_frac=0.0)
    case[0][1, 2], case[1][1, 2] = -1, 2                      # an interior -1 with a label ...
    case[2]["e0"][0][1, 3], case[2]["e0"][1][1, 3] = -1, 0.5  # ... and one with a finite score: what the pad columns report
    case[0][3, 4:], case[1][3, 4:] = -1, 0                    # ordinary pads at the end of a list
    case[2]["e2"][0][3, 2:], case[2]["e2"][1][3, 2:] = -1, -np.inf
    return case, _oracle(*case)


def _cursors(ref_case):
    """Per-row cursors after every engine, restated: distinct non-negative ids among the first segments."""
    l_idx, _, engs, _ = ref_case
    out = np.zeros((l_idx.shape[0], len(engs)), dtype=np.int32)
    for r in range(l_idx.shape[0]):
        seen = {int(i) for i in l_idx[r] if i >= 0}
        for e, (idx, _) in enumerate(engs.values()):
            seen |= {int(i) for i in idx[r] if i >= 0}
            out[r, e] = len(seen)
    return out


def test_abi_optional_outputs(abi_case):
    case, ref = abi_case
    a = _Abi(case, lbl_out=False)
    assert a.call() == 0
    a.check(case, ref)
    a = _Abi(case, lbl_in=False)   # no labels to look up: every label, pads included, is -1
    assert a.call() == 0
    a.check(case, ref, lbl_in=False)
    a = _Abi(case, raw=[True, False, True])
    assert a.call() == 0
    a.check(case, ref)


def test_abi_wider_stride_and_both_cursor_outputs(abi_case):
    case, ref = abi_case
    a = _Abi(case, extra=9, width=True, rows=True)
    assert a.call() == 0
    a.check(case, ref)
    cur = _cursors(case)
    n_e = cur.shape[1]
    rows, width = a.rows.cpu().numpy(), a.width.cpu().numpy()
    _eq(rows[: a.nq, :n_e], cur)
    assert (rows[: a.nq, n_e:] == SENT_I).all() and (rows[a.nq:] == SENT_I).all()
    _eq(width[:4], np.concatenate([cur.max(0), np.zeros(4 - n_e, np.int32)]))
    assert (width[4:] == SENT_I).all()


def test_abi_maxima_do_not_remember_the_previous_batch(abi_case):
    case, ref = abi_case
    wide = _Abi(case, width=True)
    assert wide.call() == 0
    first = wide.width.cpu().numpy()[:3].copy()
    l_idx, l_lbl, engs, weights = case
    narrow_case = (l_idx[:2, :2], l_lbl[:2, :2], {n: (i[:2, :3], s[:2, :3]) for n, (i, s) in engs.items()}, weights)
    narrow = _Abi(narrow_case, width_buf=wide.width)
    assert narrow.call() == 0
    narrow.check(narrow_case, _oracle(*narrow_case))
    second = narrow.width.cpu().numpy()
    _eq(second[:3], _cursors(narrow_case).max(0))
    assert (second[:3] < first).all() and second[3] == 0 and (second[4:] == SENT_I).all()


def test_abi_empty_batch_clears_the_maxima_and_nothing_else(abi_case):
    case, _ = abi_case
    a = _Abi(case, nq=0, width=True, rows=True)
    assert a.call() == 0
    assert a.width.tolist() == [0, 0, 0, 0] + [SENT_I] * 4
    assert bool((a.rows == SENT_I).all()) and bool((a.idx == SENT_I).all()) and bool((a.lbl == SENT_I).all())
    assert all(bool((t == SENT_F).all()) for t in (a.scr, *a.raw))


def test_abi_refuses_width_4097_and_the_next_call_works(abi_case):
    case, ref = abi_case
    l_idx = np.zeros((1, 4096), dtype=np.int64)
    over = (l_idx, np.ones_like(l_idx), {"e0": (np.ones((1, 1), np.int64), np.zeros((1, 1), np.float32))}, {"e0": 1.0})
    a = _Abi(over)
    assert a.W == 4097 and a.call() != 0
    assert b"4096" in a.native.load_library().vodhip_last_error()
    assert bool((a.idx == SENT_I).all()) and bool((a.scr == SENT_F).all())
    b = _Abi(case)
    assert b.call() == 0
    b.check(case, ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# run to run
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["degenerate_rows", "W4095"])
def test_repeated_launches_are_bit_identical(which):
    case = _degenerate_batch(DEGENERATE, 5) if which == "degenerate_rows" else _width_case(4095, True)
    ins = (_t(case[0]), _t(case[1]), {n: (_t(i), _t(s)) for n, (i, s) in case[2].items()}, case[3])
    from vod_amd.core.merge import merge_hybrid_device

    def run():
        m = merge_hybrid_device(*ins, cursors="per_row")
        n_e = len(m.engine_k)
        outs = [m.indices, m.scores.view(torch.int32), m.labels, m.row_cursor[:, :n_e]] + [r.view(torch.int32) for r in m.raw.values()]
        return [o.cpu().numpy() for o in outs]

    first = run()
    for _ in range(4):
        for a, b in zip(first, run()):
            assert np.array_equal(a, b)
    ref = _oracle(*case)
    _eq(first[0][:, : ref[0].shape[1]], ref[0])
