"""The case tables of tests/test_gradients_edges_gpu.py, their seeded inputs, and a host-only restatement of the launch arithmetic of
`vod_amd/csrc/kernels_retrieval.hip` that says which branch each row runs.  NumPy only: tests/test_retrieval_edge_cases_cpu.py checks
on the CPU that every branch the GPU module is there for is hit by a row, and by a 16-bit row."""
from __future__ import annotations

import functools

import numpy as np

AUX = dict(guidance="sparse", guidance_weight=0.2, self_supervision_weight=0.3, score_decay=0.01)
UPSTREAM = 2.5  # d(loss * UPSTREAM): the backward kernels' alpha is not 1

# (B, D, H, why the row is there).  B in {1, 63, 64, 65, 130}, D in {1, 63, 65, 511, 512, 513, 1001, 2048, 4100},
# H in {1, 2, 63, 65, 510, 511, 512, 513, 516, 520, 768, 1024, 1030}: every value appears, not their product.
CASES_2D = [
    (1, 1, 1, "one element: every tile is an edge tile"),
    (1, 512, 520, "dq: 16 splits of 64, 8 empty; forward: slab 3 starts beyond K"),
    (63, 63, 63, "one below the tile in M, N and K"),
    (64, 65, 65, "one above the tile in N and K: scalar edge tiles after a full one"),
    (65, 63, 2, "M one above the tile, K = 2 (one MFMA step)"),
    (64, 64, 64, "exactly one interior tile everywhere: vector staging of all six operands, nothing else"),
    (65, 513, 513, "dq: 7 splits of 128 (4 full, one of a single column, 2 empty); scalar by pitch H; dS^T pitch 513"),
    (64, 2048, 768, "the training shape: dq 16 full splits, forward 4 full slabs of 192"),
    (300, 512, 512, "dq: D / B < 2 gives no split; forward 4 full slabs; 5 tiles of M"),
    (64, 511, 511, "dq: D < 512 gives no split; forward: H < 512 unsplit; odd pitches"),
    (130, 1001, 516, "vector tiles followed by a partial K tile (516 = 8 * 64 + 4); dS^T pitch 1001"),
    (64, 512, 510, "scalar by pitch (510 % 4 = 2) at full tiles; forward unsplit"),
    (130, 65, 520, "forward slab 3 empty with 3 tiles of M"),
    (63, 2048, 1030, "forward: 3 slabs of 320 and one of 70; dq 16 splits with M < 64"),
    (64, 4100, 512, "D = 4100: 65 tiles of N; dq 12 slabs of 320, one of 260, 3 empty"),
    (65, 1001, 1024, "forward 4 full slabs of 256; dq 15 splits over an odd pitch"),
    (130, 511, 513, "H = 513: forward slabs of 192, 192, 129 and an empty one; all scalar by pitch"),
    (1, 4100, 63, "one query row against many sections, K below the tile"),
    (63, 512, 1024, "dq 8 splits of 64 with M < 64"),
    (64, 513, 516, "dS^T pitch 513 with vector tiles of q and s followed by a partial K tile"),
    (130, 2048, 65, "dq 15 splits of 192 (the last 4 empty: 11 * 192 >= 2048) with 3 tiles of M"),
    (65, 65, 1030, "forward ragged slabs with one-above-the-tile M and N"),
    (64, 1, 768, "D = 1 under a split forward"),
    (1, 63, 511, "B = 1, all below the tile, forward unsplit at 511"),
    (130, 512, 1, "H = 1: K = 1 in the forward, N = 1 in both backward GEMMs"),
    (63, 1001, 2, "H = 2 with an odd dS^T pitch"),
    (65, 2048, 520, "forward slab 3 empty at the in-batch width; dq 16 splits of 128"),
    (64, 512, 512, "the smallest shape that splits both ways with full slabs"),
    (64, 63, 768, "forward split with N below the tile"),
    (2, 16384, 65, "the largest D the entry point takes"),
]
# the 16-bit subset: every group of labels above again, in fp16 and in bf16; (64, 2048, 512) and (64, 64, 64) have B, D, H >= 64 and
# H % 4 == 0, so both operands of all three GEMMs take the 16-bit vector path
CASES_2D_16BIT = [
    (1, 512, 520, "dq 16 splits, 8 empty; forward slab 3 empty"),
    (65, 513, 513, "dq 7 splits; scalar by pitch; dS^T pitch 513"),
    (64, 2048, 512, "dq 16 full splits; forward 4 full slabs; every operand on the vector path"),
    (300, 512, 1030, "dq D / B < 2; forward ragged slabs"),
    (64, 511, 511, "dq D < 512; forward unsplit"),
    (130, 1001, 516, "vector tiles followed by a partial K tile; dS^T pitch 1001"),
    (64, 64, 64, "one interior tile: the 16-bit vector unpack alone"),
]
# B in {1, 5, 64}, D in {1, 3, 255, 256, 257, 1000}, H in {1, 63, 65, 1024}: the row kernels' strides of 256 threads / 64 lanes
CASES_3D = [
    (1, 1, 1, "one element"),
    (5, 3, 63, "fewer sections than waves, H one below the wave"),
    (5, 255, 65, "D one below the workgroup, H one above the wave"),
    (1, 256, 1024, "D = the workgroup"),
    (64, 257, 63, "D one above the workgroup"),
    (5, 1000, 65, "four strides of D, the last partial"),
    (64, 3, 1024, "the training batch, few sections"),
    (64, 256, 1, "H = 1"),
]


def launch_labels(B: int, D: int, H: int) -> set[str]:
    """Restatement of launch_retrieval_forward / _backward / launch_small_gemm / stage_vec's `vec_ok` for 2-D sections through the
    wrapper (4-slab workspace).  Of `vec_ok`'s conditions, `c0 % 4 == 0` always holds (c0 is a multiple of 64), so an operand
    [R rows, C unit-stride columns, pitch P] has vector tiles iff P % 4 == 0 and R >= 64 and a 64-wide column tile fits in a slab."""
    def slabs(K, n):  # lengths of the n split-K slabs
        per = -(-(-(-K // n)) // 64) * 64
        return [max(0, min(K, (z + 1) * per) - z * per) for z in range(n)]

    def split_labels(tag, lens):
        kinds = (["split_empty_slab"] if 0 in lens else []) + (["split_ragged"] if any(0 < x < lens[0] for x in lens) else [])
        return {f"{tag}:{k}" for k in (kinds or ["split_full"])}

    def stage(tag, R, C, P, lens):  # lens: the slab lengths when C is the K dimension, else None
        vec = P % 4 == 0 and R >= 64 and (max(lens) >= 64 if lens else C >= 64)
        out = {f"{tag}:vector" if vec else f"{tag}:scalar"}
        if not vec and P % 4 and R >= 64 and C >= 64:
            out.add(f"{tag}:scalar_by_pitch")
        if vec and lens and any(x % 64 for x in lens):
            out.add(f"{tag}:vector_then_partial_k")
        return out

    fwd = slabs(H, 4 if H >= 512 else 1)
    n_dq = min(16, D // max(B, 1))
    dq = slabs(D, 1 if (n_dq < 2 or D < 512) else n_dq)
    out = {"fwd:unsplit"} if len(fwd) == 1 else split_labels("fwd", fwd)
    out |= {"dq:unsplit_small_d" if D < 512 else "dq:unsplit_ratio"} if len(dq) == 1 else split_labels("dq", dq)
    out |= stage("fwd.q", B, H, H, fwd) | stage("fwd.s", D, H, H, fwd)          # A = q [B, H]; B = s [D, H], stored transposed
    out |= stage("dq.dS", B, D, D, dq) | stage("dq.s", D, H, H, None)           # A = dS [B, D] (k fast); B = s [D, H] (n fast)
    out |= stage("ds.dST", B, D, D, None) | stage("ds.q", B, H, H, None)        # A = dS^T, stored transposed; B = q [B, H]
    return out


# every branch named in the issue: each must be hit by one fp32 row and by one 16-bit row
REQUIRED_LABELS = [
    "fwd:unsplit", "fwd:split_full", "fwd:split_empty_slab", "fwd:split_ragged",
    "dq:split_empty_slab", "dq:split_ragged", "dq:split_full", "dq:unsplit_ratio", "dq:unsplit_small_d",
    "fwd.q:vector", "fwd.s:vector", "dq.dS:vector", "dq.s:vector", "ds.dST:vector", "ds.q:vector",
    "fwd.q:scalar_by_pitch", "fwd.s:scalar_by_pitch", "dq.s:scalar_by_pitch", "ds.q:scalar_by_pitch",
    "fwd.q:vector_then_partial_k", "fwd.s:vector_then_partial_k",
    "dq.dS:scalar_by_pitch", "ds.dST:scalar_by_pitch",
]


def round_to(x: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values of `x` rounded to fp16 / bf16 (round to nearest even), or `x` itself for fp32."""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "float32":
        return x
    if dtype == "float16":
        return x.astype(np.float16).astype(np.float32)
    bits = x.view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return bits.astype(np.uint32).view(np.float32)


def make_inputs(B, D, H, three_d=False, dtype="float32", aux=False, seed=0, q_scale=3.0, edge=None):
    """Seeded inputs.  At most 3 % pads (column 0 stays live), 5 % positives + column 0, 20 % NaN in the sparse / dense sampling scores; without
    the auxiliary terms one row has no positives (with them the reference's loss would be NaN by design).  `edge` in
    {padrow, onelive, tie, allpad, nopos} rewrites row B // 3 (or every row) the way the edge fixtures do."""
    rng = np.random.default_rng([B, D, H, int(three_d), seed])
    q = round_to(rng.normal(size=(B, H)) * (q_scale / np.sqrt(H)), dtype)
    s = round_to(rng.normal(size=((B, D, H) if three_d else (D, H))), dtype)
    score = rng.normal(size=(B, D)).astype(np.float32)
    pad = rng.uniform(size=(B, D)) < 0.03
    pad[:, 0] = False
    pad.reshape(-1)[np.flatnonzero(pad)[int(0.03 * B * D):]] = False  # never above 3 %: small shapes carry no pads (the fixtures do)
    rel = (rng.uniform(size=(B, D)) < 0.05).astype(np.int64)
    rel[:, 0] = 1
    if not aux and B > 2:
        rel[B // 2] = 0
    r = B // 3
    if edge == "padrow":
        pad[r] = True
    elif edge == "onelive":
        pad[r, 1:] = True
    elif edge == "allpad":
        pad[:] = True
    elif edge == "nopos":
        rel[:] = 0
    elif edge == "tie":
        a, b = (1, D - 1) if D > 2 else (0, D - 1)
        pad[r] = False
        rel[r] = 0
        rel[r, [a, b]] = 1
        score[r, b] = score[r, a]
        if three_d:
            s[r, b] = s[r, a]
        else:
            s[b] = s[a]
    score[pad] = -np.inf
    sparse = (rng.gamma(2.0, 2.0, size=(B, D)) - 6).astype(np.float32)
    sparse[rng.uniform(size=(B, D)) < 0.2] = np.nan
    dense = rng.normal(size=(B, D)).astype(np.float32)
    dense[rng.uniform(size=(B, D)) < 0.2] = np.nan
    return dict(q=q, s=s, score=score, relevance=rel, sparse=sparse, dense=dense)


@functools.lru_cache(maxsize=None)
def reference(B, D, H, three_d=False, dtype="float32", aux=False, seed=0, q_scale=3.0, edge=None):
    """(inputs, float64 oracle, float32 oracle) of one case: computed once, shared by the tests that need it, never modified."""
    from oracle.gradients import retrieval_gradients

    x = make_inputs(B, D, H, three_d, dtype, aux, seed, q_scale, edge)
    cfg = AUX if aux else {}
    r64 = retrieval_gradients(x["q"], x["s"], x["score"], x["relevance"], x["sparse"], x["dense"], **cfg)
    r32 = retrieval_gradients(x["q"], x["s"], x["score"], x["relevance"], x["sparse"], x["dense"], dtype=np.float32, **cfg)
    for d in (x, r64, r32):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return x, r64, r32


def compared_outputs(r: dict) -> dict[str, np.ndarray]:
    """The outputs a case compares: loss, every diagnostic the oracle produced, retriever_scores, dq, ds (gradients of loss * UPSTREAM)."""
    out = {k: np.asarray(v) for k, v in r.items() if k not in ("d_scores", "dq", "ds")}
    out["dq"] = UPSTREAM * np.asarray(r["dq"])
    out["ds"] = UPSTREAM * np.asarray(r["ds"])
    return out


def finite_share(r64: dict) -> dict[str, float]:
    return {k: float(np.isfinite(v).mean()) for k, v in compared_outputs(r64).items()}
