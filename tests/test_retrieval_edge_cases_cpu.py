"""CPU checks on the case tables of tests/test_gradients_edges_gpu.py: every launch branch the GPU module is there for is hit by a
row and by a 16-bit row (recomputed from a restatement of the host-side launch arithmetic), and the float64 oracle alone is finite in
at least 95 % of every array a case compares."""
import pytest

import retrieval_edge_cases as rc


def test_the_restatement_knows_the_shapes_the_launch_code_documents():
    assert {"fwd:split_full", "dq:split_full"} <= rc.launch_labels(64, 2048, 768)       # 4 slabs of 192; 16 of 128
    assert "fwd:split_empty_slab" in rc.launch_labels(64, 512, 520)                     # slabs of 192: slab 3 starts at 576
    assert "fwd:split_empty_slab" not in rc.launch_labels(64, 512, 512)
    assert "dq:split_empty_slab" in rc.launch_labels(1, 512, 520)                       # 16 splits of 64, 8 empty
    assert {"dq:split_empty_slab", "dq:split_ragged"} <= rc.launch_labels(65, 513, 513)  # 7 splits of 128: 4 full, 1 column, 2 empty
    assert "dq:unsplit_ratio" in rc.launch_labels(300, 512, 512) and "dq:unsplit_small_d" in rc.launch_labels(64, 511, 511)
    assert "fwd:unsplit" in rc.launch_labels(64, 511, 511) and "fwd:split_ragged" in rc.launch_labels(300, 512, 1030)
    assert "fwd.q:scalar_by_pitch" in rc.launch_labels(64, 512, 510) and "fwd.q:vector_then_partial_k" in rc.launch_labels(64, 513, 516)
    assert "ds.dST:scalar_by_pitch" in rc.launch_labels(64, 513, 516) and "ds.dST:vector" in rc.launch_labels(64, 64, 64)


@pytest.mark.parametrize("table", ["fp32", "16bit"])
def test_every_named_branch_is_hit(table):
    rows = rc.CASES_2D if table == "fp32" else rc.CASES_2D_16BIT
    hit = set().union(*(rc.launch_labels(B, D, H) for B, D, H, _why in rows))
    missing = [label for label in rc.REQUIRED_LABELS if label not in hit]
    assert not missing, missing
    if table == "16bit":  # a row whose q AND s operands of all three GEMMs take the 16-bit vector unpack
        assert any({"fwd.q:vector", "fwd.s:vector", "dq.s:vector", "ds.q:vector"} <= rc.launch_labels(B, D, H) and B >= 64 and D >= 64
                   for B, D, H, _why in rows)


def test_the_tables_hold_every_edge_value():
    b, d, h = (set(col) for col in list(zip(*rc.CASES_2D))[:3])
    assert {1, 63, 64, 65, 130} <= b and {1, 63, 65, 511, 512, 513, 1001, 2048, 4100, 16384} <= d
    assert {1, 2, 63, 65, 510, 511, 512, 513, 516, 520, 768, 1024, 1030} <= h
    b, d, h = (set(col) for col in list(zip(*rc.CASES_3D))[:3])
    assert {1, 5, 64} <= b and {1, 3, 255, 256, 257, 1000} <= d and {1, 63, 65, 1024} <= h


@pytest.mark.parametrize("aux", [False, True])
def test_the_oracle_is_finite_in_95_percent_of_every_compared_array(aux):
    """No case passes by masking: the only elements left out of a comparison are the float64 oracle's own NaN / inf (padded scores)."""
    cases = [dict(B=B, D=D, H=H) for B, D, H, _ in rc.CASES_2D] + [dict(B=B, D=D, H=H, three_d=True) for B, D, H, _ in rc.CASES_3D]
    cases += [dict(B=B, D=D, H=H, dtype=dt) for B, D, H, _ in rc.CASES_2D_16BIT for dt in ("float16", "bfloat16")]
    cases += [dict(B=B, D=D, H=H, three_d=True, dtype=dt) for B, D, H, _ in rc.CASES_3D for dt in ("float16", "bfloat16")]
    for three_d in (False, True):  # the row edges at the split shapes, D = 1, large logits, the misaligned-view shapes
        B, D, H = (64, 32, 768) if three_d else (64, 2048, 768)
        cases += [dict(B=B, D=D, H=H, three_d=three_d, edge=e) for e in ("padrow", "onelive", "tie")]
        cases += [dict(B=B, D=D, H=H, three_d=three_d, q_scale=20.0), dict(B=64, D=1, H=768, three_d=three_d)]
        if not aux:
            cases.append(dict(B=B, D=D, H=H, three_d=three_d, edge="nopos"))
    if aux:
        cases += [dict(B=64, D=32, H=768, three_d=True, dtype=dt, edge="padrow") for dt in ("float16", "bfloat16")]
        cases += [dict(B=64, D=512, H=520), dict(B=65, D=513, H=516)]
        cases += [dict(B=B, D=D, H=H, three_d=td, dtype=dt) for td, B, D, H in ((False, 64, 128, 128), (False, 65, 513, 516), (True, 5, 64, 64))
                  for dt in ("float32", "float16")]
    else:
        cases += [dict(B=64, D=300, H=256), dict(B=65, D=513, H=520)]  # the plain entry point's
    for kw in cases:
        _x, r64, _r32 = rc.reference(aux=aux, **kw)
        low = {k: v for k, v in rc.finite_share(r64).items() if v < 0.95}
        assert not low, (kw, low)
