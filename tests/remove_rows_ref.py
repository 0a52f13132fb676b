"""NumPy restatement of `remove_rows` (include/vodhip.h H2r): which rows leave, what is skipped, what counts as a duplicate, and
where every old row ends up.  Shared by tests/test_remove_rows_cpu.py and tests/test_remove_rows_gpu.py."""
from __future__ import annotations

import numpy as np


def resolve_removal(ntotal: int, ids=None, begin: int = 0, n: int | None = None, id_base: int = 0):
    """-> (keep [ntotal] bool, (removed, skipped, duplicates)).  Listed form: a slot whose id is negative, below `id_base` or not below
    `id_base + ntotal` is skipped; a row listed more than once leaves once, its other slots are duplicates.  Range form: rows
    `begin .. begin + n` leave."""
    keep = np.ones(ntotal, dtype=bool)
    if ids is None:
        assert 0 <= begin and begin + n <= ntotal
        keep[begin:begin + n] = False
        return keep, (int(n), 0, 0)
    skipped = duplicates = 0
    for i in (int(v) for v in np.asarray(ids).reshape(-1)):
        row = i - id_base
        if i < 0 or row < 0 or row >= ntotal:
            skipped += 1
        elif not keep[row]:
            duplicates += 1
        else:
            keep[row] = False
    return keep, (int((~keep).sum()), skipped, duplicates)


def new_ids(keep: np.ndarray) -> np.ndarray:
    """the new id of every old row: its old id minus the removed rows below it; -1 for a removed row"""
    out = np.cumsum(keep).astype(np.int64) - 1
    out[~keep] = -1
    return out
