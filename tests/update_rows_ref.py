"""NumPy restatement of `update_rows` / `add_to_rows` (include/vodhip.h H2u).

It decides WHICH slot writes which row and WHAT float32 value the row gets.  It does not round to the store dtype or form bias
columns or row statistics: the expected store is a fresh index built by `add` - the ingest path, not the code under test - from the
matrix this returns.  For ADD on a 16-bit store the matrix handed in is `stored_rows().float()`, the master copy there.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class Counts(NamedTuple):
    written: int
    skipped: int
    duplicates: int


def resolve_slots(ids, ntotal: int, id_base: int = 0) -> tuple[dict[int, int], Counts]:
    """`{row: slot}` of the slots that write, and the three counts.  A slot whose id is negative, below `id_base` or not below
    `id_base + ntotal` is skipped; of the slots that list one row the LAST writes, the others are duplicates."""
    winner: dict[int, int] = {}
    skipped = duplicates = 0
    for j, i in enumerate(np.asarray(ids, dtype=np.int64).reshape(-1).tolist()):
        row = i - id_base
        if i < 0 or row < 0 or row >= ntotal:
            skipped += 1
            continue
        if row in winner:
            duplicates += 1
        winner[row] = j
    return winner, Counts(len(winner), skipped, duplicates)


def apply_update(x: np.ndarray, rows: np.ndarray, ids=None, begin: int = 0, mode: str = "set", alpha: float = 1.0,
                 id_base: int = 0) -> tuple[np.ndarray, Counts]:
    """The float32 matrix after the update and the counts.  `x` is float32 `[ntotal, dim]` (not modified), `rows` `[n, dim]` of any
    float dtype (widened to float32, exactly).  ADD is two float32 roundings: p = alpha * rows, then x + p - no fused multiply-add."""
    assert mode in ("set", "add")
    x = np.array(x, dtype=np.float32, copy=True)
    rows = np.asarray(rows).astype(np.float32)
    n = rows.shape[0]
    if ids is None:
        assert 0 <= begin and begin + n <= x.shape[0], "row range out of bounds"
        winner = {begin + j: j for j in range(n)}
        counts = Counts(n, 0, 0)
    else:
        assert len(np.asarray(ids).reshape(-1)) == n
        winner, counts = resolve_slots(ids, x.shape[0], id_base)
    if not winner:
        return x, counts
    r = np.fromiter(winner.keys(), dtype=np.int64, count=len(winner))
    j = np.fromiter(winner.values(), dtype=np.int64, count=len(winner))
    with np.errstate(all="ignore"):
        if mode == "set":
            x[r] = rows[j]
        else:
            p = (np.float32(alpha) * rows[j]).astype(np.float32)
            x[r] = (x[r] + p).astype(np.float32)
    return x, counts
