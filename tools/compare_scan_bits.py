#!/usr/bin/env python3
"""Do two builds of libvodhip.so give the same bits in the five scans that share vod_amd/csrc/scan_contract.h?

Run once per library, a fresh process each (`VODHIP_LIB=<path>` selects the library; without it the package's own), then `cmp` the
two files.  The run builds seeded stores and appends, as raw bytes and in a fixed order, every output tensor of
  posterior_mean                      (mean, max_score, log_rel)
  posterior_expectation               (values, max_score, log_rel)
  posterior_expectation_backward      (the backward of expected_values)
  posterior_adjoint
  key_gradient                        with grad_log_z only, with grad_values only, and with both
to ONE file.  The shapes are the smallest that reach every instantiation and every loop boundary of those kernels - not workload
shapes; the whole run takes seconds:
  rows     20,557 = 16,384 + 4,096 + 77: a second posterior group, a sixth read-out group, a last tile partial at 256 and at 64 rows
  dim      64 .. 448: 1 - 4 slices; a full chunk + a remainder of 1 for the 4-slice and the 3-slice chunking (320, 256), a remainder of
           2 for the 3-slice one (320), of 3 for the 4-slice one (448)
  columns  5, 70, 130, 256: c_pad 64 / 128 / 192 / 256
  queries  70 (a partial 64-query tile) and 300 (a second 256-query tile for the kernels that exchange the operands)
  dtype    fp16 and bf16; with and without subset labels that allow two of four row labels; beta = dim^-1/2
  NaN      one stored row holds a NaN in one column: its propagation is documented behaviour
Every value of every axis appears with both dtypes and both subset settings; the cross product is not taken.
usage: [VODHIP_LIB=...] python tools/compare_scan_bits.py --out FILE"""
import argparse
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from vod_amd.index import HipFlatIndex  # noqa: E402

ROWS = 16_384 + 4_096 + 77
# (dim, value columns, queries)
CASES = [(64, 5, 70), (128, 70, 300), (192, 130, 70), (256, 256, 300), (320, 256, 300), (448, 130, 70)]
NAN_ROW, NAN_COL = 4_321, 3


def run_case(f, dim, n_cols, nq, dtype, subset, gen):
    dev = torch.device("cuda", 0)
    x = torch.randn((ROWS, dim), generator=gen).to(dtype)
    x[NAN_ROW, NAN_COL] = float("nan")
    table = torch.randn((ROWS, n_cols), generator=gen).to(dtype)
    q = torch.randn((nq, dim), generator=gen)
    g = torch.randn((nq, n_cols), generator=gen) * 1e-3
    a = torch.randn((nq,), generator=gen) * 1e-3
    t = float(dim) ** 0.5
    n_bytes = n_nonfinite = 0

    def put(*tensors):
        nonlocal n_bytes, n_nonfinite
        torch.cuda.synchronize()
        for ten in tensors:
            n_nonfinite += int((~torch.isfinite(ten)).sum())
            raw = ten.detach().contiguous().cpu().numpy().tobytes()
            f.write(raw)
            n_bytes += len(raw)

    with HipFlatIndex(dim, ROWS, dtype=dtype, device=0) as ix:
        ix.add(x.to(dev))
        ix.set_row_values(table.to(dev))
        sub = None
        if subset:
            ix.set_row_labels(torch.arange(ROWS, dtype=torch.int32) % 4)
            sub = torch.tensor([[0, 2]], dtype=torch.int32).repeat(nq, 1).to(dev)
        qd, gd, ad = q.to(dev), g.to(dev), a.to(dev)
        pm = ix.posterior_mean(qd, temperature=t, subset=sub)
        put(pm.mean, pm.log_partition.max_score, pm.log_partition.log_rel)
        pe = ix.posterior_expectation(qd, temperature=t, subset=sub)
        put(pe.values, pe.log_partition.max_score, pe.log_partition.log_rel)
        put(ix.posterior_expectation_backward(qd, gd, pe, temperature=t, subset=sub))
        put(ix.posterior_adjoint(qd, gd, pe.log_partition, temperature=t, subset=sub))
        put(ix.key_gradient(qd, grad_log_z=ad, log_partition=pe.log_partition, temperature=t, subset=sub))
        put(ix.key_gradient(qd, grad_values=gd, expectation=pe, temperature=t, subset=sub))
        put(ix.key_gradient(qd, grad_log_z=ad, grad_values=gd, expectation=pe, temperature=t, subset=sub))
    return n_bytes, n_nonfinite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compare_scan_bits.py needs the GPU")
    gen = torch.Generator().manual_seed(20_557)  # (on the host: the same inputs in every process)
    total = 0
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, "wb") as f:
        for dtype in (torch.float16, torch.bfloat16):
            for subset in (False, True):
                for dim, n_cols, nq in CASES:
                    n, bad = run_case(f, dim, n_cols, nq, dtype, subset, gen)
                    total += n
                    print(f"{str(dtype).split('.')[-1]} subset={int(subset)} dim {dim} cols {n_cols} nq {nq}: {n} bytes, {bad} elements not finite", flush=True)
    print(f"{out}: {total} bytes")


if __name__ == "__main__":
    main()
