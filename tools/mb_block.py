#!/usr/bin/env python3
"""Block-operator microbenchmark: per-product time of the native lo_block_mv_f32 (csrc/lo_block.hip) against the
composition of the reference's algorithm on the same GPU, written here from ATen `permute().contiguous()` / `sum` and
the existing `K.matvec` on the same descriptor (independent of the operator classes), on device events after warm-up.
The two are timed alternately in `--rounds` rounds; the table gives the median and the spread (min .. max) of each.

Shapes: interleaved low-rank (T 4, n 8192, R 32), interleaved dense (T 4, n 4096), sum dense (T 16, n 4096); c = 1, 17.
Usage:  python tools/mb_block.py [--reps 20] [--rounds 5] [--shapes a,b] [--cols 1,17]    Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linear_operator_amd import kernels as K  # noqa: E402

H = K._hip
SHAPES = {
    "interleaved_lowrank": dict(layout=H.LO_BLOCK_INTERLEAVED, T=4, n=8192, R=32),
    "interleaved_dense": dict(layout=H.LO_BLOCK_INTERLEAVED, T=4, n=4096, R=0),
    "sum_dense": dict(layout=H.LO_BLOCK_SUM, T=16, n=4096, R=0),
    "sum_lowrank": dict(layout=H.LO_BLOCK_SUM, T=16, n=8192, R=32),  # (beyond the three headline shapes: routing only)
}
HEADLINE = "interleaved_lowrank,interleaved_dense,sum_dense"


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def composition(desc, layout, T, n, v):
    """The reference's product: the vectors moved into the batch of the base operator, one batched product, and back."""
    c = v.shape[-1]
    if layout == H.LO_BLOCK_SUM:
        return K.matvec(desc, v.unsqueeze(0).expand(T, n, c).contiguous()).sum(0)
    cols = v.reshape(n, T, c).permute(1, 0, 2).contiguous()
    return K.matvec(desc, cols).permute(1, 0, 2).contiguous().reshape(n * T, c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=HEADLINE)
    ap.add_argument("--cols", default="1,17")
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in args.shapes.split(","):
        s = SHAPES[name]
        T, n, R, layout = s["T"], s["n"], s["R"], s["layout"]
        if R:
            desc = K.lowrank_diag_descriptor(torch.randn(T, n, R, device="cuda", generator=g) / R ** 0.5, None)
            op_bytes = 4 * T * n * R
        else:
            desc = K.dense_diag_descriptor(torch.randn(T, n, n, device="cuda", generator=g) / n ** 0.5, None)
            op_bytes = 4 * T * n * n
        for c in (int(k) for k in args.cols.split(",")):
            rows = n if layout == H.LO_BLOCK_SUM else n * T
            v = torch.randn(rows, c, device="cuda", generator=g)
            nat_fn = lambda: K.block_matvec(desc, layout, T, v)  # noqa: E731
            ref_fn = lambda: composition(desc, layout, T, n, v)  # noqa: E731
            yr = ref_fn()
            err = float((nat_fn() - yr).abs().max() / yr.abs().max())
            for _ in range(3):
                nat_fn(), ref_fn()
            torch.cuda.synchronize()
            nat, ref = [], []
            for _ in range(args.rounds):  # alternate: both see the same state of the machine
                nat.append(timed(nat_fn, args.reps))
                ref.append(timed(ref_fn, args.reps))
            mn, mr = statistics.median(nat), statistics.median(ref)
            print(json.dumps(dict(shape=name, T=T, n=n, R=R, c=c, native_us=round(mn, 1),
                                  native_spread=[round(min(nat), 1), round(max(nat), 1)], composition_us=round(mr, 1),
                                  composition_spread=[round(min(ref), 1), round(max(ref), 1)],
                                  speedup=round(mr / mn, 2), faster_beyond_spread=bool(max(nat) < min(ref)),
                                  native_gbs=round((op_bytes + 8 * rows * c) / mn / 1e3, 1), max_rel_diff=err)),
                  flush=True)


if __name__ == "__main__":
    main()
