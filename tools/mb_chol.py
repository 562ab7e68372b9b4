#!/usr/bin/env python3
"""Exact small-N path microbenchmark: the native batched Cholesky and Cholesky solve (csrc/lo_chol.hip) against the
ATen route they replace, workarounds included (utils/cholesky.py with the native routing switched off), in one process
on one GPU: warm-up, device events over `--reps` launches per sample, median of `--samples` samples.

Each shape (B x N^2) is timed three ways: factor alone, factor + one-column solve, factor + 16-column solve.  The
factorisation also reports its effective bandwidth against the compulsory 2 B N^2 elements.  `--dtype float64` times
csrc/lo_chol_f64.hip against ATen float64 and adds the native float32 time of the same matrices from the same run;
for the single matrix, whose solve the routing leaves to ATen, `native_forced_us` is the native substitution.
Usage:  python tools/mb_chol.py [--reps 10] [--samples 5] [--dtype float64]    Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linear_operator_amd.functions import _cholesky as FC  # noqa: E402
from linear_operator_amd.utils import cholesky as UC  # noqa: E402

SHAPES = ((512, 128), (512, 256), (256, 320), (64, 512), (64, 600), (64, 800), (1, 800))


def timed_us(fn, reps, samples):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    args = ap.parse_args()
    dtype = getattr(torch, args.dtype)
    for B, N in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(N)
        X = torch.randn(B, N, 24, generator=g, device="cuda", dtype=dtype)
        A = X @ X.mT + 0.5 * torch.eye(N, device="cuda", dtype=dtype)
        rhs = {c: torch.randn(B, N, c, generator=g, device="cuda", dtype=dtype) for c in (1, 16)}
        A32, rhs32 = A.float(), {c: r.float() for c, r in rhs.items()}

        def run(c, A=A, rhs=rhs):
            L, _ = UC._cholesky_ex(A)
            if c:
                UC.cholesky_solve(rhs[c], L)

        for c, what in ((0, "factor"), (1, "factor+solve1"), (16, "factor+solve16")):
            native = timed_us(lambda: run(c), args.reps, args.samples)
            with mock.patch.object(FC, "native_ok", lambda *a, **k: False):
                aten = timed_us(lambda: run(c), args.reps, args.samples)
            rec = {"shape": f"{B}x{N}^2", "dtype": args.dtype, "what": what, "native_us": round(native, 1),
                   "aten_us": round(aten, 1), "speedup": round(aten / native, 2)}
            if dtype == torch.float64:  # the native float32 kernels on the same matrices, same run
                rec["native_f32_us"] = round(timed_us(lambda: run(c, A32, rhs32), args.reps, args.samples), 1)
            if c == 0:
                rec["native_GBps_of_compulsory"] = round(2 * B * N * N * A.element_size() / (native * 1e-6) / 1e9, 1)
            if c and B == 1:  # the unbatched solve stays on ATen by default: time the native substitution too
                name = "SINGLE_SOLVE_MAX_N" if dtype == torch.float32 else "SINGLE_SOLVE_MAX_N_F64"
                with mock.patch.object(FC, name, 1024):
                    rec["native_forced_us"] = round(timed_us(lambda: run(c), args.reps, args.samples), 1)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
