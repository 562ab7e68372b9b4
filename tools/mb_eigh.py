#!/usr/bin/env python3
"""Symmetric eigensolver microbenchmark: the native batched float64 eigensolver (csrc/lo_eigh_f64.hip) against ATen's
float64 torch.linalg.eigh / eigvalsh, in one process on one GPU: warm-up, device events over `--reps` launches per
sample, median of `--samples` samples.  Both go through functions/_eigh.py; the native route is forced by opening the
routing constants and ATen is reached by replacing `native_ok`, so the routing in force does not matter.

Each shape (B x N^2) is timed with vectors and eigenvalues-only.  `--calls` adds the whole-call timings of the
consumers (SumKroneckerLinearOperator.solve, set-up included, and the KroneckerProduct + ConstantDiag closed-form solve)
under the routing the package ships with; run it on two commits alternately to compare them.
Usage:  python tools/mb_eigh.py [--reps 10] [--samples 5] [--sweep | --calls]    Prints one JSON line per measurement.
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

SHAPES = ((256, 256), (128, 256), (64, 512), (16, 1024), (64, 8), (16, 16), (1, 256), (1, 1024))
# --sweep: the sizes between the task factors and 256 rows, where the two routes cross, at three batch sizes
SWEEP = tuple((B, N) for N in (32, 64, 128) for B in (1, 16, 256))


def timed_us(fn, reps, samples):
    for _ in range(2):
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


def rbf_gram(B, N, seed):
    """The workload's matrices: an RBF Gram matrix on 2-D points plus a small diagonal (clustered tiny eigenvalues)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(B, N, 2, generator=g, device="cuda", dtype=torch.float64)
    d2 = (x.unsqueeze(-2) - x.unsqueeze(-3)).pow(2).sum(-1)
    return torch.exp(-0.5 * d2 / 0.3 ** 2) + 1e-3 * torch.eye(N, device="cuda", dtype=torch.float64)


def kernel_shapes(args):
    from linear_operator_amd.functions import _eigh as FE

    for B, N in (SWEEP if args.sweep else SHAPES):
        A = rbf_gram(B, N, N + B)
        for what, fn in (("eigh", FE.eigh), ("eigvalsh", FE.eigvalsh)):
            with mock.patch.object(FE, "native_ok", lambda a: False):
                aten = timed_us(lambda: fn(A), args.reps, args.samples)
            with mock.patch.object(FE, "EIGH_NATIVE_MAX_N", 1024), mock.patch.object(FE, "EIGH_NATIVE_MIN_BATCH", 1):
                native = timed_us(lambda: fn(A), args.reps, args.samples)
            print(json.dumps({"shape": f"{B}x{N}^2", "what": what, "native_us": round(native, 1),
                              "aten_us": round(aten, 1), "speedup": round(aten / native, 2)}), flush=True)


def whole_calls(args):
    from linear_operator_amd.operators import (ConstantDiagLinearOperator, DenseLinearOperator,
                                               KroneckerProductLinearOperator, SumKroneckerLinearOperator)

    def dense(B, n, seed):
        return DenseLinearOperator(rbf_gram(B, n, seed).float())

    for B, n1, n2 in ((64, 512, 8), (16, 1024, 16)):
        rhs = torch.randn(B, n1 * n2, 1, device="cuda")

        def run(B=B, n1=n1, n2=n2, rhs=rhs):
            op = SumKroneckerLinearOperator(KroneckerProductLinearOperator(dense(B, n1, 1), dense(B, n2, 2)),
                                            KroneckerProductLinearOperator(dense(B, n1, 3), dense(B, n2, 4)))
            return op.solve(rhs)

        us = timed_us(run, max(1, args.reps // 5), args.samples)
        print(json.dumps({"call": "SumKronecker.solve", "shape": f"{B}x({n1}x{n2})", "us": round(us, 1)}), flush=True)
    B, n = 128, 256
    rhs = torch.randn(B, n * n, 1, device="cuda")

    def run_kd():
        op = KroneckerProductLinearOperator(dense(B, n, 5), dense(B, n, 6))
        return (op + ConstantDiagLinearOperator(torch.full((B, 1), 0.1, device="cuda"), diag_shape=n * n)).solve(rhs)

    us = timed_us(run_kd, max(1, args.reps // 5), args.samples)
    print(json.dumps({"call": "KroneckerProduct+ConstantDiag.solve", "shape": f"{B}x({n}x{n})", "us": round(us, 1)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--sweep", action="store_true", help="the crossover sizes (N = 32 .. 128) instead of the main shapes")
    ap.add_argument("--calls", action="store_true", help="whole-call timings of the consumers instead of the kernel")
    args = ap.parse_args()
    if args.calls:
        whole_calls(args)
    else:
        kernel_shapes(args)


if __name__ == "__main__":
    main()
