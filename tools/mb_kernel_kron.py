#!/usr/bin/env python3
"""The matrix-free multitask operator Kron(Kernel(X, X), Dense(Bt)) (csrc/lo_kernel_kron.hip, LO_OP_KERNEL_KRON_DIAG): the
fused product against the per-factor composition it may replace in `_matmul`, on the same inputs, the two taking turns
over several rounds (median round, spread next to it; device events after warm-up).

  product   lo_kernel_kron_mv_f32  against  `_kron_matmul`: lo_kernel_mv_f32 with T c columns, the transposing reshape,
            Bt by ATen, the reshape back
  solve     one preconditioned solve of Kron(Kernel, Bt) + D at 1 x 8192 (D 4, T 4): the native descriptor against the
            callback route (the gate patched shut: a Python call per product, the pivoted Cholesky through the generic
            row fetch); a fresh operator per solve, host clock around a synchronise

T in {2, 4, 8}, c in {1, 17}, shapes 1 x 16384 (D 4) and 8 x 4096 (D 16).  The routing table of
operators/kronecker_product_linear_operator.py rests on this one: a cell in which the fused call is
not at least as fast, beyond the spread and at both shapes, keeps the composition.
Usage:  python tools/mb_kernel_kron.py [--what product,solve] [--reps 20] [--rounds 5]
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mb_ski_grid import alternated  # noqa: E402

from linear_operator_amd import covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator, KroneckerProductLinearOperator)
from linear_operator_amd.operators.kronecker_product_linear_operator import _kron_matmul  # noqa: E402

SHAPES = ((1, 16384, 4), (8, 4096, 16))  # (B, n, D)
TASKS = (2, 4, 8)
COLS = (1, 17)
SOLVE = (1, 8192, 4, 4)  # (B, n, D, T)
NB = {"outputscale": 0}


def r1(t):
    return [round(x, 1) for x in t]


def make(B, n, D, T, gen, dev):
    x = torch.rand(B, n, D, generator=gen).to(dev)
    ls = (0.3 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
    os_ = (0.8 + 0.6 * torch.rand(B, generator=gen)).to(dev)
    off = (0.5 + 0.4 * torch.rand(B, T, T, generator=gen)) / max(T - 1, 1)
    Bt = (0.5 * (off + off.mT) * (1 - torch.eye(T)) + torch.diag(1.0 + 0.35 * torch.arange(T))).to(dev)
    return x, ls, os_, Bt


def rel_diff(a, b):
    return ((a - b).norm() / b.norm()).item()


def product(args, dev, gen):
    for B, n, D in SHAPES:
        for T in TASKS:
            x, ls, os_, Bt = make(B, n, D, T, gen, dev)
            theta = K.kernel_theta(ls, os_, (B,), D)
            kern = KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_)
            ops = (kern, DenseLinearOperator(Bt))
            shape = torch.Size((B, n * T, n * T))
            for c in COLS:
                V = torch.randn(B, n * T, c, generator=gen).to(dev)
                fused = lambda: K.kernel_kron_mv(x, theta, Bt, covariance.rbf.native_family, V)  # noqa: E731
                composed = lambda: _kron_matmul(ops, shape, V)  # noqa: E731
                times = alternated([fused, composed], args.reps, args.rounds)
                print(json.dumps(dict(
                    what="product", B=B, n=n, D=D, T=T, c=c, fused_us=r1(times[0]), composed_us=r1(times[1]),
                    fused_over_composed=round(times[0][0] / times[1][0], 3),
                    fused_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=rel_diff(fused(), composed()))),
                    flush=True)


def solve(args, dev, gen):
    B, n, D, T = SOLVE
    x, ls, os_, Bt = make(B, n, D, T, gen, dev)
    noise = (0.05 + 0.1 * torch.rand(B, n * T, generator=gen)).to(dev)
    rhs = torch.randn(B, n * T, 1, generator=gen).to(dev)

    def run():
        kern = KernelLinearOperator(x, x, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_)
        kron = KroneckerProductLinearOperator(kern, DenseLinearOperator(Bt))
        out = AddedDiagLinearOperator(kron, DiagLinearOperator(noise)).solve(rhs)
        torch.cuda.synchronize()
        return out

    def callback():  # (the gate shut: the operator as it was before the kind existed)
        with mock.patch.object(KroneckerProductLinearOperator, "_kernel_kron_refusal", return_value="switched off"):
            return run()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    with settings.max_cholesky_size(0), settings.min_preconditioning_size(0), settings.cg_tolerance(1e-3):
        a, b = run(), callback()  # (warm-up)
        times = [[], []]
        for _ in range(args.rounds):
            for k, fn in enumerate((run, callback)):
                times[k].append(clock(fn))
    med = [statistics.median(t) for t in times]
    print(json.dumps(dict(what="solve", B=B, n=n, D=D, T=T,
                          native_us=r1((med[0], min(times[0]), max(times[0]))),
                          callback_us=r1((med[1], min(times[1]), max(times[1]))),
                          native_over_callback=round(med[0] / med[1], 3), rel_diff=rel_diff(a, b))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="product,solve")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_kron.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    for what in args.what.split(","):
        if what == "solve":
            solve(args, "cuda", gen)
        else:
            product(args, "cuda", gen)


if __name__ == "__main__":
    main()
