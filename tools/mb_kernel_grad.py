#!/usr/bin/env python3
"""The matrix-free RBF gradient kernel (csrc/lo_kernel_grad.hip, LO_OP_KERNEL_GRAD_DIAG): a GP with derivative
observations, D + 1 outputs per input.  The native routes against what they replace, on the same inputs, the two taking
turns over several rounds (median round, spread next to it; device events after warm-up).

  product   lo_kernel_grad_mv_f32 against one matmul with the STORED dense block matrix (built once, outside the clock)
            where one fits: 1 x 4096 (D 3; stored 1 GiB) and 8 x 1024 (D 8; stored 2.5 GiB), 1 and 17 columns
  large     lo_kernel_grad_mv_f32 alone at 1 x 16384 (D 3), where the stored matrix would be 16 GiB
  solve     one preconditioned solve of GradKernel + D at 1 x 4096 (D 3): the native descriptor against the route of the
            parent commit (the gate patched shut: a Python call per product that evaluates covar_func densely, the pivoted
            Cholesky through the generic row fetch); a fresh operator per solve, host clock around a synchronise
  bilinear  lo_kernel_grad_bilinear_f32 against float32 autograd through the dense block matrix (formed inside the clock:
            that is the general path of `_bilinear_derivative`) at 1 x 4096 (D 3) and 8 x 1024 (D 8), 11 columns

`_matmul` always takes the native product inside its gate (its purpose is memory), so no routing table rests on this tool;
DESIGN.md section 6o records what it measured.
Usage:  python tools/mb_kernel_grad.py [--what product,large,solve,bilinear] [--reps 20] [--rounds 5]
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
from linear_operator_amd.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator  # noqa: E402

SHAPES = ((1, 4096, 3), (8, 1024, 8))  # (B, n, D)
LARGE = (1, 16384, 3)
COLS = (1, 17)
SOLVE = (1, 4096, 3)
BIL_COLS = 11
NB = {"outputscale": 0}
RBF = covariance.rbf_grad.native_family


def r1(t):
    return [round(x, 1) for x in t]


def make(B, n, D, gen, dev):
    x = torch.rand(B, n, D, generator=gen).to(dev)
    ls = (0.35 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
    os_ = (0.8 + 0.6 * torch.rand(B, generator=gen)).to(dev)
    return x, ls, os_


def rel_diff(a, b):
    return ((a - b).norm() / b.norm()).item()


def product(args, dev, gen):
    for B, n, D in SHAPES:
        x, ls, os_ = make(B, n, D, gen, dev)
        theta = K.kernel_theta(ls, os_, (B,), D)
        stored = covariance.rbf_grad(x, x, ls, os_)
        for c in COLS:
            V = torch.randn(B, n * (D + 1), c, generator=gen).to(dev)
            native = lambda: K.kernel_grad_mv(x, x, theta, RBF, V)  # noqa: E731
            dense = lambda: stored @ V  # noqa: E731
            times = alternated([native, dense], args.reps, args.rounds)
            print(json.dumps(dict(
                what="product", B=B, n=n, D=D, c=c, native_us=r1(times[0]), stored_us=r1(times[1]),
                native_over_stored=round(times[0][0] / times[1][0], 3), stored_gib=round(stored.numel() * 4 / 2 ** 30, 2),
                native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=rel_diff(native(), dense()))), flush=True)
        del stored


def large(args, dev, gen):
    B, n, D = LARGE
    x, ls, os_ = make(B, n, D, gen, dev)
    theta = K.kernel_theta(ls, os_, (B,), D)
    for c in COLS:
        V = torch.randn(B, n * (D + 1), c, generator=gen).to(dev)
        times = alternated([lambda: K.kernel_grad_mv(x, x, theta, RBF, V)], args.reps, args.rounds)
        print(json.dumps(dict(what="large", B=B, n=n, D=D, c=c, native_us=r1(times[0]),
                              stored_gib=round((B * (n * (D + 1)) ** 2) * 4 / 2 ** 30, 2),
                              native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1))), flush=True)


def solve(args, dev, gen):
    B, n, D = SOLVE
    x, ls, os_ = make(B, n, D, gen, dev)
    N = n * (D + 1)
    noise = (0.05 + 0.1 * torch.rand(B, N, generator=gen)).to(dev)
    rhs = torch.randn(B, N, 1, generator=gen).to(dev)

    def run():
        op = KernelLinearOperator(x, x, covariance.rbf_grad, num_outputs_per_input=(D + 1, D + 1),
                                  num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_)
        out = AddedDiagLinearOperator(op, DiagLinearOperator(noise)).solve(rhs)
        torch.cuda.synchronize()
        return out

    def parent():  # (the gate shut: the operator as it was before the kind existed)
        with mock.patch.object(KernelLinearOperator, "_native_grad_refusal", return_value="switched off"):
            return run()

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    with settings.max_cholesky_size(0), settings.min_preconditioning_size(0), settings.cg_tolerance(1e-3):
        a, b = run(), parent()  # (warm-up)
        times = [[], []]
        for _ in range(args.rounds):
            for k, fn in enumerate((run, parent)):
                times[k].append(clock(fn))
    med = [statistics.median(t) for t in times]
    print(json.dumps(dict(what="solve", B=B, n=n, D=D, native_us=r1((med[0], min(times[0]), max(times[0]))),
                          parent_us=r1((med[1], min(times[1]), max(times[1]))),
                          native_over_parent=round(med[0] / med[1], 3), rel_diff=rel_diff(a, b))), flush=True)


def bilinear(args, dev, gen):
    for B, n, D in SHAPES:
        x, ls, os_ = make(B, n, D, gen, dev)
        theta = K.kernel_theta(ls, os_, (B,), D)
        U = torch.randn(B, n * (D + 1), BIL_COLS, generator=gen).to(dev)
        V = torch.randn(B, n * (D + 1), BIL_COLS, generator=gen).to(dev)

        def autograd():
            l, o = ls.clone().requires_grad_(True), os_.clone().requires_grad_(True)
            (U * (covariance.rbf_grad(x, x, l, o) @ V)).sum().backward()
            return l.grad

        native = lambda: K.kernel_grad_bilinear(x, x, theta, RBF, U, V)  # noqa: E731
        times = alternated([native, autograd], max(args.reps // 4, 2), args.rounds)
        g = native()
        d_ls = (-(theta[:, :D] ** 2) * g[:, :D]).reshape(B, 1, D)
        print(json.dumps(dict(what="bilinear", B=B, n=n, D=D, t=BIL_COLS, native_us=r1(times[0]), autograd_us=r1(times[1]),
                              native_over_autograd=round(times[0][0] / times[1][0], 4),
                              rel_diff=rel_diff(d_ls, autograd()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="product,large,solve,bilinear")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_grad.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    todo = dict(product=product, large=large, solve=solve, bilinear=bilinear)
    for what in args.what.split(","):
        todo[what](args, "cuda", gen)


if __name__ == "__main__":
    main()
