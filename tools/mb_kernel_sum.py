#!/usr/bin/env python3
"""Sums of matrix-free kernel operators (csrc/lo_kernel_sum.hip, LO_OP_KERNEL_SUM_DIAG): the fused multi-term calls against
the per-term route they replace -- T calls of the single-term entry point of csrc/lo_kernel_op.hip plus the adds -- on the
same inputs, the two taking turns over several rounds (median round, spread next to it; device events after warm-up).

  product   lo_kernel_sum_mv_f32           against  T x lo_kernel_mv_f32 + (T - 1) adds
  bilinear  lo_kernel_sum_bilinear_f32     against  T x lo_kernel_bilinear_f32
  points    lo_kernel_sum_points_grad_f32  against  T x lo_kernel_points_grad_f32 + (T - 1) adds   (the x1 side)
  solve     one preconditioned solve of K_1 + K_2 + D at the first shape: the native descriptor against the callback
            route (the descriptors of the sum patched to None: a Python call per product, the pivoted Cholesky through
            the generic row fetch); a fresh operator per solve, host clock around a synchronise

T in {2, 3}, c (or t) in {1, 17}, shapes 1 x 16384 (D 4) and 8 x 8192 (D 16).  The routing of SumLinearOperator rests on
this table: a cell in which the fused call is not at least as fast keeps the per-term calls.
Usage:  python tools/mb_kernel_sum.py [--what product,bilinear,points,solve] [--reps 20] [--rounds 5]
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
    AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator, SumLinearOperator)

SHAPES = ((1, 16384, 4), (8, 8192, 16))  # (B, N, D)
TERMS = {2: ("rbf", "matern52"), 3: ("matern12", "matern32", "rbf")}
COLS = (1, 17)


def r1(t):
    return [round(x, 1) for x in t]


def make(B, N, D, names, gen, dev):
    x = torch.rand(B, N, D, generator=gen).to(dev)
    ls = [(0.3 * D ** 0.5 * 0.5 * (t + 1) * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
          for t in range(len(names))]
    os_ = [(0.6 + 0.6 * torch.rand(B, generator=gen)).to(dev) for _ in names]
    fams = [covariance.FAMILIES[n].native_family for n in names]
    thetas = [K.kernel_theta(l, o, (B,), D) for l, o in zip(ls, os_)]
    return x, ls, os_, fams, thetas, K.kernel_sum_theta(ls, os_, (B,), D)


def rel_diff(a, b):
    return ((a - b).norm() / b.norm()).item()


def calls(args, dev, gen, what):
    for B, N, D in SHAPES:
        for T, names in TERMS.items():
            x, ls, os_, fams, thetas, theta = make(B, N, D, names, gen, dev)
            for c in COLS:
                U, V = torch.randn(B, N, c, generator=gen).to(dev), torch.randn(B, N, c, generator=gen).to(dev)
                if what == "product":
                    fused = lambda: K.kernel_sum_mv(x, x, theta, fams, V)  # noqa: E731
                    per_term = lambda: sum(K.kernel_mv(x, x, th, f, V) for th, f in zip(thetas, fams))  # noqa: E731
                elif what == "bilinear":
                    fused = lambda: K.kernel_sum_bilinear(x, x, theta, fams, U, V)  # noqa: E731
                    per_term = lambda: torch.stack(  # noqa: E731
                        [K.kernel_bilinear(x, x, th, f, U, V) for th, f in zip(thetas, fams)], 1)
                else:
                    fused = lambda: K.kernel_sum_points_grad(x, x, theta, fams, U, V)  # noqa: E731
                    per_term = lambda: sum(  # noqa: E731
                        K.kernel_points_grad(x, x, th, f, U, V) for th, f in zip(thetas, fams))
                times = alternated([fused, per_term], args.reps, args.rounds)
                pairs = B * N * N
                print(json.dumps(dict(
                    what=what, terms="+".join(names), B=B, N=N, D=D, c=c, fused_us=r1(times[0]),
                    per_term_us=r1(times[1]), fused_over_per_term=round(times[0][0] / times[1][0], 3),
                    fused_gpairs_s=round(pairs / times[0][0] / 1e3, 1), rel_diff=rel_diff(fused(), per_term()))),
                    flush=True)


def solve(args, dev, gen):
    B, N, D = SHAPES[0]
    names = TERMS[2]
    x, ls, os_, fams, thetas, theta = make(B, N, D, names, gen, dev)
    noise = (0.05 + 0.1 * torch.rand(B, N, generator=gen)).to(dev)
    rhs = torch.randn(B, N, 1, generator=gen).to(dev)

    def run():
        ops = [KernelLinearOperator(x, x, covariance.FAMILIES[n], num_nonbatch_dimensions={"outputscale": 0},
                                    lengthscale=l, outputscale=o) for n, l, o in zip(names, ls, os_)]
        out = AddedDiagLinearOperator(ops[0] + ops[1], DiagLinearOperator(noise)).solve(rhs)
        torch.cuda.synchronize()
        return out

    def callback():
        with mock.patch.object(AddedDiagLinearOperator, "_kernel_descriptor", return_value=None), \
                mock.patch.object(SumLinearOperator, "_kernel_descriptor", return_value=None):
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
    print(json.dumps(dict(what="solve", terms="+".join(names), B=B, N=N, D=D,
                          native_us=r1((med[0], min(times[0]), max(times[0]))),
                          callback_us=r1((med[1], min(times[1]), max(times[1]))),
                          native_over_callback=round(med[0] / med[1], 3), rel_diff=rel_diff(a, b))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="product,bilinear,points,solve")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_sum.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    for what in args.what.split(","):
        if what == "solve":
            solve(args, "cuda", gen)
        else:
            calls(args, "cuda", gen, what)


if __name__ == "__main__":
    main()
