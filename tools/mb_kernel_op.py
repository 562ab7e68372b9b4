#!/usr/bin/env python3
"""Matrix-free kernel operator microbenchmark (csrc/lo_kernel_op.hip, LO_OP_KERNEL_DIAG): the on-the-fly product
lo_kernel_mv_f32 against the stored dense product of the SAME matrix (K evaluated once by the covariance function, then
lo_matvec_f32 on LO_OP_DENSE_DIAG, which streams 4 N^2 bytes per member), per family.  The largest shape has no dense
alternative (a stored K would be 64 GiB) and is timed alone.  Device events after warm-up, the alternatives taking turns
over several rounds (median round, spread next to it).

No routing decision depends on these numbers: the native path is taken whenever its gate holds, because its purpose is
memory; the table says what that costs or saves in time.

Points' gradient (--what points): lo_kernel_points_grad_f32 for BOTH sides (two calls) against what the operator did up to
ABI 26, restated here as chunked_autograd_points: torch autograd through the covariance function on row blocks of at
most 64 MiB of differences.  Same inputs, the two taking turns; the slow alternative is repeated fewer times per turn
(its count is printed), never fewer turns.
Usage:  python tools/mb_kernel_op.py [--what product,points] [--reps 20] [--rounds 5] [--families rbf,matern52]
One JSON line per measurement.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mb_ski_grid import alternated, timed  # noqa: E402

from linear_operator_amd import covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402

# (B, N, D, c, time the stored dense product too)
SHAPES = ((1, 16384, 4, 1, True), (1, 16384, 4, 17, True), (8, 8192, 16, 1, True), (1, 131072, 8, 1, False))
# (B, N, D, t) of the points' gradient
POINT_SHAPES = ((1, 16384, 4, 1), (1, 16384, 4, 17), (8, 8192, 16, 1), (1, 131072, 8, 1))
CHUNK_BYTES = 64 * 1024 * 1024  # the differences [rows, N, D] of one row block of the autograd path


def r1(t):
    return [round(x, 1) for x in t]


def chunked_autograd_points(fn, x1, x2, ls, os_, U, V):
    """d / d x1 and d / d x2 of sum_s u_s^T K v_s as KernelLinearOperator computed them up to ABI 26: autograd through
    the covariance function on blocks of rows, x1 and x2 separate leaves."""
    B, M, D = x1.shape
    N = x2.shape[1]
    rows = max(1, min(M, CHUNK_BYTES // (B * N * D * x1.element_size())))
    g1, g2 = torch.zeros_like(x1), torch.zeros_like(x2)
    for lo in range(0, M, rows):
        hi = min(M, lo + rows)
        with torch.enable_grad():
            a = x1[:, lo:hi].clone().requires_grad_(True)
            b = x2.clone().requires_grad_(True)
            loss = (U[:, lo:hi] * (fn(a, b, ls, os_) @ V)).sum()
            ga, gb = torch.autograd.grad(loss, [a, b])
        g1[:, lo:hi] = ga
        g2 += gb
    return g1, g2


def alternated_within(fns, reps, rounds, turn_us=1e6):
    """alternated() for alternatives of very different cost: every function is warmed up, its call time estimated, and
    its repetitions per turn cut (down to 1) so that a turn stays near `turn_us`.  Returns the times and the counts."""
    per = []
    for fn in fns:
        fn()
        est = timed(fn, 1)
        per.append(max(1, min(reps, int(turn_us / est))))
        for _ in range(min(4, per[-1] - 1)):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(timed(fn, per[k]))
    return [(statistics.median(t), min(t), max(t)) for t in times], per


def points_gradient(args, dev, gen):
    for B, N, D, t in POINT_SHAPES:
        x = torch.rand(B, N, D, generator=gen).to(dev)
        ls = (0.3 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
        os_ = (0.8 + 0.7 * torch.rand(B, generator=gen)).to(dev)
        U, V = torch.randn(B, N, t, generator=gen).to(dev), torch.randn(B, N, t, generator=gen).to(dev)
        theta = K.kernel_theta(ls, os_, (B,), D)
        for name in args.families.split(","):
            fn = covariance.FAMILIES[name]
            fam = fn.native_family
            fns = [lambda: (K.kernel_points_grad(x, x, theta, fam, U, V), K.kernel_points_grad(x, x, theta, fam, V, U)),
                   lambda: chunked_autograd_points(fn, x, x, ls, os_, U, V)]
            times, per = alternated_within(fns, args.reps, args.rounds)
            (n1, n2), (c1, c2) = fns[0](), fns[1]()
            pairs = 2 * B * N * N
            print(json.dumps(dict(
                what="kernel_points_grad", family=name, B=B, N=N, D=D, t=t, native_us=r1(times[0]),
                chunked_autograd_us=r1(times[1]), calls_per_turn=per, native_gpairs_s=round(pairs / times[0][0] / 1e3, 1),
                native_over_chunked=round(times[0][0] / times[1][0], 4),
                rel_diff_x1=((n1 - c1).norm() / c1.norm()).item(), rel_diff_x2=((n2 - c2).norm() / c2.norm()).item())),
                flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--families", default="rbf,matern12,matern32,matern52")
    ap.add_argument("--what", default="product,points")
    args = ap.parse_args()
    dev = "cuda"
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_op.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    if "product" in args.what.split(","):
        product(args, dev, gen)
    if "points" in args.what.split(","):
        points_gradient(args, dev, gen)


def product(args, dev, gen):
    for B, N, D, c, with_dense in SHAPES:
        x = torch.rand(B, N, D, generator=gen).to(dev)
        ls = (0.3 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
        os_ = (0.8 + 0.7 * torch.rand(B, generator=gen)).to(dev)
        v = torch.randn(B, N, c, generator=gen).to(dev)
        theta = K.kernel_theta(ls, os_, (B,), D)
        for name in args.families.split(","):
            fn = covariance.FAMILIES[name]
            fns = [lambda: K.kernel_mv(x, x, theta, fn.native_family, v)]
            dense_desc = None
            if with_dense:
                dense = torch.cat([fn(x[b:b + 1], x[b:b + 1], ls[b:b + 1], os_[b:b + 1]) for b in range(B)])
                dense_desc = K.dense_diag_descriptor(dense, None)
                fns.append(lambda: K.matvec(dense_desc, v))
            reps = args.reps if N <= 16384 else max(2, args.reps // 10)
            times = alternated(fns, reps, args.rounds)
            pairs = B * N * N
            out = dict(what="kernel_mv", family=name, B=B, N=N, D=D, c=c, native_us=r1(times[0]),
                       native_gpairs_s=round(pairs / times[0][0] / 1e3, 1),
                       stored_k_gib=round(4 * pairs / 2 ** 30, 2))
            if with_dense:
                y_n, y_d = fns[0](), fns[1]()
                out.update(dense_us=r1(times[1]), dense_gb_s=round(4 * pairs / times[1][0] / 1e3, 1),
                           native_over_dense=round(times[0][0] / times[1][0], 2),
                           rel_diff=((y_n - y_d).norm() / y_d.norm()).item())
                del dense, dense_desc
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
