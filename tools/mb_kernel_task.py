#!/usr/bin/env python3
"""The matrix-free task-indexed multitask operator (csrc/lo_kernel_task.hip, LO_OP_KERNEL_TASK_DIAG): its three entry
points against what they replace, on the same inputs, the two taking turns over several rounds (median round, spread next
to it; device events after warm-up).

  product   lo_kernel_task_mv_f32 (1 and 17 columns)  against  ONE matmul with the stored dense matrix (forming the matrix
            is not timed: the comparison favours the stored route)
  bilinear  lo_kernel_task_bilinear_f32               against  autograd through the dense function for theta and task_covar
  points    lo_kernel_task_points_grad_f32            against  autograd through the dense function for x1
  big       the product alone at a shape whose stored K (1 TiB) no device holds
  solve     one preconditioned solve of TaskKernel + D at 1 x 8192 (D 4, T 4): the native descriptor against the dense
            callback route (the gate patched shut, the operator as it was before the kind existed: covar_func evaluated
            densely from Python once per product, the pivoted Cholesky through the generic row fetch); a fresh operator
            per solve, host clock around a synchronise

Shapes 1 x 16384 (D 4, T 4) and 8 x 4096 (D 16, T 8).  No routing rests on these numbers: inside its gate the kernel is
always taken, its purpose is memory.
Usage:  python tools/mb_kernel_task.py [--what product,bilinear,points,big,solve] [--reps 20] [--rounds 5]
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

SHAPES = ((1, 16384, 4, 4), (8, 4096, 16, 8))  # (B, n, D, T)
BIG = (1, 524288, 4, 4)  # K would be 1 TiB
COLS = (1, 17)
DERIV_COLS = 8
SOLVE = (1, 8192, 4, 4)
NB = {"outputscale": 0}
FN = covariance.rbf_task


def r1(t):
    return [round(x, 1) for x in t]


def make(B, n, D, T, gen, dev):
    ids = torch.randint(0, T, (B, n, 1), generator=gen).float()
    x = torch.cat((torch.rand(B, n, D, generator=gen), ids), -1).to(dev)
    ls = (0.3 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
    os_ = (0.8 + 0.6 * torch.rand(B, generator=gen)).to(dev)
    off = (0.5 + 0.4 * torch.rand(B, T, T, generator=gen)) / max(T - 1, 1)
    Bt = (0.5 * (off + off.mT) * (1 - torch.eye(T)) + torch.diag(1.0 + 0.35 * torch.arange(T))).to(dev)
    return x, ls, os_, Bt


def rel_diff(a, b):
    return ((a - b).norm() / b.norm()).item()


def product(args, dev, gen):
    for B, n, D, T in SHAPES:
        x, ls, os_, Bt = make(B, n, D, T, gen, dev)
        theta = K.kernel_theta(ls, os_, (B,), D)
        stored = FN(x, x, ls, os_, Bt)
        for c in COLS:
            V = torch.randn(B, n, c, generator=gen).to(dev)
            native = lambda: K.kernel_task_mv(x, x, theta, Bt, FN.native_family, V)  # noqa: E731
            dense = lambda: stored @ V  # noqa: E731
            times = alternated([native, dense], args.reps, args.rounds)
            print(json.dumps(dict(
                what="product", B=B, n=n, D=D, T=T, c=c, native_us=r1(times[0]), stored_matmul_us=r1(times[1]),
                native_over_stored=round(times[0][0] / times[1][0], 3),
                native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=rel_diff(native(), dense()))), flush=True)
        del stored


def derivatives(args, dev, gen, what):
    for B, n, D, T in SHAPES:
        x, ls, os_, Bt = make(B, n, D, T, gen, dev)
        theta = K.kernel_theta(ls, os_, (B,), D)
        U = torch.randn(B, n, DERIV_COLS, generator=gen).to(dev)
        V = torch.randn(B, n, DERIV_COLS, generator=gen).to(dev)

        def autograd(leaves):
            t = {"x": x, "ls": ls, "os": os_, "Bt": Bt}
            for k in leaves:
                t[k] = t[k].detach().clone().requires_grad_(True)
            (U * (FN(t["x"], x, t["ls"], t["os"], t["Bt"]) @ V)).sum().backward()
            return [t[k].grad for k in leaves]

        if what == "bilinear":
            native = lambda: K.kernel_task_bilinear(x, x, theta, Bt, FN.native_family, U, V)  # noqa: E731
            dense = lambda: autograd(("ls", "os", "Bt"))  # noqa: E731
            diff = rel_diff(native()[1], dense()[2])
        else:
            native = lambda: K.kernel_task_points_grad(x, x, theta, Bt, FN.native_family, U, V)  # noqa: E731
            dense = lambda: autograd(("x",))  # noqa: E731
            diff = rel_diff(native(), dense()[0])
        times = alternated([native, dense], max(args.reps // 4, 2), args.rounds)
        print(json.dumps(dict(
            what=what, B=B, n=n, D=D, T=T, t=DERIV_COLS, native_us=r1(times[0]), dense_autograd_us=r1(times[1]),
            native_over_autograd=round(times[0][0] / times[1][0], 4),
            native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=diff)), flush=True)


def big(args, dev, gen):
    B, n, D, T = BIG
    x, ls, os_, Bt = make(B, n, D, T, gen, dev)
    theta = K.kernel_theta(ls, os_, (B,), D)
    V = torch.randn(B, n, 1, generator=gen).to(dev)
    native = lambda: K.kernel_task_mv(x, x, theta, Bt, FN.native_family, V)  # noqa: E731
    torch.cuda.reset_peak_memory_stats()
    times = alternated([native], 2, 3)
    print(json.dumps(dict(what="big", B=B, n=n, D=D, T=T, c=1, native_us=r1(times[0]),
                          native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1),
                          stored_gib=round(B * n * n * 4 / 2 ** 30, 1),
                          peak_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))), flush=True)


def solve(args, dev, gen):
    B, n, D, T = SOLVE
    x, ls, os_, Bt = make(B, n, D, T, gen, dev)
    noise = (0.05 + 0.1 * torch.rand(B, n, generator=gen)).to(dev)
    rhs = torch.randn(B, n, 1, generator=gen).to(dev)

    def run():
        kern = KernelLinearOperator(x, x, FN, num_nonbatch_dimensions=NB, lengthscale=ls, outputscale=os_, task_covar=Bt)
        out = AddedDiagLinearOperator(kern, DiagLinearOperator(noise)).solve(rhs)
        torch.cuda.synchronize()
        return out

    def callback():  # (the gate shut: the operator as it was before the kind existed)
        with mock.patch.object(KernelLinearOperator, "_native_task_refusal", return_value="switched off"):
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
                          native_over_callback=round(med[0] / med[1], 4), rel_diff=rel_diff(a, b))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="product,bilinear,points,big,solve")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_task.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    for what in args.what.split(","):
        if what == "solve":
            solve(args, "cuda", gen)
        elif what == "big":
            big(args, "cuda", gen)
        elif what == "product":
            product(args, "cuda", gen)
        else:
            derivatives(args, "cuda", gen, what)


if __name__ == "__main__":
    main()
