#!/usr/bin/env python3
"""The matrix-free LMC operator sum_q Kron(Kernel_q(X, X), Dense(B_q)) (csrc/lo_kernel_lmc.hip, LO_OP_KERNEL_LMC_DIAG): the
fused product against the per-term composition it may replace in `_matmul`, on the same inputs, the two taking turns over
several rounds (median round, spread next to it; device events after warm-up), and the solvers on the kind against the
closure route.

  product   lo_kernel_lmc_mv_f32  against  Q calls of lo_kernel_kron_mv_f32 and the Q - 1 adds
  solve     one preconditioned solve of sum_q Kron(Kernel_q, B_q) + D at 1 x 8192 (D 4, T 4, Q 2), and one
            inv_quad_logdet + backward of the same operator: the native descriptor against the closure route (the
            descriptor forced to None: a Python call per product, the pivoted Cholesky through the generic row fetch); a
            fresh operator per call, host clock around a synchronise

Q in {2, 4}, T in {2, 4}, c in {1, 17}, shapes 1 x 16384 (D 4) and 8 x 4096 (D 16).  The routing table
kernels._NATIVE_MATMUL_KERNEL_LMC rests on this one: a cell in which the fused call is not faster,
beyond the spread and at both shapes, keeps the composition.
Usage:  python tools/mb_kernel_lmc.py [--what product,solve] [--reps 20] [--rounds 5]
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

from mb_kernel_kron import r1, rel_diff  # noqa: E402
from mb_ski_grid import alternated  # noqa: E402

from linear_operator_amd import covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, KernelLinearOperator,
    KroneckerProductLinearOperator, SumLinearOperator)

SHAPES = ((1, 16384, 4), (8, 4096, 16))  # (B, n, D)
TERMS = (2, 4)
TASKS = (2, 4)
COLS = (1, 17)
SOLVE = (1, 8192, 4, 4, 2)  # (B, n, D, T, Q)
NB = {"outputscale": 0}
FAMILIES = ("rbf", "matern52", "matern32", "matern12")  # term q's family


def make(B, n, D, T, Q, gen, dev):
    x = torch.rand(B, n, D, generator=gen).to(dev)
    ls = [(0.3 * D ** 0.5 * (0.6 + 0.5 * q) * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev) for q in range(Q)]
    os_ = [(0.6 + 0.5 * torch.rand(B, generator=gen)).to(dev) for _ in range(Q)]
    off = (0.5 + 0.4 * torch.rand(B, Q, T, T, generator=gen)) / max(T - 1, 1)
    Bt = (0.5 * (off + off.mT) * (1 - torch.eye(T)) + torch.diag(1.0 + 0.35 * torch.arange(T))).to(dev)
    return x, ls, os_, Bt.contiguous()


def product(args, dev, gen):
    for B, n, D in SHAPES:
        for Q in TERMS:
            for T in TASKS:
                x, ls, os_, Bt = make(B, n, D, T, Q, gen, dev)
                theta = K.kernel_sum_theta(ls, os_, (B,), D)
                fams = [covariance.FAMILIES[f].native_family for f in FAMILIES[:Q]]
                th = [theta[:, q].contiguous() for q in range(Q)]
                bq = [Bt[:, q].contiguous() for q in range(Q)]
                for c in COLS:
                    V = torch.randn(B, n * T, c, generator=gen).to(dev)
                    fused = lambda: K.kernel_lmc_mv(x, theta, Bt, fams, V)  # noqa: E731

                    def composed():
                        y = K.kernel_kron_mv(x, th[0], bq[0], fams[0], V)
                        for q in range(1, Q):
                            y += K.kernel_kron_mv(x, th[q], bq[q], fams[q], V)
                        return y

                    times = alternated([fused, composed], args.reps, args.rounds)
                    print(json.dumps(dict(
                        what="product", B=B, n=n, D=D, Q=Q, T=T, c=c, fused_us=r1(times[0]), composed_us=r1(times[1]),
                        fused_over_composed=round(times[0][0] / times[1][0], 3),
                        fused_gpairs_s=round(B * n * n * Q / times[0][0] / 1e3, 1), rel_diff=rel_diff(fused(), composed()))),
                        flush=True)


def solve(args, dev, gen):
    B, n, D, T, Q = SOLVE
    x, ls, os_, Bt = make(B, n, D, T, Q, gen, dev)
    noise = (0.05 + 0.1 * torch.rand(B, n * T, generator=gen)).to(dev)
    rhs = torch.randn(B, n * T, 1, generator=gen).to(dev)

    def operator(grad):
        leaves = [x.clone().requires_grad_(grad)]
        terms = []
        for q in range(Q):
            l, o, b = (t.clone().requires_grad_(grad) for t in (ls[q], os_[q], Bt[:, q]))
            leaves += [l, o, b]
            kern = KernelLinearOperator(leaves[0], leaves[0], covariance.FAMILIES[FAMILIES[q]], num_nonbatch_dimensions=NB,
                                        lengthscale=l, outputscale=o)
            terms.append(KroneckerProductLinearOperator(kern, DenseLinearOperator(b)))
        return AddedDiagLinearOperator(SumLinearOperator(*terms), DiagLinearOperator(noise)), leaves

    def run_solve():
        out = operator(False)[0].solve(rhs)
        torch.cuda.synchronize()
        return out

    def run_iqld():
        A, leaves = operator(True)
        iq, ld = A.inv_quad_logdet(rhs, logdet=True)
        (iq.sum() + ld.sum()).backward()
        torch.cuda.synchronize()
        return leaves[1].grad

    def closure(fn):  # (the descriptor forced to None: the operator as it was before the kind existed)
        def call():
            with mock.patch.object(SumLinearOperator, "_kernel_descriptor", return_value=None):
                return fn()
        return call

    def clock(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e6

    with settings.max_cholesky_size(0), settings.min_preconditioning_size(0), settings.cg_tolerance(1e-3):
        for what, fn in (("solve", run_solve), ("inv_quad_logdet_backward", run_iqld)):
            pair = (fn, closure(fn))
            torch.manual_seed(0)
            a = pair[0]()  # (warm-up)
            torch.manual_seed(0)
            b = pair[1]()
            times = [[], []]
            for _ in range(args.rounds):
                for k, f in enumerate(pair):
                    times[k].append(clock(f))
            med = [statistics.median(t) for t in times]
            print(json.dumps(dict(what=what, B=B, n=n, D=D, T=T, Q=Q,
                                  native_us=r1((med[0], min(times[0]), max(times[0]))),
                                  closure_us=r1((med[1], min(times[1]), max(times[1]))),
                                  native_over_closure=round(med[0] / med[1], 3), rel_diff=rel_diff(a, b))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="product,solve")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_lmc.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    for what in args.what.split(","):
        if what == "solve":
            solve(args, "cuda", gen)
        else:
            product(args, "cuda", gen)


if __name__ == "__main__":
    main()
