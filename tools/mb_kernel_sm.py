#!/usr/bin/env python3
"""The matrix-free spectral mixture kernel (csrc/lo_kernel_sm.hip, LO_OP_KERNEL_SM_DIAG): the three entry points against
what they replace, on the same inputs, the two (or three) taking turns over several rounds (median round, spread next to
it; device events after warm-up).

  product   lo_kernel_sm_mv_f32 (1 and 17 columns)  against  ONE matmul with the stored dense matrix (forming the matrix is
            not timed: the comparison favours the stored route)  and against  the general path, the operator's `_matmul`
            with the gate patched shut: covar_func evaluated densely inside the product
  bilinear  lo_kernel_sm_bilinear_f32               against  autograd through the dense function for the parameters
  points    lo_kernel_sm_points_grad_f32            against  autograd through the dense function for x1
  solve     one preconditioned solve of SM + D at 1 x 8192 (D 1, Q 4): the native descriptor against the dense callback
            route (the gate patched shut); a fresh operator per solve, host clock around a synchronise

Shapes 1 x 16384 (D 1, Q 4: the time-series shape) and 8 x 8192 (D 4, Q 4).  The dense function holds [Q, M, N, D]
intermediates (4 GiB per tensor per member at both shapes), so every dense route runs member by member; a route that runs
out of memory is reported as null.  No routing rests on these numbers: inside its gate the kernel is always taken, its
purpose is memory.
Usage:  python tools/mb_kernel_sm.py [--what product,bilinear,points,solve] [--reps 20] [--rounds 5]
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

SHAPES = ((1, 16384, 1, 4), (8, 8192, 4, 4))  # (B, n, D, Q)
COLS = (1, 17)
DERIV_COLS = 8
SOLVE = (1, 8192, 1, 4)
NB = {"mixture_weights": 1}
NAMES = ("mixture_weights", "mixture_means", "mixture_scales")
FN = covariance.spectral_mixture


def r1(t):
    return [round(x, 1) for x in t]


def make(B, n, D, Q, gen, dev, span=30.0):
    """(x, the parameters by name, theta): points over about `span` periods of the fastest mixture, envelopes of a tenth
    of the domain and more."""
    x = (span * torch.rand(B, n, D, generator=gen)).to(dev)
    p = {"mixture_weights": (0.3 + 0.7 * torch.rand(B, Q, generator=gen)).to(dev),
         "mixture_means": (0.3 + 0.7 * torch.rand(B, Q, D, generator=gen)).to(dev),
         "mixture_scales": ((0.02 + 0.06 * torch.rand(B, Q, D, generator=gen)) / D ** 0.5).to(dev)}
    return x, p, K.kernel_sm_theta(*(p[k] for k in NAMES), (B,), D)


def member(p, b):
    return {k: v[b:b + 1] for k, v in p.items()}


def dense_fn(x1, x2, p):
    return FN(x1, x2, *(p[k] for k in NAMES))


def rel_diff(a, b):
    return ((a - b).norm() / b.norm()).item()


def product(args, dev, gen):
    for B, n, D, Q in SHAPES:
        x, p, theta = make(B, n, D, Q, gen, dev)
        stored = torch.cat([dense_fn(x[b:b + 1], x[b:b + 1], member(p, b)) for b in range(B)])
        members = [KernelLinearOperator(x[b:b + 1], x[b:b + 1], FN, num_nonbatch_dimensions=NB, **member(p, b))
                   for b in range(B)]
        for c in COLS:
            V = torch.randn(B, n, c, generator=gen).to(dev)
            native = lambda: K.kernel_sm_mv(x, x, theta, V)  # noqa: E731
            dense = lambda: stored @ V  # noqa: E731

            def general():
                with mock.patch.object(KernelLinearOperator, "_native_sm_refusal", return_value="switched off"):
                    return torch.cat([op._matmul(V[b:b + 1]) for b, op in enumerate(members)])

            try:
                times = alternated([native, dense, general], args.reps, args.rounds)
            except torch.cuda.OutOfMemoryError:
                torch.cuda.empty_cache()
                times = alternated([native, dense], args.reps, args.rounds) + [None]
            print(json.dumps(dict(
                what="product", B=B, n=n, D=D, Q=Q, c=c, native_us=r1(times[0]), stored_matmul_us=r1(times[1]),
                general_path_us=None if times[2] is None else r1(times[2]),
                native_over_stored=round(times[0][0] / times[1][0], 3),
                native_over_general=None if times[2] is None else round(times[0][0] / times[2][0], 4),
                native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=rel_diff(native(), dense()))), flush=True)
        del stored


def derivatives(args, dev, gen, what):
    for B, n, D, Q in SHAPES:
        x, p, theta = make(B, n, D, Q, gen, dev)
        U = torch.randn(B, n, DERIV_COLS, generator=gen).to(dev)
        V = torch.randn(B, n, DERIV_COLS, generator=gen).to(dev)

        def autograd(points):
            grads = []
            for b in range(B):
                xb, pb = x[b:b + 1], member(p, b)
                if points:
                    leaf = xb.detach().clone().requires_grad_(True)
                    (U[b:b + 1] * (dense_fn(leaf, xb, pb) @ V[b:b + 1])).sum().backward()
                    grads.append(leaf.grad)
                else:
                    pb = {k: v.detach().clone().requires_grad_(True) for k, v in pb.items()}
                    (U[b:b + 1] * (dense_fn(xb, xb, pb) @ V[b:b + 1])).sum().backward()
                    grads.append(torch.cat((pb[NAMES[0]].grad[..., None], pb[NAMES[1]].grad, pb[NAMES[2]].grad), -1))
            return torch.cat(grads)

        if what == "bilinear":
            native = lambda: K.kernel_sm_bilinear(x, x, theta, U, V)  # noqa: E731
            dense = lambda: autograd(False)  # noqa: E731
        else:
            native = lambda: K.kernel_sm_points_grad(x, x, theta, U, V)  # noqa: E731
            dense = lambda: autograd(True)  # noqa: E731
        try:
            diff = rel_diff(native(), dense())
            times = alternated([native, dense], max(args.reps // 4, 2), args.rounds)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            diff, times = None, alternated([native], max(args.reps // 4, 2), args.rounds) + [None]
        print(json.dumps(dict(
            what=what, B=B, n=n, D=D, Q=Q, t=DERIV_COLS, native_us=r1(times[0]),
            dense_autograd_us=None if times[1] is None else r1(times[1]),
            native_over_autograd=None if times[1] is None else round(times[0][0] / times[1][0], 4),
            native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=diff)), flush=True)


def solve(args, dev, gen):
    B, n, D, Q = SOLVE
    x, p, _ = make(B, n, D, Q, gen, dev)
    noise = (0.05 + 0.1 * torch.rand(B, n, generator=gen)).to(dev)
    rhs = torch.randn(B, n, 1, generator=gen).to(dev)

    def run():
        kern = KernelLinearOperator(x, x, FN, num_nonbatch_dimensions=NB, **p)
        out = AddedDiagLinearOperator(kern, DiagLinearOperator(noise)).solve(rhs)
        torch.cuda.synchronize()
        return out

    def callback():  # (the gate shut: the operator as it was before the kind existed)
        with mock.patch.object(KernelLinearOperator, "_native_sm_refusal", return_value="switched off"):
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
    print(json.dumps(dict(what="solve", B=B, n=n, D=D, Q=Q,
                          native_us=r1((med[0], min(times[0]), max(times[0]))),
                          callback_us=r1((med[1], min(times[1]), max(times[1]))),
                          native_over_callback=round(med[0] / med[1], 4), rel_diff=rel_diff(a, b))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="product,bilinear,points,solve")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_sm.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    for what in args.what.split(","):
        if what == "solve":
            solve(args, "cuda", gen)
        elif what == "product":
            product(args, "cuda", gen)
        else:
            derivatives(args, "cuda", gen, what)


if __name__ == "__main__":
    main()
