#!/usr/bin/env python3
"""The matrix-free rational-quadratic and periodic kernels (csrc/lo_kernel_param.hip, LO_OP_KERNEL_PARAM_DIAG): the three
entry points against what they replace, on the same inputs, the two (or three) taking turns over several rounds (median
round, spread next to it; device events after warm-up).

  product   lo_kernel_param_mv_f32 (1 and 17 columns)  against  ONE matmul with the stored dense matrix (forming the matrix
            is not timed: the comparison favours the stored route)  and against  the general path, the operator's `_matmul`
            with the gate patched shut: covar_func evaluated densely inside the product
  bilinear  lo_kernel_param_bilinear_f32               against  autograd through the dense function for the parameters
  points    lo_kernel_param_points_grad_f32            against  autograd through the dense function for x1
  solve     one preconditioned solve of ParamKernel + D at 1 x 8192 (D 4): the native descriptor against the dense
            callback route (the gate patched shut); a fresh operator per solve, host clock around a synchronise

Shapes 1 x 16384 (D 4) and 8 x 8192 (D 16).  The dense function of the periodic kernel holds [M, N, D] intermediates (64
GiB per tensor at the second shape), so every dense route runs member by member.  No routing rests on these numbers: inside
its gate the kernel is always taken, its purpose is memory.
Usage:  python tools/mb_kernel_param.py [--what product,bilinear,points,solve] [--families rq,periodic] [--reps 20] [--rounds 5]
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

SHAPES = ((1, 16384, 4), (8, 8192, 16))  # (B, n, D)
COLS = (1, 17)
DERIV_COLS = 8
SOLVE = (1, 8192, 4)
NB = {"outputscale": 0, "alpha": 0}
SHAPE = {"rq": "alpha", "periodic": "period_length"}


def r1(t):
    return [round(x, 1) for x in t]


def make(family, B, n, D, gen, dev):
    """(x, the parameters by name, theta): points over three periods / the unit cube."""
    p = {"outputscale": (0.8 + 0.6 * torch.rand(B, generator=gen)).to(dev)}
    if family == "rq":
        x = torch.rand(B, n, D, generator=gen).to(dev)
        p["lengthscale"] = (0.3 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
        p["alpha"] = (0.5 + 2.5 * torch.rand(B, generator=gen)).to(dev)
    else:
        x = (3.0 * torch.rand(B, n, D, generator=gen)).to(dev)
        p["lengthscale"] = (D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
        p["period_length"] = (0.8 + 0.4 * torch.rand(B, 1, D, generator=gen)).to(dev)
    theta = K.kernel_param_theta(p["lengthscale"], p["outputscale"], (B,), D, alpha=p.get("alpha"),
                                 period_length=p.get("period_length"))
    return x, p, theta


def member(p, b):
    return {k: v[b:b + 1] for k, v in p.items()}


def dense_fn(family, x1, x2, p):
    return covariance.PARAM_FAMILIES[family](x1, x2, p["lengthscale"], p["outputscale"], p[SHAPE[family]])


def rel_diff(a, b):
    return ((a - b).norm() / b.norm()).item()


def product(args, dev, gen, family):
    fam = covariance.PARAM_FAMILIES[family].native_family
    for B, n, D in SHAPES:
        x, p, theta = make(family, B, n, D, gen, dev)
        stored = torch.cat([dense_fn(family, x[b:b + 1], x[b:b + 1], member(p, b)) for b in range(B)])
        members = [KernelLinearOperator(x[b:b + 1], x[b:b + 1], covariance.PARAM_FAMILIES[family],
                                        num_nonbatch_dimensions=NB, **member(p, b)) for b in range(B)]
        for c in COLS:
            V = torch.randn(B, n, c, generator=gen).to(dev)
            native = lambda: K.kernel_param_mv(x, x, theta, fam, V)  # noqa: E731
            dense = lambda: stored @ V  # noqa: E731

            def general():
                with mock.patch.object(KernelLinearOperator, "_native_param_refusal", return_value="switched off"):
                    return torch.cat([op._matmul(V[b:b + 1]) for b, op in enumerate(members)])

            times = alternated([native, dense, general], args.reps, args.rounds)
            print(json.dumps(dict(
                what="product", family=family, B=B, n=n, D=D, c=c, native_us=r1(times[0]), stored_matmul_us=r1(times[1]),
                general_path_us=r1(times[2]), native_over_stored=round(times[0][0] / times[1][0], 3),
                native_over_general=round(times[0][0] / times[2][0], 4),
                native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=rel_diff(native(), dense()))), flush=True)
        del stored


def derivatives(args, dev, gen, family, what):
    fam = covariance.PARAM_FAMILIES[family].native_family
    for B, n, D in SHAPES:
        x, p, theta = make(family, B, n, D, gen, dev)
        U = torch.randn(B, n, DERIV_COLS, generator=gen).to(dev)
        V = torch.randn(B, n, DERIV_COLS, generator=gen).to(dev)

        def autograd(points):
            grads = []
            for b in range(B):
                xb, pb = x[b:b + 1], member(p, b)
                if points:
                    leaf = xb.detach().clone().requires_grad_(True)
                    (U[b:b + 1] * (dense_fn(family, leaf, xb, pb) @ V[b:b + 1])).sum().backward()
                    grads.append(leaf.grad)
                else:
                    pb = {k: v.detach().clone().requires_grad_(True) for k, v in pb.items()}
                    (U[b:b + 1] * (dense_fn(family, xb, xb, pb) @ V[b:b + 1])).sum().backward()
                    grads.append(pb["outputscale"].grad)
            return torch.cat(grads)

        if what == "bilinear":
            native = lambda: K.kernel_param_bilinear(x, x, theta, fam, U, V)  # noqa: E731
            dense = lambda: autograd(False)  # noqa: E731
            diff = rel_diff(native()[:, D] * 2.0 * p["outputscale"], dense())  # (d os = 2 os d os^2)
        else:
            native = lambda: K.kernel_param_points_grad(x, x, theta, fam, U, V)  # noqa: E731
            dense = lambda: autograd(True)  # noqa: E731
            diff = rel_diff(native(), dense())
        times = alternated([native, dense], max(args.reps // 4, 2), args.rounds)
        print(json.dumps(dict(
            what=what, family=family, B=B, n=n, D=D, t=DERIV_COLS, native_us=r1(times[0]), dense_autograd_us=r1(times[1]),
            native_over_autograd=round(times[0][0] / times[1][0], 4),
            native_gpairs_s=round(B * n * n / times[0][0] / 1e3, 1), rel_diff=diff)), flush=True)


def solve(args, dev, gen, family):
    B, n, D = SOLVE
    x, p, _ = make(family, B, n, D, gen, dev)
    noise = (0.05 + 0.1 * torch.rand(B, n, generator=gen)).to(dev)
    rhs = torch.randn(B, n, 1, generator=gen).to(dev)

    def run():
        kern = KernelLinearOperator(x, x, covariance.PARAM_FAMILIES[family], num_nonbatch_dimensions=NB, **p)
        out = AddedDiagLinearOperator(kern, DiagLinearOperator(noise)).solve(rhs)
        torch.cuda.synchronize()
        return out

    def callback():  # (the gate shut: the operator as it was before the kind existed)
        with mock.patch.object(KernelLinearOperator, "_native_param_refusal", return_value="switched off"):
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
    print(json.dumps(dict(what="solve", family=family, B=B, n=n, D=D,
                          native_us=r1((med[0], min(times[0]), max(times[0]))),
                          callback_us=r1((med[1], min(times[1]), max(times[1]))),
                          native_over_callback=round(med[0] / med[1], 4), rel_diff=rel_diff(a, b))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--what", default="product,bilinear,points,solve")
    ap.add_argument("--families", default="rq,periodic")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_param.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    for family in args.families.split(","):
        for what in args.what.split(","):
            if what == "solve":
                solve(args, "cuda", gen, family)
            elif what == "product":
                product(args, "cuda", gen, family)
            else:
                derivatives(args, "cuda", gen, family, what)


if __name__ == "__main__":
    main()
