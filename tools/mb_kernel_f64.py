#!/usr/bin/env python3
"""Float64 matrix-free kernel operator microbenchmark (csrc/lo_kernel_op_f64.hip): lo_kernel_mv_f64 against

  stored    one torch.matmul with the stored float64 K (8 N^2 bytes per member, evaluated once outside the timing), and
  parent    what a float64 KernelLinearOperator did per product up to ABI 30: covar_func densely, then the matmul (one
            member at a time here, so that the [N, N, D] differences of the covariance function stay below 20 GiB; the
            operator itself evaluated the whole batch at once),

the same inputs, device events after warm-up, the routes taking turns, median of --rounds rounds of --reps calls with
min - max (a slow route is repeated fewer times per turn, never fewer turns; the counts are printed).  The fp32 kernel at the same shape is timed next to it (pairs/s and the float64 / float32 ratio).  The largest
shape has no stored alternative (128 GiB) and is timed alone.  --what derivs: lo_kernel_bilinear_f64 and the two
lo_kernel_points_grad_f64 calls against float64 autograd through the dense matrix on row blocks of at most 1 GiB of
differences.  --what solve: one preconditioned float64 solve of Kernel + Diag at 1 x 16384 on the descriptor route against
the parent's route (the float64 gate patched shut), residuals printed.

No route depends on these numbers: the float64 gate is taken whenever it holds, because its purpose is memory (DESIGN.md
section 6p).
Usage:  python tools/mb_kernel_f64.py [--what product,derivs,solve] [--reps 20] [--rounds 5] [--families rbf,matern52]
One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mb_kernel_op import alternated_within, r1  # noqa: E402

from linear_operator_amd import covariance, settings  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator  # noqa: E402

F64 = torch.float64
# (B, N, D, time the stored and the parent's product too)
SHAPES = ((1, 16384, 4, True), (8, 8192, 16, True), (1, 131072, 8, False))
COLS = (1, 17)
DERIV_SHAPES = ((1, 16384, 4, 1), (1, 16384, 4, 17), (8, 8192, 16, 1))
CHUNK_BYTES = 1 << 30


def draw(B, N, D, gen, dev):
    x = torch.rand(B, N, D, generator=gen, dtype=F64).to(dev)
    ls = (0.3 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen, dtype=F64))).to(dev)
    os_ = (0.8 + 0.7 * torch.rand(B, generator=gen, dtype=F64)).to(dev)
    return x, ls, os_


def per_member(fn, x, ls, os_, v):
    return torch.cat([fn(x[b:b + 1], x[b:b + 1], ls[b:b + 1], os_[b:b + 1]) @ v[b:b + 1] for b in range(x.shape[0])])


def product(args, dev, gen):
    for B, N, D, with_dense in SHAPES:
        x, ls, os_ = draw(B, N, D, gen, dev)
        theta = K.kernel_theta(ls, os_, (B,), D, dtype=F64)
        x32, theta32 = x.float(), theta.float()
        for c in COLS:
            v = torch.randn(B, N, c, generator=gen, dtype=F64).to(dev)
            v32 = v.float()
            for name in args.families.split(","):
                fn = covariance.FAMILIES[name]
                fam = fn.native_family
                fns = [lambda: K.kernel_mv(x, x, theta, fam, v), lambda: K.kernel_mv(x32, x32, theta32, fam, v32)]
                if with_dense:
                    dense = torch.cat([fn(x[b:b + 1], x[b:b + 1], ls[b:b + 1], os_[b:b + 1]) for b in range(B)])
                    fns += [lambda: torch.matmul(dense, v), lambda: per_member(fn, x, ls, os_, v)]
                reps = args.reps if N <= 16384 else max(2, args.reps // 10)
                times, per = alternated_within(fns, reps, args.rounds, turn_us=3e5)
                pairs = B * N * N
                out = dict(what="kernel_mv_f64", family=name, B=B, N=N, D=D, c=c, native_us=r1(times[0]),
                           native_gpairs_s=round(pairs / times[0][0] / 1e3, 2), fp32_us=r1(times[1]),
                           f64_over_f32=round(times[0][0] / times[1][0], 2), calls_per_turn=per,
                           stored_k_gib=round(8 * pairs / 2 ** 30, 2))
                if with_dense:
                    y_n, y_d = fns[0](), fns[2]()
                    out.update(stored_us=r1(times[2]), parent_us=r1(times[3]),
                               native_over_stored=round(times[0][0] / times[2][0], 2),
                               native_over_parent=round(times[0][0] / times[3][0], 4),
                               rel_diff=((y_n - y_d).norm() / y_d.norm()).item())
                    del dense
                print(json.dumps(out), flush=True)


def chunked_autograd(fn, x1, x2, ls, os_, U, V):
    """d / d (x1, x2, lengthscale, outputscale) of sum_s u_s^T K v_s by float64 autograd through the dense matrix, on
    blocks of rows."""
    B, M, D = x1.shape
    N = x2.shape[1]
    rows = max(1, min(M, CHUNK_BYTES // (B * N * D * 8)))
    g1, g2, gl, go = torch.zeros_like(x1), torch.zeros_like(x2), torch.zeros_like(ls), torch.zeros_like(os_)
    for lo in range(0, M, rows):
        hi = min(M, lo + rows)
        with torch.enable_grad():
            a = x1[:, lo:hi].clone().requires_grad_(True)
            b, l_, o_ = (t.clone().requires_grad_(True) for t in (x2, ls, os_))
            loss = (U[:, lo:hi] * (fn(a, b, l_, o_) @ V)).sum()
            ga, gb, dl, do = torch.autograd.grad(loss, [a, b, l_, o_])
        g1[:, lo:hi] = ga
        g2 += gb
        gl += dl
        go += do
    return g1, g2, gl, go


def derivatives(args, dev, gen):
    for B, N, D, t in DERIV_SHAPES:
        x, ls, os_ = draw(B, N, D, gen, dev)
        U = torch.randn(B, N, t, generator=gen, dtype=F64).to(dev)
        V = torch.randn(B, N, t, generator=gen, dtype=F64).to(dev)
        theta = K.kernel_theta(ls, os_, (B,), D, dtype=F64)
        for name in args.families.split(","):
            fn = covariance.FAMILIES[name]
            fam = fn.native_family
            fns = [lambda: K.kernel_bilinear(x, x, theta, fam, U, V),
                   lambda: (K.kernel_points_grad(x, x, theta, fam, U, V), K.kernel_points_grad(x, x, theta, fam, V, U)),
                   lambda: chunked_autograd(fn, x, x, ls, os_, U, V)]
            times, per = alternated_within(fns, args.reps, args.rounds, turn_us=3e5)
            g, (p1, p2), (a1, a2, al, _) = fns[0](), fns[1](), fns[2]()
            d_ls = (-(theta[:, :D] ** 2) * g[:, :D])[:, None, :]
            pairs = B * N * N
            print(json.dumps(dict(
                what="kernel_derivs_f64", family=name, B=B, N=N, D=D, t=t, bilinear_us=r1(times[0]),
                points_grad_both_sides_us=r1(times[1]), autograd_us=r1(times[2]), calls_per_turn=per,
                bilinear_gpairs_s=round(pairs / times[0][0] / 1e3, 2),
                points_gpairs_s=round(2 * pairs / times[1][0] / 1e3, 2),
                native_over_autograd=round((times[0][0] + times[1][0]) / times[2][0], 4),
                rel_diff_ls=((d_ls - al).norm() / al.norm()).item(), rel_diff_x1=((p1 - a1).norm() / a1.norm()).item(),
                rel_diff_x2=((p2 - a2).norm() / a2.norm()).item())), flush=True)


def solve(args, dev, gen):
    from linear_operator_amd.operators.added_diag_linear_operator import clear_preconditioner_memo

    B, N, D = 1, 16384, 4
    x, ls, os_ = draw(B, N, D, gen, dev)
    noise = (0.05 + 0.1 * torch.rand(B, N, generator=gen, dtype=F64)).to(dev)
    rhs = torch.randn(B, N, 1, generator=gen, dtype=F64).to(dev)
    for name in args.families.split(","):
        fn = covariance.FAMILIES[name]
        A = AddedDiagLinearOperator(KernelLinearOperator(x, x, fn, num_nonbatch_dimensions={"outputscale": 0},
                                                         lengthscale=ls, outputscale=os_), DiagLinearOperator(noise))
        out = dict(what="kernel_solve_f64", family=name, B=B, N=N, D=D, cg_tolerance=args.cg_tolerance)
        real = KernelLinearOperator._native_f64_refusal
        for route in ("descriptor", "parent"):
            if route == "parent":
                KernelLinearOperator._native_f64_refusal = lambda self, check_device=True: "shut"
            try:
                ms = []
                with settings.max_cholesky_size(0), settings.cg_tolerance(args.cg_tolerance), warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    for _ in range(1 + args.solve_rounds):
                        clear_preconditioner_memo()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        sol = A.solve(rhs)
                        torch.cuda.synchronize()
                        ms.append((time.perf_counter() - t0) * 1e3)
            finally:
                KernelLinearOperator._native_f64_refusal = real
            resid = rhs - (K.kernel_mv(x, x, K.kernel_theta(ls, os_, (B,), D, dtype=F64), fn.native_family, sol)
                           + noise.unsqueeze(-1) * sol)
            ms = sorted(ms[1:])  # (the first call warms up)
            out[route + "_ms"] = [round(ms[len(ms) // 2], 2), round(ms[0], 2), round(ms[-1], 2)]
            out[route + "_rel_residual"] = (resid.norm() / rhs.norm()).item()
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--solve-rounds", type=int, default=3)
    ap.add_argument("--cg-tolerance", type=float, default=1e-2)
    ap.add_argument("--families", default="rbf,matern52")
    ap.add_argument("--what", default="product,derivs,solve")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mb_kernel_f64.py measures on the device; none is available")
    gen = torch.Generator().manual_seed(0)
    what = args.what.split(",")
    if "product" in what:
        product(args, "cuda", gen)
    if "derivs" in what:
        derivatives(args, "cuda", gen)
    if "solve" in what:
        solve(args, "cuda", gen)


if __name__ == "__main__":
    main()
