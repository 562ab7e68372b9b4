#!/usr/bin/env python3
"""Additive-SKI microbenchmark: the kind LO_OP_SKI_SUM_DIAG (csrc/lo_ski_sum.hip) against the composition
SumBatchLinearOperator runs otherwise (v expanded to [P, N, c], the batched SKI product, a reduction of the [P, N, c]
result), the descriptor forced to None in the same process -- the route of a commit without the kind.  Device events
after warm-up, the two alternated over several rounds (the median round is reported, the range next to it); per-kernel
times (lo_prof) with bytes / FLOPs from the shapes; the preconditioned AddedDiag.solve and inv_quad_logdet forward +
backward both ways, with the float64 residual of the solve.

Shapes: S1 (1 x 262144, P 8, M 8192, J 4), S2 (16 x 16384, P 4, M 2048, J 4); 1 and 17 columns.
Usage:  python tools/mb_ski_sum.py [--reps 20] [--rounds 5] [--shapes S1,S2] [--no-solve]
Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from make_golden_ski import column, interp  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, InterpolatedLinearOperator, SumBatchLinearOperator,
    ToeplitzLinearOperator)
from linear_operator_amd.operators import added_diag_linear_operator as adl  # noqa: E402

SHAPES = {"S1": (1, 262144, 8, 8192, 4), "S2": (16, 16384, 4, 2048, 4)}  # B, N, P, M, J


class Composed(SumBatchLinearOperator):
    """The same operator with the lowering switched off: every product is the Python composition."""

    def _kernel_descriptor(self, batch_shape=None):
        return None


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def alternated(fns, reps, rounds, warm=3):
    """Median and (min, max) over `rounds` of the per-call time of every function, the functions taking turns."""
    for fn in fns:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(timed(fn, reps))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def model(B, N, P, M, J, c):
    """(bytes, FLOPs) per kernel of one product, from the shapes.  W^T v: the copy of W_r (ids, values) and v's rows
    gathered once per entry, u written; T u: u read and T u written per split, the column; the summing gather: indices,
    values and J gathered rows of T u per term, v and d read, y written."""
    G = B * P
    return {
        "ski_interp_t": (G * N * J * (4 + 4 + 4 * c) + G * M * c * 4, 2 * G * N * J * c),
        "ski_toeplitz_mv": (2 * G * M * c * 4 + G * M * 4, 2 * G * M * M * c),
        "ski_interp_sum": (G * N * J * (8 + 4 + 4 * c) + 2 * B * N * c * 4 + B * N * 4, 2 * G * N * J * c + 2 * B * N * c),
    }


def build(name, dev):
    B, N, P, M, J = SHAPES[name]
    col = np.stack([column(100 + p, B, M, ls=0.01 + 0.004 * p) for p in range(P)], 1)
    parts = [interp(200 + p, B, N, M, J, cubic=True) for p in range(P)]
    li, lv = np.stack([t[0] for t in parts], 1), np.stack([t[1] for t in parts], 1)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    return T(col), T(li), T(lv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="S1,S2")
    ap.add_argument("--no-solve", action="store_true")
    args = ap.parse_args()
    dev = "cuda"
    for name in args.shapes.split(","):
        B, N, P, M, J = SHAPES[name]
        col, li, lv = build(name, dev)

        def ops(col=col, lvl=lv, lvr=lv):
            base = InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lvl, li, lvr)
            return SumBatchLinearOperator(base), Composed(base)

        A, comp = ops()
        for c in (1, 17):
            v = torch.randn(B, N, c, device=dev)
            desc = A._kernel_descriptor(torch.Size([B]))
            assert desc is not None and desc.kind == K._hip.LO_OP_SKI_SUM_DIAG
            # the kernel whatever the routing table says: the table is filled from this measurement
            mv = lambda: K.matvec(desc, v)  # noqa: E731
            cm = lambda: comp._matmul_composition(v)  # noqa: E731
            tn, tc = alternated([mv, cm], args.reps, args.rounds)
            y_ref = cm()
            err = ((mv() - y_ref).norm() / y_ref.norm()).item()
            routed = bool(K.NATIVE_MATMUL_SKI_SUM.get(1 if c == 1 else 2, False))
            print(json.dumps(dict(shape=name, B=B, N=N, P=P, M=M, J=J, c=c, native_us=round(tn[0], 1),
                                  native_range=[round(tn[1], 1), round(tn[2], 1)], composition_us=round(tc[0], 1),
                                  composition_range=[round(tc[1], 1), round(tc[2], 1)],
                                  speedup=round(tc[0] / tn[0], 2), routed_to_kernel=routed, rel_diff=err)), flush=True)
            K._hip.prof_enable(True)
            K._hip.prof_report()
            for _ in range(args.reps):
                mv()
            torch.cuda.synchronize()
            prof = K._hip.prof_report()
            K._hip.prof_enable(False)
            for kname, (nb, nf) in model(B, N, P, M, J, c).items():
                if kname in prof:
                    cnt, ms = prof[kname]
                    us = ms / cnt * 1e3
                    print(json.dumps(dict(shape=name, c=c, kernel=kname, us=round(us, 1), bytes=nb, flops=nf,
                                          gbs=round(nb / us / 1e3, 1), gflops=round(nf / us / 1e3, 1))), flush=True)
        if args.no_solve:
            continue
        # the preconditioned solve and inv_quad_logdet forward + backward, both ways (pivoted Cholesky + preconditioner
        # + CG / Lanczos quadrature; the preconditioner memo cleared per call)
        sig = torch.full((B, 1), 0.05, device=dev)  # (stiff on purpose: both routes run into the iteration cap)
        rhs = torch.randn(B, N, 1, device=dev)

        def solve(op):
            adl.clear_preconditioner_memo()
            with settings.cg_tolerance(1e-3), settings.max_cg_iterations(200):
                return AddedDiagLinearOperator(op, ConstantDiagLinearOperator(sig, N)).solve(rhs)

        def iql(native):
            adl.clear_preconditioner_memo()
            colg, lvg = col.clone().requires_grad_(True), lv.clone().requires_grad_(True)
            op = ops(colg, lvg, lvg)[0 if native else 1]
            with settings.cg_tolerance(1e-3), settings.max_cg_iterations(200), settings.num_trace_samples(10):
                iq, ld = AddedDiagLinearOperator(op, ConstantDiagLinearOperator(sig, N)).inv_quad_logdet(rhs, logdet=True)
                (iq.sum() + ld.sum()).backward()
            return iq, ld

        def residual(x):
            """|| (K + sigma) x - rhs || / || rhs || with the product of the composition in float64."""
            base64 = InterpolatedLinearOperator(ToeplitzLinearOperator(col.double()), li, lv.double(), li, lv.double())
            r = SumBatchLinearOperator(base64)._matmul(x.double()) + sig.double().unsqueeze(-1) * x.double() - rhs.double()
            return (r.norm() / rhs.double().norm()).item()

        res = alternated([lambda: solve(A), lambda: solve(comp)], 2, 3, warm=1)
        print(json.dumps(dict(shape=name, what="preconditioned AddedDiag.solve, 1 column",
                              native_ms=round(res[0][0] / 1e3, 2), native_range=[round(t / 1e3, 2) for t in res[0][1:]],
                              composition_ms=round(res[1][0] / 1e3, 2),
                              composition_range=[round(t / 1e3, 2) for t in res[1][1:]],
                              native_residual=residual(solve(A)), composition_residual=residual(solve(comp)))),
              flush=True)
        res = alternated([lambda: iql(True), lambda: iql(False)], 2, 3, warm=1)
        print(json.dumps(dict(shape=name, what="inv_quad_logdet forward + backward",
                              native_ms=round(res[0][0] / 1e3, 2), native_range=[round(t / 1e3, 2) for t in res[0][1:]],
                              composition_ms=round(res[1][0] / 1e3, 2),
                              composition_range=[round(t / 1e3, 2) for t in res[1][1:]])), flush=True)


if __name__ == "__main__":
    main()
