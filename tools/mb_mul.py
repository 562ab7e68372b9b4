#!/usr/bin/env python3
"""Hadamard-root microbenchmark: per-matvec time of the native LO_OP_HADAMARD_DIAG path (csrc/lo_hadamard.hip) against
the torch composition of the reference's algorithm (the [N, p, t] broadcast through the right root's two GEMMs,
MulLinearOperator._matmul_composition) on the same GPU, on device events after warm-up; TFLOP/s as a share of the fp32
matrix peak; the solve forward + backward (AddedDiag(Mul, Diag), fixed rhs), native against the torch composition.

Shapes (B, N, p, q): S1 one large product (1, 65536, 100, 100), S2 a batch (16, 8192, 32, 32); t = 1 and 17 columns.
Usage:  python tools/mb_mul.py [--reps 20]    Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DiagLinearOperator, MulLinearOperator, RootLinearOperator)

FP32_MATRIX_PEAK = 157.3e12  # FLOP/s, MI355X spec (fp32 MFMA)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="S1,S2")
    args = ap.parse_args()
    shapes = {"S1": (1, 65536, 100, 100), "S2": (16, 8192, 32, 32)}
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in args.shapes.split(","):
        B, N, p, q = shapes[name]
        F = torch.randn(B, N, p, device="cuda", generator=g) / p ** 0.5
        G = torch.randn(B, N, q, device="cuda", generator=g) / q ** 0.5
        d = torch.full((B, N), 0.5, device="cuda")
        A = MulLinearOperator(RootLinearOperator(F), RootLinearOperator(G))
        desc = K.hadamard_diag_descriptor(F, G, None)
        for t in (1, 17):
            v = torch.randn(B, N, t, device="cuda", generator=g)
            nat = timed(lambda: K.matvec(desc, v), args.reps)
            ref = timed(lambda: A._matmul_composition(v), args.reps)
            yr = A._matmul_composition(v)
            err = float((K.matvec(desc, v) - yr).abs().max() / yr.abs().max())
            flops = 4.0 * B * N * p * q * t
            print(json.dumps(dict(shape=name, B=B, N=N, p=p, q=q, t=t, native_us=round(nat, 1), torch_us=round(ref, 1),
                                  speedup=round(ref / nat, 2), native_tflops=round(flops / nat / 1e6, 2),
                                  share_of_fp32_matrix_peak=round(flops / nat * 1e6 / FP32_MATRIX_PEAK, 3),
                                  max_rel_diff=err)), flush=True)
        # solve forward + backward: the native kind against the torch composition (closure CG, composed backward)
        rhs = torch.randn(B, N, 2, device="cuda", generator=g)

        def solve_fb():
            Fg, Gg, dg = (t.clone().requires_grad_(True) for t in (F, G, d))
            op = AddedDiagLinearOperator(MulLinearOperator(RootLinearOperator(Fg), RootLinearOperator(Gg)),
                                         DiagLinearOperator(dg))
            with settings.cg_tolerance(1e-4), settings.max_cg_iterations(200), settings.max_preconditioner_size(0):
                x = op.solve(rhs)
            (x * rhs).sum().backward()

        reps = max(2, args.reps // 5)
        t_nat = timed(solve_fb, reps)
        with mock.patch.object(MulLinearOperator, "_kernel_descriptor", lambda self, batch_shape=None: None), \
                mock.patch.object(MulLinearOperator, "_bilinear_derivative",
                                  MulLinearOperator._bilinear_derivative_composition):
            t_ref = timed(solve_fb, reps)
        print(json.dumps(dict(shape=name, what="solve fwd+bwd (2 rhs, no preconditioner, tol 1e-4)",
                              native_ms=round(t_nat / 1e3, 2), torch_composition_ms=round(t_ref / 1e3, 2),
                              speedup=round(t_ref / t_nat, 2))), flush=True)


if __name__ == "__main__":
    main()
