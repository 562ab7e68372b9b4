#!/usr/bin/env python3
"""Kronecker-of-Toeplitz microbenchmark (csrc/lo_ski_grid.hip, LO_OP_TOEPLITZ_KRON_DIAG), for 1 and 17 columns:
  - the native product against the per-factor composition `_matmul` runs otherwise (the descriptor forced to None in the
    same process), the diagonal term in the last pass and as an epilogue kernel (LO_TKRON_EPILOGUE);
  - one preconditioned AddedDiag(.., ConstantDiag).solve on the descriptor against the closure route (the route the
    same call takes on a commit without the kind);
  - `_bilinear_derivative` native against its torch closed form.
Device events after warm-up, the alternatives taking turns over several rounds (median round, spread next to it).

Shapes: S3 (1 x 128 (x) 128), B2 (16 x 64 (x) 64), D3 (1 x 32 (x) 32 (x) 32); S = 17 vector pairs for the gradients.
Usage:  python tools/mb_toeplitz_kron.py [--reps 50] [--rounds 5]     Prints one JSON line per measurement.
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_golden_ski import column  # noqa: E402
from mb_ski_grid import alternated  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, DiagLinearOperator, KroneckerProductLinearOperator,
    ToeplitzLinearOperator)
from linear_operator_amd.operators import kronecker_product_linear_operator as kpm  # noqa: E402

SHAPES = (("S3", 1, (128, 128)), ("B2", 16, (64, 64)), ("D3", 1, (32, 32, 32)))


class Composed(KroneckerProductLinearOperator):
    """The same operator with the lowering switched off: products are the per-factor composition, solvers take the
    closure route, the gradients the torch closed form."""

    def _kernel_descriptor(self, batch_shape=None):
        return None

    def _toeplitz_native(self, cols):
        return False


def r1(t):
    return [round(x, 1) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda"
    for name, B, grid in SHAPES:
        N = 1
        for m in grid:
            N *= m
        cols = [torch.from_numpy(column(10 + k, B, m, ls=0.05)).to(dev) for k, m in enumerate(grid)]
        A = KroneckerProductLinearOperator(*[ToeplitzLinearOperator(t) for t in cols])
        comp = Composed(*[ToeplitzLinearOperator(t) for t in cols])
        d = 0.5 + torch.rand(B, N, device=dev)
        for c in (1, 17):
            v = torch.randn(B, N, c, device=dev)
            desc = A._kernel_descriptor()
            assert desc is not None and desc.kind == K._hip.LO_OP_TOEPLITZ_KRON_DIAG
            with_d = AddedDiagLinearOperator(A, DiagLinearOperator(d))._kernel_descriptor()
            # the kernel whatever the routing table says: the table is filled from this measurement
            mv = lambda: K.matvec(desc, v)  # noqa: E731
            mvd = lambda: K.matvec(with_d, v)  # noqa: E731

            def mvd_epilogue():
                with mock.patch.dict(os.environ, {"LO_TKRON_EPILOGUE": "1"}):
                    return K.matvec(with_d, v)

            tn, tc, tf, te = alternated([mv, lambda: comp._matmul(v), mvd, mvd_epilogue], args.reps, args.rounds)
            y_ref = comp._matmul(v)
            routed = bool(kpm._NATIVE_MATMUL_TOEPLITZ.get((len(grid), 1 if c == 1 else 2), False))
            print(json.dumps(dict(shape=name, grid=grid, B=B, c=c, native_us=r1(tn), composition_us=r1(tc),
                                  speedup=round(tc[0] / tn[0], 2), routed_to_kernel=routed,
                                  diag_in_last_pass_us=r1(tf), diag_epilogue_us=r1(te),
                                  rel_diff=((mv() - y_ref).norm() / y_ref.norm()).item())), flush=True)
        # the column gradients, S = 17
        u, v = torch.randn(B, N, 17, device=dev), torch.randn(B, N, 17, device=dev)
        tn, tc = alternated([lambda: A._bilinear_derivative(u, v), lambda: comp._bilinear_derivative(u, v)],
                            max(args.reps // 5, 3), args.rounds)
        gn, gc = A._bilinear_derivative(u, v), comp._bilinear_derivative(u, v)
        print(json.dumps(dict(shape=name, what="_bilinear_derivative, S 17", native_us=r1(tn), torch_us=r1(tc),
                              speedup=round(tc[0] / tn[0], 2),
                              rel_diff=max(((a - b).norm() / b.norm()).item() for a, b in zip(gn, gc)))), flush=True)
        # one preconditioned solve per column class (pivoted Cholesky + preconditioner + CG, caches cleared per call)
        sig = torch.full((B, 1), 0.1, device=dev)
        for c in (1, 17):
            rhs = torch.randn(B, N, c, device=dev)

            def solve(op):
                from linear_operator_amd.operators import added_diag_linear_operator as adl

                adl.clear_preconditioner_memo()
                with settings.cg_tolerance(1e-3), settings.max_cg_iterations(200):
                    return AddedDiagLinearOperator(op, ConstantDiagLinearOperator(sig, N)).solve(rhs)

            res = alternated([lambda: solve(A), lambda: solve(comp)], 3, 3)
            print(json.dumps(dict(shape=name, what=f"preconditioned AddedDiag.solve, {c} column(s)",
                                  native_ms=round(res[0][0] / 1e3, 2), closure_ms=round(res[1][0] / 1e3, 2),
                                  rel_diff=((solve(A) - solve(comp)).norm() / solve(comp).norm()).item())), flush=True)


if __name__ == "__main__":
    main()
