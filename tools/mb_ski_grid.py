#!/usr/bin/env python3
"""SKI-grid microbenchmark: per-product time of the native LO_OP_SKI_GRID_DIAG `_matmul` (csrc/lo_ski_grid.hip) against
the composition the operator runs otherwise (left_t_interp -> per-factor Toeplitz products -> left_interp), the
descriptor forced to None in the same process; device events after warm-up, the two alternated over several rounds (the
median round is reported, the spread next to it); per-kernel times (lo_prof) with bytes / FLOPs from the shapes; one
preconditioned AddedDiag(SKI-grid, ConstantDiag).solve at S3 both ways.

Shapes: S3 (1 x 65536 on 128 (x) 128, J 16), B2 (16 x 16384 on 64 (x) 64, J 16), D3 (1 x 65536 on 32 (x) 32 (x) 32,
J 64); 1 and 17 columns.  Usage:  python tools/mb_ski_grid.py [--reps 50] [--rounds 5] [--composition-only]
(--composition-only: the composition alone, for the baseline of record on a commit without the kind.)  Prints one JSON
line per measurement.
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from make_golden_ski import column  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, InterpolatedLinearOperator, KroneckerProductLinearOperator,
    ToeplitzLinearOperator)
from linear_operator_amd.operators import interpolated_linear_operator as ilo  # noqa: E402

SHAPES = (("S3", 1, 65536, (128, 128)), ("B2", 16, 16384, (64, 64)), ("D3", 1, 65536, (32, 32, 32)))


class Composed(InterpolatedLinearOperator):
    """The same operator with the lowering switched off: every product is the Python composition."""

    def _kernel_descriptor(self, batch_shape=None):
        return None


def grid_interp_torch(seed, B, N, grid, dev):
    """Cubic-style interpolation on a D-dimensional grid: 4 consecutive points per axis, J = 4^D, weights the product of
    per-axis weights that sum to one."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = len(grid)
    idx = torch.zeros(B, N, 1, dtype=torch.long)
    vals = torch.ones(B, N, 1)
    for m in grid:
        base = (torch.rand(B, N, generator=g) * (m - 3)).floor().long().clamp_(0, m - 4)
        w = 0.1 + torch.rand(B, N, 4, generator=g)
        w = w / w.sum(-1, keepdim=True)
        idx = (idx.unsqueeze(-1) * m + (base[..., None, None] + torch.arange(4))).reshape(B, N, -1)
        vals = (vals.unsqueeze(-1) * w.unsqueeze(-2)).reshape(B, N, -1)
    assert idx.shape[-1] == 4 ** D
    return idx.to(dev), vals.to(dev)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # us


def alternated(fns, reps, rounds):
    """Median and (min, max) over `rounds` of the per-call time of every function, the functions taking turns."""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            times[k].append(timed(fn, reps))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def grid_model(B, grid, c):
    """(bytes, FLOPs) of the D axis passes of one grid product, from the shapes: every pass reads and writes the grid
    vector once (the re-reads of a line by the workgroups that share it hit the L2) and reads the lags."""
    M = 1
    for m in grid:
        M *= m
    nbytes = sum(2 * B * M * c * 4 + B * m * 4 for m in grid)
    return nbytes, 2 * B * M * c * sum(grid)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--composition-only", action="store_true")
    args = ap.parse_args()
    dev = "cuda"
    native = not args.composition_only
    for name, B, N, grid in SHAPES:
        cols = [torch.from_numpy(column(10 + k, 1, m, ls=0.05)[0]).to(dev) for k, m in enumerate(grid)]
        li, lv = grid_interp_torch(20, B, N, grid, dev)
        base = KroneckerProductLinearOperator(*[ToeplitzLinearOperator(t) for t in cols])
        comp = Composed(base, li, lv, li, lv)
        A = InterpolatedLinearOperator(base, li, lv, li, lv)
        for c in (1, 17):
            v = torch.randn(B, N, c, device=dev)
            if not native:
                (tc,) = alternated([lambda: comp._matmul(v)], args.reps, args.rounds)
                print(json.dumps(dict(shape=name, grid=grid, B=B, N=N, c=c, composition_us=round(tc[0], 1),
                                      composition_range=[round(tc[1], 1), round(tc[2], 1)])), flush=True)
                continue
            desc = A._kernel_descriptor(torch.Size([B]))
            assert desc is not None and desc.kind == K._hip.LO_OP_SKI_GRID_DIAG
            # the kernel whatever the routing table says: the table is filled from this measurement
            mv = lambda: K.matvec(desc, v)  # noqa: E731
            tn, tc = alternated([mv, lambda: comp._matmul(v)], args.reps, args.rounds)
            y_ref = comp._matmul(v)
            err = ((mv() - y_ref).norm() / y_ref.norm()).item()
            routed = bool(ilo._NATIVE_MATMUL.get((len(grid), 1 if c == 1 else 2), False))
            print(json.dumps(dict(shape=name, grid=grid, B=B, N=N, c=c, native_us=round(tn[0], 1),
                                  native_range=[round(tn[1], 1), round(tn[2], 1)], composition_us=round(tc[0], 1),
                                  composition_range=[round(tc[1], 1), round(tc[2], 1)],
                                  speedup=round(tc[0] / tn[0], 2), routed_to_kernel=routed, rel_diff=err)), flush=True)
            K._hip.prof_enable(True)
            for _ in range(args.reps):
                mv()
            torch.cuda.synchronize()
            prof = K._hip.prof_report()
            K._hip.prof_enable(False)
            nb, nf = grid_model(B, grid, c)
            for kname in ("ski_interp_t", "ski_grid_mv", "ski_interp"):
                if kname in prof:
                    cnt, ms = prof[kname]
                    rec = dict(shape=name, c=c, kernel=kname, us=round(ms / cnt * 1e3, 1))
                    if kname == "ski_grid_mv":
                        rec.update(bytes=nb, flops=nf, gbs=round(nb / (ms / cnt * 1e-3) / 1e9, 1),
                                   gflops=round(nf / (ms / cnt * 1e-3) / 1e9, 1))
                    print(json.dumps(rec), flush=True)
        if name != "S3":
            continue
        # one preconditioned solve at S3, both ways (pivoted Cholesky + preconditioner + CG, caches cleared per call)
        sig = torch.full((B, 1), 0.1, device=dev)
        rhs = torch.randn(B, N, 1, device=dev)

        def solve(op):
            from linear_operator_amd.operators import added_diag_linear_operator as adl

            adl.clear_preconditioner_memo()
            with settings.cg_tolerance(1e-3), settings.max_cg_iterations(200):
                return AddedDiagLinearOperator(op, ConstantDiagLinearOperator(sig, N)).solve(rhs)

        fns = [lambda: solve(comp)] + ([lambda: solve(A)] if native else [])
        res = alternated(fns, 3, 3)
        rec = dict(shape=name, what="preconditioned AddedDiag.solve, 1 column", composition_ms=round(res[0][0] / 1e3, 2))
        if native:
            rec.update(native_ms=round(res[1][0] / 1e3, 2),
                       rel_diff=((solve(A) - solve(comp)).norm() / solve(comp).norm()).item())
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
