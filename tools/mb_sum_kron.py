#!/usr/bin/env python3
"""Sum-of-Kronecker-products microbenchmark (csrc/lo_kron_eigsolve.hip, SumKroneckerLinearOperator), 1 and 17 columns:
  - y = scale o ((M1 (x) S2^T) z): the fused launch of lo_kron_eig_apply_f32 against the composition a cell of the
    routing table `kernels._NATIVE_KRON_EIG` that is not set runs (the Kronecker matvec kernels on (M1, S2^T) and one
    scale pass) and against the entry point's own general route (LO_KRON_EIG_NO_FUSED: transpose, Kronecker matvec,
    scale kernel);
  - `(Kron(A, B) + Kron(C, D)).solve(rhs)` end to end, set-up included (a new operator per call), against
    `SumLinearOperator(Kron(A, B), Kron(C, D)).solve(rhs)`: CG on LO_OP_SUM, what `+` built before the class existed.
Device events after warm-up, the alternatives taking turns over several rounds (median round, spread next to it).

Shapes: 1 x (4096 (x) 4), 64 x (512 (x) 8), 16 x (1024 (x) 16).
Usage:  python tools/mb_sum_kron.py [--reps 50] [--rounds 5] [--no-solve]     Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from unittest import mock

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mb_ski_grid import alternated, timed  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import KroneckerProductLinearOperator, SumLinearOperator  # noqa: E402

SHAPES = ((1, 4096, 4), (64, 512, 8), (16, 1024, 16))


def r1(t):
    return [round(x, 1) for x in t]


def rbf(B, n, ls, jitter, gen, dev):
    x = torch.rand(B, n, 2, generator=gen).to(dev)
    return torch.exp(-0.5 * torch.cdist(x, x) ** 2 / ls ** 2) + jitter * torch.eye(n, device=dev)


def task(B, n, gen, dev):
    f = torch.randn(B, n, n + 2, generator=gen).to(dev)
    return f @ f.mT / (n + 2) + 0.3 * torch.eye(n, device=dev)


def apply_model(B, n1, n2, c):
    """(bytes, FLOPs) the product needs, from the shapes: M1, S2, scale, z read once, y written once."""
    N = n1 * n2
    return 4 * B * (n1 * n1 + n2 * n2 + N + 2 * N * c), 2 * B * N * c * (n1 + n2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-solve", action="store_true")
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    for B, n1, n2 in SHAPES:
        N = n1 * n2
        M1 = torch.randn(B, n1, n1, generator=gen).to(dev) / n1 ** 0.5
        S2 = torch.randn(B, n2, n2, generator=gen).to(dev)
        scale = (0.5 + torch.rand(B, N, generator=gen)).to(dev)
        for c in (1, 17):
            z = torch.randn(B, N, c, generator=gen).to(dev)

            def general():
                with mock.patch.dict(os.environ, {"LO_KRON_EIG_NO_FUSED": "1"}):
                    return K.kron_eig_apply(M1, S2, scale, z, fused=True)

            fns = [lambda: K.kron_eig_apply(M1, S2, scale, z, fused=True),
                   lambda: K.kron_eig_apply(M1, S2, scale, z, fused=False), general]
            tf, tc, tg = alternated(fns, args.reps, args.rounds)
            y_f, y_c = fns[0](), fns[1]()
            nbytes, flops = apply_model(B, n1, n2, c)
            print(json.dumps(dict(what="kron_eig_apply", B=B, n1=n1, n2=n2, c=c, fused_us=r1(tf), composition_us=r1(tc),
                                  entry_general_us=r1(tg), speedup=round(tc[0] / tf[0], 2),
                                  routed_to_fused=K.kron_eig_routed(n2, c),
                                  fused_gb_s=round(nbytes / tf[0] / 1e3, 1), fused_gflop_s=round(flops / tf[0] / 1e3, 1),
                                  rel_diff=((y_f - y_c).norm() / y_c.norm()).item())), flush=True)
        if args.no_solve:
            continue
        A, Cm = rbf(B, n1, 0.3, 1e-3, gen, dev), rbf(B, n1, 0.05, 0.5, gen, dev)
        Bm, D = task(B, n2, gen, dev), task(B, n2, gen, dev)
        for c in (1, 17):
            rhs = torch.randn(B, N, c, generator=gen).to(dev)

            def closed():
                return (KroneckerProductLinearOperator(A, Bm) + KroneckerProductLinearOperator(Cm, D)).solve(rhs)

            def cg():
                return SumLinearOperator(KroneckerProductLinearOperator(A, Bm),
                                         KroneckerProductLinearOperator(Cm, D)).solve(rhs)

            x_closed, x_cg = closed(), cg()  # (warm-up)
            torch.cuda.synchronize()
            times = [[], []]
            for _ in range(3):
                for k, fn in enumerate((closed, cg)):
                    times[k].append(timed(fn, 2))
            plain = SumLinearOperator(KroneckerProductLinearOperator(A, Bm), KroneckerProductLinearOperator(Cm, D))
            resid = lambda x: ((plain._matmul(x) - rhs).norm() / rhs.norm()).item()  # noqa: E731
            op = KroneckerProductLinearOperator(A, Bm) + KroneckerProductLinearOperator(Cm, D)
            op._setup()
            t_apply = alternated([lambda: op._solve(rhs)], args.reps, args.rounds)[0]
            print(json.dumps(dict(what="solve end to end", B=B, n1=n1, n2=n2, c=c,
                                  closed_form_ms=[round(statistics.median(times[0]) / 1e3, 2),
                                                  round(min(times[0]) / 1e3, 2), round(max(times[0]) / 1e3, 2)],
                                  cg_on_sum_ms=[round(statistics.median(times[1]) / 1e3, 2),
                                                round(min(times[1]) / 1e3, 2), round(max(times[1]) / 1e3, 2)],
                                  closed_form_cached_setup_us=r1(t_apply),
                                  closed_form_residual=resid(x_closed), cg_residual=resid(x_cg))), flush=True)


if __name__ == "__main__":
    main()
