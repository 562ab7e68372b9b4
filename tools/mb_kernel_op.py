#!/usr/bin/env python3
"""Matrix-free kernel operator microbenchmark (csrc/lo_kernel_op.hip, LO_OP_KERNEL_DIAG): the on-the-fly product
lo_kernel_mv_f32 against the stored dense product of the SAME matrix (K evaluated once by the covariance function, then
lo_matvec_f32 on LO_OP_DENSE_DIAG, which streams 4 N^2 bytes per member), per family.  The largest shape has no dense
alternative (a stored K would be 64 GiB) and is timed alone.  Device events after warm-up, the alternatives taking turns
over several rounds (median round, spread next to it).

No routing decision depends on these numbers: the native path is taken whenever its gate holds, because its purpose is
memory; the table says what that costs or saves in time.
Usage:  python tools/mb_kernel_op.py [--reps 20] [--rounds 5] [--families rbf,matern52]   One JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mb_ski_grid import alternated  # noqa: E402

from linear_operator_amd import covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402

# (B, N, D, c, time the stored dense product too)
SHAPES = ((1, 16384, 4, 1, True), (1, 16384, 4, 17, True), (8, 8192, 16, 1, True), (1, 131072, 8, 1, False))


def r1(t):
    return [round(x, 1) for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--families", default="rbf,matern12,matern32,matern52")
    args = ap.parse_args()
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    for B, N, D, c, with_dense in SHAPES:
        x = torch.rand(B, N, D, generator=gen).to(dev)
        ls = (0.3 * D ** 0.5 * (0.7 + 0.6 * torch.rand(B, 1, D, generator=gen))).to(dev)
        os_ = (0.8 + 0.7 * torch.rand(B, generator=gen)).to(dev)
        v = torch.randn(B, N, c, generator=gen).to(dev)
        theta = K.kernel_theta(ls, os_, (B,), D)
        for name in args.families.split(","):
            fn = covariance.FAMILIES[name]
            fns = [lambda: K.kernel_mv(x, x, theta, fn.native_family, v)]
            dense_desc = None
            if with_dense:
                dense = torch.cat([fn(x[b:b + 1], x[b:b + 1], ls[b:b + 1], os_[b:b + 1]) for b in range(B)])
                dense_desc = K.dense_diag_descriptor(dense, None)
                fns.append(lambda: K.matvec(dense_desc, v))
            reps = args.reps if N <= 16384 else max(2, args.reps // 10)
            times = alternated(fns, reps, args.rounds)
            pairs = B * N * N
            out = dict(what="kernel_mv", family=name, B=B, N=N, D=D, c=c, native_us=r1(times[0]),
                       native_gpairs_s=round(pairs / times[0][0] / 1e3, 1),
                       stored_k_gib=round(4 * pairs / 2 ** 30, 2))
            if with_dense:
                y_n, y_d = fns[0](), fns[1]()
                out.update(dense_us=r1(times[1]), dense_gb_s=round(4 * pairs / times[1][0] / 1e3, 1),
                           native_over_dense=round(times[0][0] / times[1][0], 2),
                           rel_diff=((y_n - y_d).norm() / y_d.norm()).item())
                del dense, dense_desc
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
