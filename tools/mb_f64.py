#!/usr/bin/env python3
"""Microbenchmark of the float64 structured operators: for one shape,
  (a) the native product lo_matvec_f64 for 1 and 17 columns against the ATen composition the operator's `_matmul`
      otherwise runs (the routing table _NATIVE_MATMUL_F64 of kernels.py is switched off for the measurement), and
  (b) one preconditioned float64 `A.solve(rhs)` (CG; the preconditioner comes from the memo after the warm-up).
Shapes:  lowrank  64 x 8192 x 32 + Diag       kron  16 x (128 (x) 128) + sigma^2 I       sum  LowRankRoot(R 16) + Dense, N 4096, B 4
Five repetitions of `--inner` calls each between HIP events, after two warm-up repetitions; prints one JSON line with the
median and the (min, max) spread in microseconds per call.  A checkout of an earlier commit (binding ABI < 22) measures
(b) only: run the tool with PYTHONPATH pointing at that checkout to get the baseline of the same visit.
Usage:  python tools/mb_f64.py --shape lowrank|kron|sum [--reps 5] [--inner 10]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import warnings

import numpy as np
import torch

if not any(os.path.isdir(os.path.join(p, "linear_operator_amd")) for p in sys.path if p):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import linear_operator_amd as lo  # noqa: E402
import linear_operator_amd.operators as ops  # noqa: E402
from linear_operator_amd import _hip, kernels as K  # noqa: E402


def build(shape, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def randn(*s):
        return torch.randn(*s, generator=g, device=dev, dtype=torch.float64)

    def spd(B, n):
        X = randn(B, n, n) / n ** 0.5
        return X @ X.mT + 0.1 * torch.eye(n, device=dev, dtype=torch.float64)

    if shape == "lowrank":
        B, N, R = 64, 8192, 32
        C, d = randn(B, N, R) / R ** 0.5, torch.rand(B, N, generator=g, device=dev, dtype=torch.float64) + 0.5
        return ops.AddedDiagLinearOperator(ops.LowRankRootLinearOperator(C), ops.DiagLinearOperator(d)), B, N, 2 * B * N * R * 8
    if shape == "kron":
        B, n = 16, 128
        A = ops.AddedDiagLinearOperator(
            ops.KroneckerProductLinearOperator(ops.DenseLinearOperator(spd(B, n)), ops.DenseLinearOperator(spd(B, n))),
            ops.ConstantDiagLinearOperator(torch.full((B, 1), 0.5, device=dev, dtype=torch.float64), diag_shape=n * n))
        return A, B, n * n, 0
    B, N, R = 4, 4096, 16
    d = torch.rand(B, N, generator=g, device=dev, dtype=torch.float64) + 0.5
    A = ops.AddedDiagLinearOperator(ops.SumLinearOperator(ops.LowRankRootLinearOperator(randn(B, N, R) / R ** 0.5),
                                                          ops.DenseLinearOperator(spd(B, N))), ops.DiagLinearOperator(d))
    return A, B, N, 0


def timed(fn, reps, inner):
    """Microseconds per call: median and (min, max) of `reps` repetitions of `inner` calls, after two warm-up ones."""
    out = []
    for rep in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        if rep >= 2:
            out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("lowrank", "kron", "sum"), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    A, B, N, lowrank_bytes = build(a.shape, dev)
    res = {"shape": a.shape, "B": B, "N": N, "abi": _hip.ABI_VERSION, "reps": a.reps, "inner": a.inner}
    native = _hip.ABI_VERSION >= 22
    if native:
        table = dict(K._NATIVE_MATMUL_F64)
        K._NATIVE_MATMUL_F64.clear()  # `_matmul` below is the ATen composition, whatever the table ships with
        desc = A._kernel_descriptor()
        assert desc is not None and desc.dtype == torch.float64
        for c in (1, 17):
            v = torch.randn(B, N, c, device=dev, dtype=torch.float64)
            err = float((K.matvec(desc, v) - A._matmul(v)).abs().max())
            res[f"matvec_c{c}_native"] = timed(lambda: K.matvec(desc, v), a.reps, a.inner)
            res[f"matvec_c{c}_aten"] = timed(lambda: A._matmul(v), a.reps, a.inner)
            res[f"matvec_c{c}_maxdiff"] = err
            if lowrank_bytes:
                byts = lowrank_bytes + 2 * B * N * c * 8
                res[f"matvec_c{c}_native_gbs"] = round(byts / res[f"matvec_c{c}_native"]["median_us"] / 1e3, 1)
        if lowrank_bytes:
            res["hbm_copy_gbs"] = round(_hip.hbm_stream_gbs(dev, "copy", n_floats=1 << 26), 1)
        K._NATIVE_MATMUL_F64.update(table)
    rhs = torch.randn(B, N, 1, device=dev, dtype=torch.float64)
    with lo.settings.max_cholesky_size(0), lo.settings.min_preconditioning_size(100), lo.settings.cg_tolerance(1e-6), \
            warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = A.solve(rhs)
        resid = float((A._matmul(x) - rhs).norm() / rhs.norm())
        res["solve"] = timed(lambda: A.solve(rhs), a.reps, max(1, a.inner // 5))
        res["solve_resid"] = resid
    print(json.dumps(res))


if __name__ == "__main__":
    main()
