#!/usr/bin/env python3
"""SKI microbenchmark: per-matvec time of the native LO_OP_SKI_DIAG path (csrc/lo_ski.hip) against a torch composition
of the reference's algorithm (gather, index_add, circulant torch.fft) on the same GPU, on device events after warm-up;
per-kernel times (lo_prof) with bytes / FLOPs from the shapes and their share of the spec peaks; inv_quad_logdet
forward + backward with probes fixed through `_probe_vectors_and_norms`, native against the closure path.

Shapes (B, N, M, J): S1 one large GP (1, 262144, 8192, 4), S2 a batch of GPs (64, 16384, 2048, 4), S3 a 2-D grid
(1, 65536, 128 x 128 Kronecker base, 16: the native path composes the interpolation kernels with the Kronecker
kernel).  Usage:  python tools/mb_ski.py [--reps 20]    Prints one JSON line per measurement.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

from make_golden_ski import column, interp  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, ConstantDiagLinearOperator, InterpolatedLinearOperator, KroneckerProductLinearOperator,
    ToeplitzLinearOperator)


def torch_ski(col, li, lv, v, M):
    """The reference's composition in torch: W^T v by index_add, T u by circulant FFT, W t by gather."""
    B, N, J = li.shape
    c = v.shape[-1]
    vals = (v.unsqueeze(-2) * lv.unsqueeze(-1)).reshape(B, N * J, c)
    u = torch.zeros(B, M, c, device=v.device).scatter_add_(1, li.reshape(B, N * J, 1).expand(B, N * J, c), vals)
    circ = torch.cat((col, col[..., 1:].flip(-1)), -1)  # [B, 2M-1]
    pad = torch.zeros(B, 2 * M - 1, c, device=v.device)
    pad[:, :M] = u
    t = torch.fft.ifft(torch.fft.fft(pad.mT) * torch.fft.fft(circ).unsqueeze(-2)).real.mT[:, :M]
    g = t.gather(1, li.reshape(B, N * J, 1).expand(B, N * J, c)).reshape(B, N, J, c)
    return (g * lv.unsqueeze(-1)).sum(-2)


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


HBM_PEAK = 8.0e12  # B/s, MI355X spec
FP32_PEAK = 157.3e12  # FLOP/s, MI355X spec (vector fp32)


def kernel_model(B, N, M, J, c, KS):
    """(bytes, FLOPs) per launch of the three kernels of one SKI matvec, from the shapes."""
    return {
        "ski_interp_t": (B * ((M + 1) * 4 + N * J * 8 + N * c * 4 + M * c * 4), 2 * B * N * J * c),
        "ski_toeplitz_mv": (B * (M * 4 + M * c * 4 + 2 * KS * M * c * 4 + M * c * 4), 2 * B * M * M * c),
        "ski_interp": (B * (N * J * 12 + M * c * 4 + N * c * 4), 2 * B * N * J * c),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda"
    for name, B, N, M, J in (("S1", 1, 262144, 8192, 4), ("S2", 64, 16384, 2048, 4)):
        col = torch.from_numpy(column(1, B, M, ls=0.01)).to(dev)
        li_np, lv_np = interp(2, B, N, M, J, cubic=True)
        li, lv = torch.from_numpy(li_np).to(dev), torch.from_numpy(lv_np).to(dev)
        A = InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, li, lv)
        for c in (1, 17):
            v = torch.randn(B, N, c, device=dev)
            # the operator's _matmul: the grid-major copy of W_r is built once and kept (kernels.interp_plan)
            nat = timed(lambda: A._matmul(v), args.reps)
            # lo_matvec_f32 with a descriptor that carries no kept copy: the copy is built inside every call
            desc = K.ski_diag_descriptor(col, li, lv, li, lv, None)
            fresh = timed(lambda: K.matvec(desc, v), args.reps)
            ref = timed(lambda: torch_ski(col, li, lv, v, M), args.reps)
            y_ref = torch_ski(col, li, lv, v, M)
            err = ((A._matmul(v) - y_ref).norm() / y_ref.norm()).item()
            torch.cuda.synchronize()
            K._hip.prof_enable(True)
            for _ in range(args.reps):
                A._matmul(v)
            torch.cuda.synchronize()
            prof = K._hip.prof_report()
            K._hip.prof_enable(False)
            print(json.dumps(dict(shape=name, c=c, native_us=round(nat, 1), native_build_per_call_us=round(fresh, 1),
                                  torch_us=round(ref, 1), speedup=round(ref / nat, 2), rel_err=err)), flush=True)
            for kname, (nb, nf) in kernel_model(B, N, M, J, c, _tz_slices(B, M)).items():
                if kname not in prof:
                    continue
                cnt, ms = prof[kname]
                t = ms / cnt * 1e-3
                print(json.dumps(dict(shape=name, c=c, kernel=kname, us=round(t * 1e6, 1), bytes=nb, flops=nf,
                                      hbm_share=round(nb / t / HBM_PEAK, 4), fp32_share=round(nf / t / FP32_PEAK, 4))),
                      flush=True)
        # inv_quad_logdet forward + backward with fixed probes, native vs the closure path (descriptor forced to None)
        sig = torch.full((B, 1), 0.01, device=dev)
        rhs = torch.randn(B, N, 1, device=dev)
        Z = torch.randn(B, N, 10, device=dev)

        class Probed(AddedDiagLinearOperator):
            def _probe_vectors_and_norms(self):  # (the reference's hook for fixed probes)
                n = Z.norm(dim=-2, keepdim=True)
                return Z / n, n

        class Closure(InterpolatedLinearOperator):
            def _kernel_descriptor(self, batch_shape=None):
                return None

        def iql(cls):
            c0 = col.clone().requires_grad_(True)
            A = Probed(cls(ToeplitzLinearOperator(c0), li, lv, li, lv), ConstantDiagLinearOperator(sig, N))
            iq, ld = A.inv_quad_logdet(rhs, logdet=True)
            (iq.sum() + ld.sum()).backward()
            return ld.detach()

        t_nat = timed(lambda: iql(InterpolatedLinearOperator), 3)
        t_clo = timed(lambda: iql(Closure), 3)
        d_ld = ((iql(InterpolatedLinearOperator) - iql(Closure)).abs().max()).item()
        print(json.dumps(dict(shape=name, what="inv_quad_logdet fwd+bwd, fixed probes", native_ms=round(t_nat / 1e3, 2),
                              closure_ms=round(t_clo / 1e3, 2), max_abs_logdet_diff=d_ld)), flush=True)
    # S3: 2-D grid, Kronecker(Toeplitz, Toeplitz) base
    B, N, J = 1, 65536, 16
    c1 = torch.from_numpy(column(3, 1, 128, ls=0.05)[0]).to(dev)
    li_np, lv_np = interp(4, B, N, 128 * 128, J)
    li, lv = torch.from_numpy(li_np).to(dev), torch.from_numpy(lv_np).to(dev)
    A = InterpolatedLinearOperator(KroneckerProductLinearOperator(ToeplitzLinearOperator(c1), ToeplitzLinearOperator(c1)),
                                   li, lv, li, lv)
    v = torch.randn(B, N, 1, device=dev)
    nat = timed(lambda: A._matmul(v), args.reps)
    print(json.dumps(dict(shape="S3", c=1, native_us=round(nat, 1), torch_us=None, note="composition: interp kernels "
                          "+ Kronecker product of Toeplitz factors")), flush=True)


def _tz_slices(B, M):
    """k slices of the Toeplitz product (tz_split in csrc/lo_ski.hip)."""
    RB = -(-M // 256)
    maxks = -(-M // 256)
    ks = max(1, min(-(-512 // (B * RB)), maxks))
    kchunk = -(-(-(-M // ks)) // 256) * 256
    return -(-M // kchunk)


if __name__ == "__main__":
    main()
