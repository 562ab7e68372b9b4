#!/usr/bin/env python3
"""Generate the golden vectors tests/golden/g32_block_*.npz of BlockDiagLinearOperator, BlockInterleavedLinearOperator,
SumBatchLinearOperator and `LinearOperator.sum` by running the REAL reference.

Runs only where the reference is importable (like make_golden_mul.py); only the .npz outputs are committed.  Inputs come
from block_inputs() below (numpy PCG64, seeded); the tests call it and build the same operators from this package.
Usage:  python tests/golden/make_golden_block.py [path of the reference checkout]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G, T, N = 2, 3, 12
KINDS = (("bd", "BlockDiagLinearOperator"), ("bi", "BlockInterleavedLinearOperator"), ("sb", "SumBatchLinearOperator"))


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def normal(seed, *shape, scale=1.0):
    return (scale * rng(seed).standard_normal(shape)).astype(np.float32)


def spd(seed, *batch, n):
    a = rng(seed).standard_normal((*batch, n, n))
    return (a @ a.swapaxes(-1, -2) / n + np.eye(n)).astype(np.float32)


def block_inputs():
    """Every input of the fixtures, by name (the tests call this too)."""
    d = {}
    d["M"] = normal(4001, G, T, N, N, scale=N ** -0.5)  # general blocks: products, transposes, indexing, sums
    d["M4"] = normal(4002, T, G, N, N, scale=N ** -0.5)  # the block dimension first
    d["K"] = spd(4003, G, T, n=N)  # positive definite blocks: solves, log-determinants
    d["K2"] = spd(4004, G, T, n=N)
    d["R"] = normal(4006, G, T, N, 4)
    d["dg"] = (0.5 + rng(4005).random((G, T, N))).astype(np.float32)
    d["c"] = np.array(1.7, np.float32)
    for k in ("bd", "bi"):
        d[k + "_rhs1"] = normal(4010, G, T * N, 1)
        d[k + "_rhs3"] = normal(4011, G, T * N, 3)
    d["sb_rhs1"] = normal(4012, G, N, 1)
    d["sb_rhs3"] = normal(4013, G, N, 3)
    # scattered entries: on the diagonal blocks, off them (zeros), first and last row
    d["ix_rows"] = np.array([0, 5, 35, 13, 7, 24, 11], np.int64)
    d["ix_cols"] = np.array([3, 5, 0, 14, 31, 26, 12], np.int64)
    d["ix_batch"] = np.array([0, 1, 1, 0, 1, 0, 1], np.int64)
    d["sb_rows"] = np.array([0, 5, 11, 3, 7], np.int64)
    d["sb_cols"] = np.array([3, 5, 0, 11, 7], np.int64)
    d["sb_batch"] = np.array([0, 1, 1, 0, 1], np.int64)
    return d


def main():
    if len(sys.argv) > 1:  # a checkout of the reference that is not installed
        sys.path.insert(0, sys.argv[1])
    import torch
    import linear_operator.operators as ops
    from linear_operator.operators import DenseLinearOperator, DiagLinearOperator

    torch.set_default_dtype(torch.float32)
    torch.set_num_threads(1)  # (bitwise reproducible CPU reductions)
    x = block_inputs()
    Tn = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    out = {}
    M, M4, K, K2 = Tn(x["M"]), Tn(x["M4"]), Tn(x["K"]), Tn(x["K2"])
    for k, name in KINDS:
        cls = getattr(ops, name)
        A = cls(DenseLinearOperator(M))
        out[k + "_shape"] = np.array(A.shape)
        out[k + "_dense"] = A.to_dense()
        r1, r3 = Tn(x[k + "_rhs1"]), Tn(x[k + "_rhs3"])
        out[k + "_y1"], out[k + "_y3"] = A @ r1, A @ r3
        out[k + "_yT3"] = A.mT @ r3
        out[k + "_yvec"] = A[0] @ r1[0, :, 0]
        out[k + "_diag"] = A.diagonal()
        pre = "sb" if k == "sb" else "ix"
        out[k + "_vals"] = A[Tn(x[pre + "_batch"]), Tn(x[pre + "_rows"]), Tn(x[pre + "_cols"])]
        sub = A[1]
        out[k + "_b1_cls"] = np.array(type(sub).__name__)
        out[k + "_b1_dense"] = sub.to_dense()
        out[k + "_slice"] = A[:, 4:10, 7:12].to_dense()  # (bounds that are no multiples of T: the plain sub-matrix)
        out[k + "_row5"] = A[0, 5]
        out[k + "_dim0_dense"] = cls(DenseLinearOperator(M4), block_dim=0).to_dense()
        out[k + "_dimm3_dense"] = cls(DenseLinearOperator(M), block_dim=-3).to_dense()
        S = A * Tn(x["c"])
        out[k + "_cm_cls"] = np.array(f"{type(S).__name__}/{type(S.base_linear_op).__name__}")
        out[k + "_cm_dense"] = S.to_dense()
        Mg = M.clone().requires_grad_(True)
        (cls(DenseLinearOperator(Mg)) @ r3).sum().backward()
        out[k + "_dM"] = Mg.grad
    D = ops.BlockDiagLinearOperator(DiagLinearOperator(Tn(x["dg"])))
    out["bd_diagbase_cls"] = np.array(type(D).__name__)
    out["bd_diagbase_dense"] = D.to_dense()
    P = ops.BlockDiagLinearOperator(DenseLinearOperator(M)) @ ops.BlockDiagLinearOperator(DenseLinearOperator(K2))
    out["bd_mm_cls"] = np.array(type(P).__name__)
    out["bd_mm_dense"] = P.to_dense()
    P = ops.BlockDiagLinearOperator(DenseLinearOperator(M)) @ DiagLinearOperator(Tn(x["dg"]).reshape(G, T * N))
    out["bd_md_cls"] = np.array(type(P).__name__)
    out["bd_md_dense"] = P.to_dense()
    # sum over a batch dimension, the rows, the columns, everything
    A = DenseLinearOperator(M)
    S3, S0 = A.sum(-3), DenseLinearOperator(M4).sum(0)
    out["sum_m3_cls"], out["sum_m3_dense"] = np.array(type(S3).__name__), S3.to_dense()
    out["sum_0_cls"], out["sum_0_dense"] = np.array(type(S0).__name__), S0.to_dense()
    SR = ops.RootLinearOperator(Tn(x["R"])).sum(-3)  # (a dense operator sums its tensor; a structured one stays lazy)
    out["sum_root_cls"], out["sum_root_dense"] = np.array(type(SR).__name__), SR.to_dense()
    out["sum_m1"], out["sum_m2"], out["sum_all"] = A.sum(-1), A.sum(-2), A.sum()
    # exact solves and log-determinants (N = 36 <= max_cholesky_size), gradients with respect to the blocks
    for k, name in KINDS[:2]:
        cls = getattr(ops, name)
        r3 = Tn(x[k + "_rhs3"])
        out[k + "_solve"] = cls(DenseLinearOperator(K)).solve(r3)
        Kg = K.clone().requires_grad_(True)
        iq, ld = cls(DenseLinearOperator(Kg)).inv_quad_logdet(r3, logdet=True)
        (iq.sum() + ld.sum()).backward()
        out[k + "_iq"], out[k + "_ld"], out[k + "_dK"] = iq, ld, Kg.grad
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    groups = {"g32_block_diag": ("bd_",), "g32_block_interleaved": ("bi_",), "g32_block_sum": ("sb_", "sum_")}
    for name, pre in groups.items():
        sel = {k: v for k, v in out.items() if k.startswith(pre)}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **sel)
        print(name, sorted(sel))


if __name__ == "__main__":
    main()
