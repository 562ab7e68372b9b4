#!/usr/bin/env python3
"""Generate the golden vectors tests/golden/g33_masked_*.npz of MaskedLinearOperator by running the REAL reference in
fp64 on the CPU.

Runs only where the reference is importable (like make_golden_block.py); only the .npz outputs are committed.  Inputs
come from masked_inputs() below (numpy PCG64, seeded); the tests call it and build the same operators from this package.
Every case has batch 2, one 70 % mask for rows and columns (`mask`) and a second, different column mask (`cmask`) for
the non-square products.  The members are well conditioned (eigenvalues within about 1e2 of each other): the reference's
CG (max_cholesky_size 0, cg_tolerance CG_TOL) stops well below max_cg_iterations, which is asserted here.  Each CG
result is recorded next to its own error against the fp64 dense solve (`*_referr`).
Usage:  python tests/golden/make_golden_masked.py [path of the reference checkout]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B = 2
CG_TOL = 1e-5
CASES = ("dense", "kron", "lowrank")


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def spd(seed, n):
    a = rng(seed).standard_normal((B, n, n))
    return (a @ a.swapaxes(-1, -2) / n + np.eye(n)).astype(np.float32)


def masked_inputs(case):
    """The tensors of one case by name (float32 values; the CPU tests use them in fp64), its masks and vectors."""
    d = {}
    if case == "dense":  # Masked(Dense(K) + Diag(D)), 40 x 40
        n, seed = 40, 3300
        d["K"] = spd(seed + 1, n)
        d["D"] = (0.5 + rng(seed + 2).random((B, n))).astype(np.float32)
    elif case == "kron":  # Masked(Kron(K1, K2) + 0.3 I), 12 (x) 5
        n, seed = 60, 3310
        d["K1"], d["K2"] = spd(seed + 1, 12), spd(seed + 2, 5)
        d["sigma2"] = np.full((B, 1), 0.3, np.float32)
    else:  # Masked(LowRankRoot(C) + Diag(D)), 60 x 4
        n, seed = 60, 3320
        d["C"] = (0.5 * rng(seed + 1).standard_normal((B, n, 4))).astype(np.float32)
        d["D"] = (0.5 + rng(seed + 2).random((B, n))).astype(np.float32)
    mask = rng(seed + 3).random(n) < 0.7
    cmask = rng(seed + 4).random(n) < 0.6
    mask[0], cmask[0] = True, False  # (the two masks differ)
    m, mc = int(mask.sum()), int(cmask.sum())
    d["mask"], d["cmask"] = mask, cmask
    d["rhs"] = rng(seed + 5).standard_normal((B, m, 3)).astype(np.float32)
    d["rhs_c"] = rng(seed + 6).standard_normal((B, mc, 2)).astype(np.float32)  # for the [m, mc] operator
    d["rhs_t"] = rng(seed + 7).standard_normal((B, m, 2)).astype(np.float32)  # for its transpose
    d["ix_rows"] = np.array([0, m - 1, 3, 5, 2], np.int64)
    d["ix_cols"] = np.array([1, 0, mc - 1, 5, 2], np.int64)
    d["ix_batch"] = np.array([0, 1, 1, 0, 1], np.int64)
    return d


GRAD_NAMES = {"dense": ("K", "D"), "kron": ("K1", "K2", "sigma2"), "lowrank": ("C", "D")}


def build_base(ops, case, t):
    """The base operator of a case from its tensors, with the classes of `ops` (the reference's or this package's)."""
    if case == "dense":
        return ops.DenseLinearOperator(t["K"]) + ops.DiagLinearOperator(t["D"])
    if case == "kron":
        kp = ops.KroneckerProductLinearOperator(ops.DenseLinearOperator(t["K1"]), ops.DenseLinearOperator(t["K2"]))
        return kp + ops.ConstantDiagLinearOperator(t["sigma2"], diag_shape=kp.size(-1))
    return ops.LowRankRootLinearOperator(t["C"]) + ops.DiagLinearOperator(t["D"])


def dense64(case, t):
    """The base matrix in fp64 from torch tensors, differentiable."""
    import torch

    if case == "dense":
        return t["K"] + torch.diag_embed(t["D"])
    if case == "kron":
        kp = torch.einsum("bij,bkl->bikjl", t["K1"], t["K2"]).reshape(B, 60, 60)
        return kp + t["sigma2"].unsqueeze(-1) * torch.eye(60, dtype=kp.dtype)
    return t["C"] @ t["C"].mT + torch.diag_embed(t["D"])


def main():
    if len(sys.argv) > 1:  # a checkout of the reference that is not installed
        sys.path.insert(0, sys.argv[1])
    import torch
    import linear_operator
    import linear_operator.operators as ops
    from linear_operator import settings

    torch.set_default_dtype(torch.float64)
    torch.set_num_threads(1)  # (bitwise reproducible CPU reductions)
    for case in CASES:
        x = masked_inputs(case)
        names = GRAD_NAMES[case]
        leaf = lambda: {k: torch.from_numpy(x[k]).double().requires_grad_(True) for k in names}  # noqa: E731
        mask, cmask = torch.from_numpy(x["mask"]), torch.from_numpy(x["cmask"])
        rhs, rhs_c, rhs_t = (torch.from_numpy(x[k]).double() for k in ("rhs", "rhs_c", "rhs_t"))
        out = {"cg_tol": np.array(CG_TOL)}
        with torch.no_grad():
            t = {k: v.detach() for k, v in leaf().items()}
            A = ops.MaskedLinearOperator(build_base(ops, case, t), mask, mask)
            R = ops.MaskedLinearOperator(build_base(ops, case, t), mask, cmask)
            out["shape"], out["shape_rc"] = np.array(A.shape), np.array(R.shape)
            out["dense"], out["dense_rc"] = A.to_dense(), R.to_dense()
            out["matmul"], out["matmul_rc"] = A.matmul(rhs), R.matmul(rhs_c)
            out["t_matmul_rc"] = R._t_matmul(rhs_t)
            out["diag"] = A.diagonal()
            out["indices_rc"] = R._get_indices(*(torch.from_numpy(x[k]) for k in ("ix_rows", "ix_cols", "ix_batch")))
            exact = torch.linalg.solve(out["dense"], rhs)
            out["solve_exact"] = exact
            with settings.max_cholesky_size(0), settings.cg_tolerance(CG_TOL), settings.max_cg_iterations(200):
                solve = A.solve(rhs)  # the reference's own CG
            out["solve"] = solve
            out["solve_referr"] = np.array(float((solve - exact).abs().max() / exact.abs().max()))
            resid = (out["dense"] @ solve - rhs).norm(dim=-2) / rhs.norm(dim=-2)
            assert float(resid.max()) < 10 * CG_TOL, f"{case}: the reference's CG did not converge ({float(resid.max())})"
        # inv_quad and its gradients: the reference through CG, and exactly from the dense matrix
        t = leaf()
        A = ops.MaskedLinearOperator(build_base(ops, case, t), mask, mask)
        with settings.max_cholesky_size(0), settings.cg_tolerance(CG_TOL), settings.max_cg_iterations(200):
            iq = A.inv_quad(rhs)
        iq.sum().backward()
        te = leaf()
        Kd = dense64(case, te)[..., mask, :][..., :, mask]
        iq_exact = (rhs * torch.linalg.solve(Kd, rhs)).sum((-2, -1))
        iq_exact.sum().backward()
        out["inv_quad"], out["inv_quad_exact"] = iq.detach(), iq_exact.detach()
        out["inv_quad_referr"] = np.array(float(((iq - iq_exact).abs() / iq_exact.abs()).max().detach()))
        for k in names:
            g, ge = t[k].grad, te[k].grad
            out["grad_" + k], out["grad_" + k + "_exact"] = g, ge
            out["grad_" + k + "_referr"] = np.array(float((g - ge).abs().max() / ge.abs().max()))
        out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
        path = os.path.join(HERE, f"g33_masked_{case}.npz")
        np.savez_compressed(path, **out)
        print(case, {k: float(v) for k, v in out.items() if k.endswith("referr")}, os.path.getsize(path), "bytes")
    print("reference", linear_operator.__version__)


if __name__ == "__main__":
    main()
