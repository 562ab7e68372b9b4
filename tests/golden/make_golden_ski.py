#!/usr/bin/env python3
"""Generate the SKI golden vectors tests/golden/g29_ski_*.npz by running the REAL reference
(ToeplitzLinearOperator, InterpolatedLinearOperator, utils/toeplitz.py, utils/interpolation.py).

Runs only where the reference is importable (like make_golden.py, which stays as it is); only the .npz outputs are
committed.  Inputs come from ski_inputs() below (numpy PCG64, seeded): the tests rebuild them from the same function.
Usage:  python tests/golden/make_golden_ski.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def column(seed, B, M, ls=0.1):
    """An RBF kernel column on a regular grid of M points in [0, 1] (symmetric positive definite Toeplitz)."""
    g = np.linspace(0.0, 1.0, M)
    t = np.exp(-0.5 * ((g - g[0]) / ls) ** 2)
    scale = 1.0 + 0.5 * rng(seed).random((B, 1))
    return (scale * t[None, :]).astype(np.float32)


def interp(seed, B, N, M, J, cubic=False):
    """(idx int64, vals fp32) [B, N, J]: J consecutive grid points per row; random positive weights (no near-ties in the
    approximate diagonal) or cubic-convolution weights that sum to 1."""
    r = rng(seed)
    x = r.random((B, N)) * (M - J - 1)
    base = np.floor(x).astype(np.int64)
    idx = base[..., None] + np.arange(J)[None, None, :]
    if cubic:
        s = (x - base)[..., None] + 1.0 - np.arange(J)[None, None, :]  # distances to the J points
        a = -0.75
        s = np.abs(s)
        w = np.where(s <= 1, (a + 2) * s ** 3 - (a + 3) * s ** 2 + 1,
                     np.where(s < 2, a * s ** 3 - 5 * a * s ** 2 + 8 * a * s - 4 * a, 0.0))
        vals = w.astype(np.float32)
    else:
        vals = (0.2 + r.random((B, N, J))).astype(np.float32) / J
    return idx, vals


def ski_inputs():
    """Every input of the fixtures, by name (the tests call this too)."""
    d = {}
    d["tz_col"] = column(2901, 3, 37)
    d["tz_rhs"] = rng(2902).standard_normal((3, 37, 5)).astype(np.float32)
    d["tz_u"] = rng(2903).standard_normal((2, 3, 37, 4)).astype(np.float32)  # broadcast batch over the column's
    d["tz_v"] = rng(2904).standard_normal((2, 3, 37, 4)).astype(np.float32)
    for J in (4, 16):
        d[f"sq{J}_col"] = column(2910 + J, 2, 64)
        d[f"sq{J}_li"], d[f"sq{J}_lv"] = interp(2920 + J, 2, 100, 64, J)
        d[f"sq{J}_ri"], d[f"sq{J}_rv"] = interp(2930 + J, 2, 100, 64, J)
        d[f"sq{J}_rhs"] = rng(2940 + J).standard_normal((2, 100, 3)).astype(np.float32)
    d["re_col"] = column(2950, 2, 64)
    d["re_li"], d["re_lv"] = interp(2951, 2, 70, 64, 4)
    d["re_ri"], d["re_rv"] = interp(2952, 2, 100, 64, 4)
    d["re_rhs"] = rng(2953).standard_normal((2, 100, 3)).astype(np.float32)
    d["re_lhs"] = rng(2954).standard_normal((2, 70, 3)).astype(np.float32)
    d["pc_col"] = column(2960, 2, 128, ls=0.05)
    d["pc_li"], d["pc_lv"] = interp(2961, 2, 300, 128, 4)
    d["big_col"] = column(2970, 2, 256, ls=0.05)
    d["big_li"], d["big_lv"] = interp(2971, 2, 2048, 256, 4)
    d["big_d"] = (0.05 + 0.1 * rng(2972).random((2, 2048))).astype(np.float32)
    d["big_rhs"] = rng(2973).standard_normal((2, 2048, 2)).astype(np.float32)
    d["big_Z"] = rng(2974).standard_normal((2, 2048, 6)).astype(np.float32)
    d["k2_c1"] = column(2980, 1, 16)[0]
    d["k2_c2"] = column(2981, 1, 12)[0]
    d["k2_li"], d["k2_lv"] = interp(2982, 1, 300, 16 * 12, 16)
    d["k2_rhs"] = rng(2983).standard_normal((1, 300, 2)).astype(np.float32)
    d["k2_d"] = np.full((1, 300), 0.1, np.float32)
    return d


def main():
    sys.path.insert(0, "/root/reference")
    import torch
    from linear_operator import settings
    from linear_operator.operators import (AddedDiagLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
                                           KroneckerProductLinearOperator, ToeplitzLinearOperator)
    from linear_operator.functions import pivoted_cholesky

    torch.set_default_dtype(torch.float32)
    x = ski_inputs()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    out = {}
    # Toeplitz
    tz = ToeplitzLinearOperator(T(x["tz_col"]))
    out["tz_matmul"] = tz._matmul(T(x["tz_rhs"]))
    out["tz_diag"] = tz._diagonal()
    out["tz_dense"] = tz.to_dense()
    out["tz_bil"] = tz._bilinear_derivative(T(x["tz_u"]), T(x["tz_v"]))[0]
    # Interpolated, square (J = 4, 16) and rectangular
    rows = torch.tensor([0, 5, 99, 42]), torch.tensor([3, 5, 0, 77])
    for J in (4, 16):
        p = f"sq{J}"
        A = InterpolatedLinearOperator(ToeplitzLinearOperator(T(x[p + "_col"])), T(x[p + "_li"]), T(x[p + "_lv"]),
                                       T(x[p + "_ri"]), T(x[p + "_rv"]))
        out[p + "_matmul"] = A._matmul(T(x[p + "_rhs"]))
        out[p + "_tmatmul"] = A._t_matmul(T(x[p + "_rhs"]))
        out[p + "_approx_diag"] = A._approx_diagonal()
        out[p + "_diag"] = torch.stack([A._get_indices(torch.arange(100), torch.arange(100), torch.tensor(b))
                                        for b in range(2)])
        out[p + "_getidx"] = A._get_indices(rows[0], rows[1], torch.tensor([0, 1, 1, 0]))
        out[p + "_mm"] = A.matmul(T(x[p + "_rhs"]))
    A = InterpolatedLinearOperator(ToeplitzLinearOperator(T(x["re_col"])), T(x["re_li"]), T(x["re_lv"]),
                                   T(x["re_ri"]), T(x["re_rv"]))
    out["re_matmul"] = A._matmul(T(x["re_rhs"]))
    out["re_tmatmul"] = A._t_matmul(T(x["re_lhs"]))
    out["re_mm"] = A.matmul(T(x["re_rhs"]))
    bil = A._bilinear_derivative(T(x["re_lhs"]), T(x["re_rhs"]))
    out["re_bil_col"], out["re_bil_lv"], out["re_bil_rv"] = bil[0], bil[2], bil[4]
    # pivoted Cholesky of Interpolated(Toeplitz), shared left / right
    A = InterpolatedLinearOperator(ToeplitzLinearOperator(T(x["pc_col"])), T(x["pc_li"]), T(x["pc_lv"]),
                                   T(x["pc_li"]), T(x["pc_lv"]))
    L, piv = pivoted_cholesky(A, 10, error_tol=1e-6, return_pivots=True)
    out["pc_L"], out["pc_piv"] = L, piv
    # AddedDiag(Interpolated(Toeplitz), Diag) at N = 2048 (preconditioned): solve, inv_quad_logdet, gradients
    Z = T(x["big_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6):
        col, dd, lv = T(x["big_col"]), T(x["big_d"]), T(x["big_lv"])
        A = AddedDiagLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), T(x["big_li"]), lv,
                                                               T(x["big_li"]), lv), DiagLinearOperator(dd))
        out["big_solve"] = A.solve(T(x["big_rhs"]))
        colg, ddg, lvl, lvr = (t.clone().requires_grad_(True) for t in (col, dd, lv, lv))
        A = Probed(InterpolatedLinearOperator(ToeplitzLinearOperator(colg), T(x["big_li"]), lvl, T(x["big_li"]), lvr),
                   DiagLinearOperator(ddg))
        iq, ld = A.inv_quad_logdet(T(x["big_rhs"]), logdet=True)
        (iq.sum() + ld.sum()).backward()
        out["big_iq"], out["big_ld"] = iq, ld
        out["big_dcol"], out["big_dd"], out["big_dlv"], out["big_drv"] = colg.grad, ddg.grad, lvl.grad, lvr.grad
    # 2-D grid: Kronecker(Toeplitz, Toeplitz) base, forward only
    base = KroneckerProductLinearOperator(ToeplitzLinearOperator(T(x["k2_c1"])), ToeplitzLinearOperator(T(x["k2_c2"])))
    A2 = InterpolatedLinearOperator(base.expand(1, 192, 192) if hasattr(base, "expand") else base,
                                    T(x["k2_li"]), T(x["k2_lv"]), T(x["k2_li"]), T(x["k2_lv"]))
    out["k2_matmul"] = A2._matmul(T(x["k2_rhs"]))
    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400):
        out["k2_solve"] = AddedDiagLinearOperator(A2, DiagLinearOperator(T(x["k2_d"]))).solve(T(x["k2_rhs"]))
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    groups = {"g29_ski_toeplitz": "tz_", "g29_ski_interp": ("sq", "re_"), "g29_ski_pivchol": "pc_",
              "g29_ski_solve": "big_", "g29_ski_kron2d": "k2_"}
    for name, pre in groups.items():
        pre = pre if isinstance(pre, tuple) else (pre,)
        sel = {k: v for k, v in out.items() if k.startswith(pre)}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **sel)
        print(name, sorted(sel))


if __name__ == "__main__":
    main()
