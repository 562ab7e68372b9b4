#!/usr/bin/env python3
"""Generate tests/golden/g35_ski_grid.npz by running the REAL reference: InterpolatedLinearOperator over a
KroneckerProductLinearOperator of 2 or 3 ToeplitzLinearOperators (SKI on a 2-D / 3-D grid).

Runs only where the reference is importable; only the .npz output is committed.  Inputs come from grid_inputs() below
(numpy PCG64, seeded; no reference needed): the tests rebuild them from the same function.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_ski_grid.py
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_ski import column, rng  # noqa: E402

PC_RANK = 10
PC_GAP = 1e-3  # relative gap between the largest and the second largest remaining diagonal at every pivot step


def grid_interp(seed, B, N, grid, pts=4):
    """(idx int64, vals fp32) [B, N, pts^D]: per axis `pts` consecutive grid points, the grid index of a combination
    g = (g_1 M_2 + g_2) M_3 + g_3 (the reference's Kronecker ordering); random positive weights, the product of per-axis
    weights times a random factor (no near-ties in the approximate diagonal)."""
    r = rng(seed)
    D = len(grid)
    base = [np.floor(r.random((B, N)) * (m - pts + 1)).astype(np.int64) for m in grid]
    w_ax = [0.2 + r.random((B, N, pts)) for _ in grid]
    J = pts ** D
    idx = np.zeros((B, N, J), np.int64)
    vals = np.ones((B, N, J))
    for j, offs in enumerate(itertools.product(range(pts), repeat=D)):
        g = np.zeros((B, N), np.int64)
        for k, o in enumerate(offs):
            g = g * grid[k] + base[k] + o
            vals[..., j] *= w_ax[k][..., o]
        idx[..., j] = g
    vals *= 0.5 + r.random((B, N, J))
    return idx, (vals / vals.sum(-1, keepdims=True).mean()).astype(np.float32)


def kron_dense64(cols):
    """T_1 (x) .. (x) T_D in fp64 from the first columns [M_k] (one member)."""
    K = np.ones((1, 1))
    for t in cols:
        M = t.shape[-1]
        T = t.astype(np.float64)[np.abs(np.arange(M)[:, None] - np.arange(M)[None, :])]
        K = np.kron(K, T)
    return K


def w_dense64(idx, vals, M):
    """One member's W [N, M] in fp64."""
    N, J = idx.shape
    W = np.zeros((N, M))
    np.add.at(W, (np.repeat(np.arange(N), J), idx.reshape(-1)), vals.astype(np.float64).reshape(-1))
    return W


def pivot_gaps64(cols, idx, vals, rank):
    """The reference's pivoted Cholesky (functions/_pivoted_cholesky.py:14-105: approximate diagonal first, then the
    downdated one) of W K W^T for one member in fp64: (pivots, the relative gap between the two largest remaining
    diagonal entries at every step)."""
    M = int(np.prod([t.shape[-1] for t in cols]))
    W = w_dense64(idx, vals, M)
    A = W @ kron_dense64(cols) @ W.T
    t0 = np.prod([float(t[0]) for t in cols])
    diag = t0 * W.sum(-1) ** 2  # _approx_diagonal of a constant base diagonal, W_l = W_r
    N = A.shape[0]
    perm = np.arange(N)
    L = np.zeros((rank, N))
    gaps = []
    for m in range(rank):
        rem = np.sort(diag[perm[m:]])[::-1]
        gaps.append((rem[0] - rem[1]) / rem[0])
        j = m + int(np.argmax(diag[perm[m:]]))
        perm[[m, j]] = perm[[j, m]]
        pi = perm[m]
        L[m, pi] = np.sqrt(diag[pi])
        rest = perm[m + 1:]
        row = (A[pi, rest] - L[:m, pi] @ L[:m, rest]) / L[m, pi]
        L[m, rest] = row
        diag[rest] -= row ** 2
    return perm[:rank], np.array(gaps)


def grid_inputs():
    """Every input of the fixture, by name (the tests call this too)."""
    d = {}
    g2 = (12, 16)
    d["g2_c1"], d["g2_c2"] = column(3501, 1, 12, ls=0.3)[0], column(3502, 1, 16, ls=0.3)[0]
    for B in (1, 3):  # unbatched base under interpolation matrices of batch 1 and 3
        p = f"g2b{B}"
        d[p + "_li"], d[p + "_lv"] = grid_interp(3510 + B, B, 192, g2)
        d[p + "_rhs1"] = rng(3520 + B).standard_normal((B, 192, 1)).astype(np.float32)
        d[p + "_rhs5"] = rng(3530 + B).standard_normal((B, 192, 5)).astype(np.float32)
        d[p + "_d"] = (0.5 + 0.5 * rng(3540 + B).random((B, 192))).astype(np.float32)
        d[p + "_rhs"] = rng(3550 + B).standard_normal((B, 192, 2)).astype(np.float32)
    d["g2b1_Z"] = rng(3560).standard_normal((1, 192, 6)).astype(np.float32)
    g3 = (6, 5, 7)
    d["g3_c1"], d["g3_c2"], d["g3_c3"] = (column(3570 + k, 1, m, ls=0.4)[0] for k, m in enumerate(g3))
    d["g3_li"], d["g3_lv"] = grid_interp(3575, 1, 150, g3)
    d["g3_rhs1"] = rng(3576).standard_normal((1, 150, 1)).astype(np.float32)
    d["g3_rhs5"] = rng(3577).standard_normal((1, 150, 5)).astype(np.float32)
    # separate left and right interpolation matrices, square
    d["lr_li"], d["lr_lv"] = grid_interp(3580, 1, 192, g2)
    d["lr_ri"], d["lr_rv"] = grid_interp(3581, 1, 192, g2)
    d["lr_rhs1"] = rng(3582).standard_normal((1, 192, 1)).astype(np.float32)
    d["lr_rhs5"] = rng(3583).standard_normal((1, 192, 5)).astype(np.float32)
    # pivoted Cholesky: a seed at which no two candidates of a pivot step are closer than PC_GAP (main() asserts it)
    d["pc_li"], d["pc_lv"] = grid_interp(3592, 1, 192, g2)
    return d


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.functions import pivoted_cholesky
    from linear_operator.operators import (AddedDiagLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
                                           KroneckerProductLinearOperator, ToeplitzLinearOperator)

    torch.set_default_dtype(torch.float32)
    x = grid_inputs()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    out = {}

    def base2():
        return KroneckerProductLinearOperator(ToeplitzLinearOperator(T(x["g2_c1"])), ToeplitzLinearOperator(T(x["g2_c2"])))

    for B in (1, 3):
        p = f"g2b{B}"
        A = InterpolatedLinearOperator(base2(), T(x[p + "_li"]), T(x[p + "_lv"]), T(x[p + "_li"]), T(x[p + "_lv"]))
        out[p + "_mm1"], out[p + "_mm5"] = A._matmul(T(x[p + "_rhs1"])), A._matmul(T(x[p + "_rhs5"]))
        with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.max_cholesky_size(0), \
                settings.min_preconditioning_size(100):
            out[p + "_solve"] = AddedDiagLinearOperator(A, DiagLinearOperator(T(x[p + "_d"]))).solve(T(x[p + "_rhs"]))
    base3 = KroneckerProductLinearOperator(*[ToeplitzLinearOperator(T(x[f"g3_c{k}"])) for k in (1, 2, 3)])
    A = InterpolatedLinearOperator(base3, T(x["g3_li"]), T(x["g3_lv"]), T(x["g3_li"]), T(x["g3_lv"]))
    out["g3_mm1"], out["g3_mm5"] = A._matmul(T(x["g3_rhs1"])), A._matmul(T(x["g3_rhs5"]))
    A = InterpolatedLinearOperator(base2(), T(x["lr_li"]), T(x["lr_lv"]), T(x["lr_ri"]), T(x["lr_rv"]))
    out["lr_mm1"], out["lr_mm5"] = A._matmul(T(x["lr_rhs1"])), A._matmul(T(x["lr_rhs5"]))
    # pivoted Cholesky: fp32 rounding must not be able to flip a pivot
    piv64, gaps = pivot_gaps64([x["g2_c1"], x["g2_c2"]], x["pc_li"][0], x["pc_lv"][0], PC_RANK)
    assert gaps.min() >= PC_GAP, f"pivot candidates closer than {PC_GAP}: {gaps}"
    A = InterpolatedLinearOperator(base2(), T(x["pc_li"]), T(x["pc_lv"]), T(x["pc_li"]), T(x["pc_lv"]))
    L, piv = pivoted_cholesky(A, PC_RANK, error_tol=1e-6, return_pivots=True)
    assert np.array_equal(piv[0, :PC_RANK].numpy(), piv64), (piv[0, :PC_RANK], piv64)
    out["pc_L"], out["pc_piv"] = L, piv
    # inv_quad_logdet with gradients (columns detached, probes fixed)
    Z = T(x["g2b1_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6), \
            settings.max_cholesky_size(0), settings.min_preconditioning_size(100):
        dd, lvl, lvr = (T(x[k]).clone().requires_grad_(True) for k in ("g2b1_d", "g2b1_lv", "g2b1_lv"))
        A = Probed(InterpolatedLinearOperator(base2(), T(x["g2b1_li"]), lvl, T(x["g2b1_li"]), lvr), DiagLinearOperator(dd))
        iq, ld = A.inv_quad_logdet(T(x["g2b1_rhs"]), logdet=True)
        (iq.sum() + ld.sum()).backward()
        out["iql_iq"], out["iql_ld"] = iq, ld
        out["iql_dd"], out["iql_dlv"], out["iql_drv"] = dd.grad, lvl.grad, lvr.grad
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "g35_ski_grid.npz"), **out)
    print("g35_ski_grid", sorted(out))


if __name__ == "__main__":
    main()
