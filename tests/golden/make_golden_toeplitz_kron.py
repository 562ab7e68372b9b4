#!/usr/bin/env python3
"""Generate tests/golden/g36_toeplitz_kron.npz by running the REAL reference: a KroneckerProductLinearOperator of 2 or 3
ToeplitzLinearOperators on its own (the covariance of a GP on a regular grid), bare and under an AddedDiagLinearOperator.

Runs only where the reference is importable; only the .npz output is committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_toeplitz_kron.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_ski import column, rng  # noqa: E402
from make_golden_ski_grid import PC_GAP, PC_RANK, kron_dense64  # noqa: E402

PC_TIE = 1e-12  # a gap below this in fp64 is an exact tie of the Toeplitz structure, not a near-tie (see pivot_gaps64)
CASES = {"g2": ((12, 16), 1), "g2b3": ((12, 16), 3), "g3": ((6, 5, 7), 1)}


def pivot_gaps64(cols, rank):
    """The reference's pivoted Cholesky of T_1 (x) .. (x) T_D for one member in fp64: (pivots, the relative gap between
    the two largest remaining diagonal entries at every step).  The diagonal of this matrix is constant and the matrix
    is persymmetric, so some steps have candidates that tie EXACTLY (gap 0 up to fp64 rounding): the first step always.
    Such a tie is decided by the order of the fp32 operations, which the pivoted-Cholesky kernels restate one by one;
    what the fixture must exclude are near-ties, gaps between PC_TIE and PC_GAP."""
    A = kron_dense64(cols)
    N = A.shape[0]
    diag = np.diag(A).copy()
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


def inputs():
    """Every input of the fixture, by name (the tests call this too)."""
    d = {}
    for p, (grid, B) in CASES.items():
        N = int(np.prod(grid))
        for k, m in enumerate(grid):
            # (members differ in more than scale: every member has a length scale of its own)
            d[f"{p}_c{k + 1}"] = np.concatenate(
                [column(3700 + 10 * len(p) + k + 100 * b, 1, m, ls=(0.35 + 0.1 * k) * (1.0 + 0.2 * b)) for b in range(B)])
        seed = 3730 + 7 * B + len(grid)
        d[p + "_rhs1"] = rng(seed).standard_normal((B, N, 1)).astype(np.float32)
        d[p + "_rhs5"] = rng(seed + 1).standard_normal((B, N, 5)).astype(np.float32)
        d[p + "_u"] = rng(seed + 2).standard_normal((B, N, 4)).astype(np.float32)
        d[p + "_v"] = rng(seed + 3).standard_normal((B, N, 4)).astype(np.float32)
        d[p + "_d"] = (0.5 + 0.5 * rng(seed + 4).random((B, N))).astype(np.float32)
        d[p + "_rhs"] = rng(seed + 5).standard_normal((B, N, 2)).astype(np.float32)
    d["g2_Z"] = rng(3790).standard_normal((1, 192, 6)).astype(np.float32)
    # pivoted Cholesky: long length scales, no near-tie at any pivot step (main() asserts it)
    d["pc_c1"], d["pc_c2"] = column(3795, 1, 12, ls=0.8), column(3796, 1, 16, ls=1.1)
    return d


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.functions import pivoted_cholesky
    from linear_operator.operators import (AddedDiagLinearOperator, DiagLinearOperator, KroneckerProductLinearOperator,
                                           ToeplitzLinearOperator)

    torch.set_default_dtype(torch.float32)
    x = inputs()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    out = {}

    def kron(p, cols=None):
        D = len(CASES[p][0]) if p in CASES else 2
        cols = [T(x[f"{p}_c{k + 1}"]) for k in range(D)] if cols is None else cols
        return KroneckerProductLinearOperator(*[ToeplitzLinearOperator(c) for c in cols])

    for p, (grid, B) in CASES.items():
        A = kron(p)
        out[p + "_mm1"], out[p + "_mm5"] = A._matmul(T(x[p + "_rhs1"])), A._matmul(T(x[p + "_rhs5"]))
        # column gradients: autograd of the reference's _matmul (what its _bilinear_derivative does)
        cols = [T(x[f"{p}_c{k + 1}"]).clone().requires_grad_(True) for k in range(len(grid))]
        (T(x[p + "_u"]) * kron(p, cols)._matmul(T(x[p + "_v"]))).sum().backward()
        for k, c in enumerate(cols):
            out[f"{p}_g{k + 1}"] = c.grad
        with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.max_cholesky_size(0), \
                settings.min_preconditioning_size(100):
            out[p + "_solve"] = AddedDiagLinearOperator(A, DiagLinearOperator(T(x[p + "_d"]))).solve(T(x[p + "_rhs"]))
    # pivoted Cholesky: fp32 rounding must not be able to flip a pivot between near-tied candidates
    piv64, gaps = pivot_gaps64([x["pc_c1"][0], x["pc_c2"][0]], PC_RANK)
    assert all(g >= PC_GAP or g <= PC_TIE for g in gaps), f"pivot candidates closer than {PC_GAP}: {gaps}"
    L, piv = pivoted_cholesky(kron("pc"), PC_RANK, error_tol=1e-6, return_pivots=True)
    out["pc_L"], out["pc_piv"], out["pc_gaps"] = L, piv, gaps
    # inv_quad_logdet with gradients on every column and on d (probes fixed)
    Z = T(x["g2_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6), \
            settings.max_cholesky_size(0), settings.min_preconditioning_size(100):
        dd, c1, c2 = (T(x[k]).clone().requires_grad_(True) for k in ("g2_d", "g2_c1", "g2_c2"))
        A = Probed(kron("g2", [c1, c2]), DiagLinearOperator(dd))
        iq, ld = A.inv_quad_logdet(T(x["g2_rhs"]), logdet=True)
        (iq.sum() + ld.sum()).backward()
        out["iql_iq"], out["iql_ld"] = iq, ld
        out["iql_dd"], out["iql_dc1"], out["iql_dc2"] = dd.grad, c1.grad, c2.grad
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "g36_toeplitz_kron.npz"), **out)
    print("g36_toeplitz_kron", sorted(out))


if __name__ == "__main__":
    main()
