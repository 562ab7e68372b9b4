#!/usr/bin/env python3
"""Generate the golden vectors tests/golden/g31_chol_*.npz of the exact small-N path by running the REAL reference:
psd_safe_cholesky, CholLinearOperator(...).solve / .inv_quad_logdet / .inverse().to_dense() for a lower and an upper
factor, and the reference's autograd gradients of solve(...).sum() and of inv_quad + logdet with respect to the dense
matrix (N = 40 and N = 300, batch 2).

Runs only where the reference is importable (like make_golden_mul.py); only the .npz outputs are committed.  Inputs come
from chol_inputs() below (numpy PCG64, seeded), which the tests import.
Usage:  python tests/golden/make_golden_chol.py [path of the reference checkout]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (40, 300)


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def chol_inputs():
    """Every input of the fixtures, by name: A = X X^T + 0.5 I with X [2, N, 24] (the family of the device tests), right-
    hand sides of one and of three columns."""
    d = {}
    for n in SIZES:
        X = rng(3100 + n).standard_normal((2, n, 24)).astype(np.float32)
        d[f"A{n}"] = (X @ np.swapaxes(X, -1, -2) + 0.5 * np.eye(n, dtype=np.float32)).astype(np.float32)
        d[f"rhs{n}"] = rng(3200 + n).standard_normal((2, n, 3)).astype(np.float32)
        d[f"col{n}"] = rng(3300 + n).standard_normal((2, n, 1)).astype(np.float32)
        # the entries (member, row, column) at which the large fixtures keep dense results (all of them at N = 40)
        r = rng(3400 + n)
        d[f"at{n}"] = np.stack([r.integers(0, 2, 4000), r.integers(0, n, 4000), r.integers(0, n, 4000)]).astype(np.int64)
    return d


def sample(dense, at, n):
    """The fixture's view of a dense [2, N, N] result: whole at N = 40, the entries `at` beyond."""
    return dense if n <= 64 else dense[at[0], at[1], at[2]]




def main():
    if len(sys.argv) > 1:
        sys.path.insert(0, sys.argv[1])
    import torch
    from linear_operator import to_linear_operator
    from linear_operator.operators import CholLinearOperator, TriangularLinearOperator
    from linear_operator.utils.cholesky import psd_safe_cholesky

    torch.set_num_threads(1)
    inp = chol_inputs()
    for n in SIZES:
        out = {}
        for dtype, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            A = torch.from_numpy(inp[f"A{n}"]).to(dtype)
            rhs = torch.from_numpy(inp[f"rhs{n}"]).to(dtype)
            col = torch.from_numpy(inp[f"col{n}"]).to(dtype)
            L = psd_safe_cholesky(A)
            out[f"L_{tag}"] = sample(L.numpy(), inp[f"at{n}"], n)
            for upper, F in ((False, L), (True, L.mT.contiguous())):
                o = "up" if upper else "lo"
                C = CholLinearOperator(TriangularLinearOperator(F, upper=upper), upper=upper)
                out[f"solve_{o}_{tag}"] = C.solve(rhs).numpy()
                out[f"solve1_{o}_{tag}"] = C.solve(col).numpy()
                iq, ld = C.inv_quad_logdet(rhs, logdet=True)
                out[f"iq_{o}_{tag}"], out[f"ld_{o}_{tag}"] = iq.numpy(), ld.numpy()
                out[f"iqcols_{o}_{tag}"] = C.inv_quad_logdet(rhs, logdet=False, reduce_inv_quad=False)[0].numpy()
                out[f"inv_{o}_{tag}"] = sample(C.inverse().to_dense().numpy(), inp[f"at{n}"], n)
            Ag = A.clone().requires_grad_(True)
            to_linear_operator(Ag).solve(rhs).sum().backward()
            out[f"grad_solve_{tag}"] = sample(Ag.grad.numpy(), inp[f"at{n}"], n)
            Ag = A.clone().requires_grad_(True)
            iq, ld = to_linear_operator(Ag).inv_quad_logdet(rhs, logdet=True)
            (iq + ld).sum().backward()
            out[f"grad_iql_{tag}"] = sample(Ag.grad.numpy(), inp[f"at{n}"], n)
        np.savez_compressed(os.path.join(HERE, f"g31_chol_n{n}.npz"), **out)
        print(f"g31_chol_n{n}.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
