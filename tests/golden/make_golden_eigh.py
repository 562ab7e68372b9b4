#!/usr/bin/env python3
"""Generate tests/golden/g44_eigh.npz by running the REAL reference: the eigenvalues of `LinearOperator.eigh()`,
`eigvalsh()` and `diagonalization(method="symeig")` for dense symmetric positive definite float64 matrices (N = 5, 40,
65, batch 3), and of `KroneckerProductLinearOperator.eigh()` / `eigvalsh()` for one pair 6 (x) 7 (in the reference's own,
unsorted, order).  Eigenvectors are not recorded (their signs are free); the tests check them through A Q = Q diag(l).

Runs only where the reference is importable (like make_golden_chol.py); only the .npz output is committed.  Inputs come
from eigh_inputs() below (numpy PCG64, seeded), which the tests import.
Usage:  python tests/golden/make_golden_eigh.py [path of the reference checkout]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (5, 40, 65)
KRON = (6, 7)


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def eigh_inputs():
    """Every input of the fixture, by name: A = X X^T / N + 0.1 I with X [3, N, N] float64, and the two Kronecker
    factors built the same way without a batch."""
    d = {}
    for n in SIZES:
        X = rng(4400 + n).standard_normal((3, n, n))
        d[f"A{n}"] = X @ np.swapaxes(X, -1, -2) / n + 0.1 * np.eye(n)
    for n in KRON:
        X = rng(4450 + n).standard_normal((n, n))
        d[f"K{n}"] = X @ X.T / n + 0.1 * np.eye(n)
    return d


def main():
    if len(sys.argv) > 1:
        sys.path.insert(0, sys.argv[1])
    import torch
    from linear_operator.operators import DenseLinearOperator, KroneckerProductLinearOperator

    torch.set_num_threads(1)
    inp = eigh_inputs()
    out = {}
    for n in SIZES:
        op = DenseLinearOperator(torch.from_numpy(inp[f"A{n}"]))
        out[f"eigh_evals{n}"] = op.eigh()[0].numpy()
        out[f"eigvalsh{n}"] = DenseLinearOperator(torch.from_numpy(inp[f"A{n}"])).eigvalsh().numpy()
        out[f"diag_symeig_evals{n}"] = DenseLinearOperator(torch.from_numpy(inp[f"A{n}"])).diagonalization(method="symeig")[0].numpy()
    kp = KroneckerProductLinearOperator(*(DenseLinearOperator(torch.from_numpy(inp[f"K{n}"])) for n in KRON))
    out["kron_eigh_evals"] = kp.eigh()[0].numpy()
    kp = KroneckerProductLinearOperator(*(DenseLinearOperator(torch.from_numpy(inp[f"K{n}"])) for n in KRON))
    out["kron_eigvalsh"] = kp.eigvalsh().numpy()
    np.savez_compressed(os.path.join(HERE, "g44_eigh.npz"), **out)
    print("g44_eigh.npz", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
