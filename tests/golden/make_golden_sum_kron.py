#!/usr/bin/env python3
"""Generate tests/golden/g37_sum_kron.npz by running the REAL reference: SumKroneckerLinearOperator, what `+` builds for
two KroneckerProductLinearOperators of one factor layout (A (x) B + C (x) D, a multitask GP with Kronecker noise).

Runs only where the reference is importable; only the .npz output is committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_sum_kron.py

Per case the file holds, for every quantity, the reference's float32 value (`<case>_<q>`), the dense float64 value
(`<case>_<q>_64`: torch float64 solve, logdet, autograd on the dense sum) and the reference's own relative error against
it (`<case>_<q>_err`; of the roots only the residuals of R R^T against the sum and of R_inv R_inv^T against its inverse).
The reference is run through its public calls with its default settings (solve, inv_quad_logdet, root_decomposition,
root_inv_decomposition); it raised on none of the gradients.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_ski import rng  # noqa: E402

# name -> (n1, n2, B)
CASES = {"c1": (24, 3, 1), "c2": (40, 5, 3), "c3": (33, 1, 2), "c4": (7, 19, 1), "c5": (130, 4, 1)}
GRAD_CASES = ("c1", "c2")
MAX_COND = 2000.0


def rbf_gram(seed, n, ls, jitter):
    """RBF Gram matrix on n random points of the unit square, sorted by their first coordinate, plus jitter."""
    x = rng(seed).random((n, 2))
    x = x[np.argsort(x[:, 0])]
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2 / ls ** 2) + jitter * np.eye(n)


def task_factor(seed, n):
    """F F^T / r + 0.3 I with F [n, r] standard normal, r = n + 2."""
    r = n + 2
    f = rng(seed).standard_normal((n, r))
    return f @ f.T / r + 0.3 * np.eye(n)


def inputs():
    """Every input of the fixture, by name (the tests call this too)."""
    d = {}
    for i, (p, (n1, n2, B)) in enumerate(CASES.items()):
        s = 4100 + 50 * i
        d[p + "_A"] = np.stack([rbf_gram(s + b, n1, 0.3, 1e-3) for b in range(B)]).astype(np.float32)
        d[p + "_C"] = np.stack([rbf_gram(s + 10 + b, n1, 0.05, 0.5) for b in range(B)]).astype(np.float32)
        d[p + "_B"] = np.stack([task_factor(s + 20 + b, n2) for b in range(B)]).astype(np.float32)
        d[p + "_D"] = np.stack([task_factor(s + 30 + b, n2) for b in range(B)]).astype(np.float32)
        d[p + "_rhs1"] = rng(s + 40).standard_normal((B, n1 * n2, 1)).astype(np.float32)
        d[p + "_rhs4"] = rng(s + 41).standard_normal((B, n1 * n2, 4)).astype(np.float32)
    return d


def dense64(x, p):
    """The dense float64 sum A (x) B + C (x) D of case p, [B, N, N] (numpy)."""
    A, Bm, C, D = (x[p + "_" + k].astype(np.float64) for k in "ABCD")
    return np.stack([np.kron(A[b], Bm[b]) + np.kron(C[b], D[b]) for b in range(A.shape[0])])


def rel(a, b):
    """Relative error of a against b over the whole array (Frobenius)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator.operators import KroneckerProductLinearOperator, SumKroneckerLinearOperator

    torch.set_default_dtype(torch.float32)
    x = inputs()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    out = {}

    def put(name, ref, exact):
        ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref)
        exact = exact.detach().numpy() if torch.is_tensor(exact) else np.asarray(exact)
        out[name], out[name + "_64"], out[name + "_err"] = ref, exact, rel(ref, exact)

    for p in CASES:
        K64 = T(dense64(x, p))
        cond = float(torch.linalg.cond(K64).max())
        assert cond <= MAX_COND, f"{p}: dense fp64 condition number {cond}"
        out[p + "_cond"] = cond
        f32 = [T(x[p + "_" + k]) for k in "ABCD"]
        op = KroneckerProductLinearOperator(f32[0], f32[1]) + KroneckerProductLinearOperator(f32[2], f32[3])
        assert isinstance(op, SumKroneckerLinearOperator)
        for c in (1, 4):
            rhs = T(x[f"{p}_rhs{c}"])
            put(f"{p}_solve{c}", op.solve(rhs), torch.linalg.solve(K64, rhs.double()))
        rhs = T(x[p + "_rhs4"])
        iq, ld = op.inv_quad_logdet(rhs, logdet=True)
        put(p + "_iq", iq, (rhs.double() * torch.linalg.solve(K64, rhs.double())).sum((-2, -1)))
        put(p + "_ld", ld, torch.logdet(K64))
        Kinv = torch.linalg.inv(K64)
        R = op.root_decomposition().root.to_dense()
        out[p + "_root_err"] = rel(R @ R.mT, K64)  # (residuals only: the N x N products are not kept)
        Ri = op.root_inv_decomposition().root.to_dense()
        out[p + "_root_inv_err"] = rel(Ri @ Ri.mT, Kinv)
        if p in GRAD_CASES:
            leaves = [t.clone().requires_grad_(True) for t in f32]
            gop = KroneckerProductLinearOperator(leaves[0], leaves[1]) + KroneckerProductLinearOperator(leaves[2], leaves[3])
            iq, ld = gop.inv_quad_logdet(rhs, logdet=True)
            (iq.sum() + ld.sum()).backward()
            l64 = [t.double().clone().requires_grad_(True) for t in f32]
            kron = lambda a, b: (a.unsqueeze(-1).unsqueeze(-3) * b.unsqueeze(-2).unsqueeze(-4)).reshape(  # noqa: E731
                a.shape[0], a.shape[-2] * b.shape[-2], a.shape[-1] * b.shape[-1])
            k = kron(l64[0], l64[1]) + kron(l64[2], l64[3])
            ((rhs.double() * torch.linalg.solve(k, rhs.double())).sum() + torch.logdet(k).sum()).backward()
            for name, t32, t64 in zip("ABCD", leaves, l64):
                put(f"{p}_g{name}", t32.grad, t64.grad)
    for k in sorted(out):
        if k.endswith("_err"):
            print(f"{k:24s} {out[k]:.3e}")
    np.savez_compressed(os.path.join(HERE, "g37_sum_kron.npz"), **out)
    print("g37_sum_kron", len(out), "arrays")


if __name__ == "__main__":
    main()
