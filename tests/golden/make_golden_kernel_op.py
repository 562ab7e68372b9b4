#!/usr/bin/env python3
"""Generate tests/golden/g38_kernel_op_<case>.npz by running the REAL reference: its KernelLinearOperator over this
project's covariance functions (linear_operator_amd.covariance, handed to the reference as `covar_func`), alone and
inside AddedDiagLinearOperator(K, DiagLinearOperator(d)).

Runs only where the reference is importable; only the .npz outputs are committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_kernel_op.py

Per case the file holds, for every quantity q, the reference's float32 CPU value (`q`), the dense float64 value (`q_64`:
the same covariance function in float64, torch.linalg on the dense matrix, autograd) and the reference's own relative
error against it (`q_err`).  Quantities: mv (K V, 4 columns), diag, idx (entries through tensor indices), solve
((K + D)^-1 rhs under SETTINGS), L / piv (pivoted_cholesky(RANK) of K), gl / go / gx (gradients of inv_quad(rhs) of
K + D with respect to lengthscale, outputscale and the points, x1 and x2 being one tensor), ld (the logdet estimate of
inv_quad_logdet with the probes Z injected through _probe_vectors_and_norms; its float64 value is the reference's own run
in float64 on the same probes), sqrt ((K + D)^-1/2 rhs by sqrt_inv_matmul against the float64 eigendecomposition) and
root_err (the residual of R R^T from root_decomposition against K + D; R itself starts from a random vector and is not kept).

The pivots are a fixture only where they are well determined: the float32 and float64 runs of the reference must agree, and
in a float64 replay of the algorithm on the dense matrix the best candidate of every step must lead the second by more
than PIVOT_GAP relative -- or tie with it exactly, as all candidates do at step 0 (a stationary kernel has a constant
diagonal; the lowest index wins, as in torch.argmax).  main() asserts both.
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_ski import rng  # noqa: E402

# name -> (family, B, N, D, ARD lengthscale?, seed)
CASES = {
    "rbf": ("rbf", 3, 257, 3, True, 5114),
    "m12": ("matern12", 1, 63, 1, False, 5420),
    "m32": ("matern32", 1, 300, 32, True, 5443),
    "m52": ("matern52", 1, 1013, 8, False, 5415),
}
RANK = 15
PROBES = 6
PIVOT_GAP = 1e-3
ERR_FLOOR = 1e-7  # a recorded error below this is taken as this (the tests' bound is a multiple of it)
# the solver settings of the reference run; the tests enter the same ones (both packages name them alike)
SETTINGS = {"max_cholesky_size": 0, "min_preconditioning_size": 0, "cg_tolerance": 1e-3}


def solver_settings(settings):
    """The SETTINGS as one context manager over the `settings` module of either package."""
    stack = contextlib.ExitStack()
    for name, val in SETTINGS.items():
        stack.enter_context(getattr(settings, name)(val))
    return stack


def inputs(p):
    """Every input of case p, by name (the tests call this too)."""
    family, B, N, D, ard, seed = CASES[p]
    g = rng(seed)
    d = {}
    d["x"] = g.random((B, N, D)).astype(np.float32)
    # lengthscales that keep a row's neighbourhood populated: ~ sqrt(D) / 3 of the unit cube's diameter scale
    base = 0.35 * np.sqrt(D)
    d["lengthscale"] = (base * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    d["outputscale"] = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    d["noise"] = (0.05 + 0.1 * g.random((B, N))).astype(np.float32)
    d["rhs"] = g.standard_normal((B, N, 1)).astype(np.float32)
    d["V"] = g.standard_normal((B, N, 4)).astype(np.float32)
    d["Z"] = g.standard_normal((B, N, PROBES)).astype(np.float32)
    n_idx = 40
    d["ib"] = g.integers(0, B, n_idx)
    d["ir"] = g.integers(0, N, n_idx)
    d["ic"] = g.integers(0, N, n_idx)
    d["ic"][:3] = d["ir"][:3]  # (a few diagonal entries: r = 0)
    return d


def rel(a, b):
    """Relative error of a against b over the whole array (Frobenius)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def pivot_gaps(K, rank):
    """Float64 replay of the greedy pivoted Cholesky on the dense K [N, N]: (pivots, per step the relative lead of the
    best remaining diagonal entry over the second)."""
    n = K.shape[0]
    diag = np.diag(K).copy()
    L = np.zeros((rank, n))
    perm = np.arange(n)
    gaps = []
    for m in range(rank):
        rest = diag[perm[m:]]
        order = np.argsort(-rest, kind="stable")
        best = rest[order[0]]
        gaps.append(float((best - rest[order[1]]) / best) if rest.size > 1 else 1.0)
        j = m + int(order[0])
        perm[[m, j]] = perm[[j, m]]
        piv = perm[m]
        L[m, piv] = np.sqrt(diag[piv])
        others = perm[m + 1:]
        row = K[piv, others] - L[:m, piv] @ L[:m, others]
        L[m, others] = row / L[m, piv]
        diag[others] -= L[m, others] ** 2
    return perm[:rank].copy(), gaps


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

    from linear_operator_amd import covariance

    torch.set_default_dtype(torch.float32)
    for p, (family, B, N, D, ard, seed) in CASES.items():
        x = inputs(p)
        fn = covariance.FAMILIES[family]
        out = {}

        def put(name, ref, exact):
            ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref)
            exact = exact.detach().numpy() if torch.is_tensor(exact) else np.asarray(exact)
            out[name], out[name + "_64"], out[name + "_err"] = ref, exact, rel(ref, exact)

        def tensors(dtype, grad=False):
            t = {k: torch.from_numpy(x[k]).to(dtype) for k in ("x", "lengthscale", "outputscale", "noise", "rhs", "V", "Z")}
            if grad:
                for k in ("x", "lengthscale", "outputscale"):
                    t[k].requires_grad_(True)
            return t

        def kernel_op(t):
            return KernelLinearOperator(t["x"], t["x"], fn, num_nonbatch_dimensions={"outputscale": 0},
                                        lengthscale=t["lengthscale"], outputscale=t["outputscale"])

        t32, t64 = tensors(torch.float32), tensors(torch.float64)
        K64 = fn(t64["x"], t64["x"], t64["lengthscale"], t64["outputscale"])
        A64 = K64 + torch.diag_embed(t64["noise"])
        out["cond"] = float(torch.linalg.cond(A64).max())
        op = kernel_op(t32)
        put("mv", op @ t32["V"], K64 @ t64["V"])
        put("diag", op.diagonal(dim1=-1, dim2=-2), K64.diagonal(dim1=-1, dim2=-2))
        ib, ir, ic = (torch.from_numpy(x[k]) for k in ("ib", "ir", "ic"))
        put("idx", op[ib, ir, ic], K64[ib, ir, ic])
        with solver_settings(settings):
            sol = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"])).solve(t32["rhs"])
        put("solve", sol, torch.linalg.solve(A64, t64["rhs"]))
        # pivoted Cholesky: float32 and float64 runs of the reference, and the replay's gaps
        L32, piv32 = op.pivoted_cholesky(RANK, return_pivots=True)
        L64, piv64 = kernel_op(t64).pivoted_cholesky(RANK, return_pivots=True)
        assert torch.equal(piv32[..., :RANK], piv64[..., :RANK]), f"{p}: float32 and float64 pivots differ"
        for b in range(B):
            piv, gaps = pivot_gaps(K64[b].numpy(), RANK)
            assert np.array_equal(piv, piv64[b, :RANK].numpy()), f"{p}[{b}]: the replay's pivots differ"
            bad = [(m, gp) for m, gp in enumerate(gaps) if 1e-12 < gp <= PIVOT_GAP]
            assert not bad, f"{p}[{b}]: near-tied pivot candidates {bad}"
            assert gaps[0] <= 1e-12 and piv[0] == 0, f"{p}[{b}]: step 0 is not the exact tie of a constant diagonal"
        put("L", L32, L64)
        out["piv"] = piv32[..., :RANK].numpy()
        # gradients of inv_quad
        g32 = tensors(torch.float32, grad=True)
        with solver_settings(settings):
            iq = AddedDiagLinearOperator(kernel_op(g32), DiagLinearOperator(g32["noise"])).inv_quad(g32["rhs"])
        iq.sum().backward()
        g64 = tensors(torch.float64, grad=True)
        k = fn(g64["x"], g64["x"], g64["lengthscale"], g64["outputscale"]) + torch.diag_embed(g64["noise"])
        (g64["rhs"] * torch.linalg.solve(k, g64["rhs"])).sum().backward()
        put("iq", iq, (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum((-2, -1)))
        put("gl", g32["lengthscale"].grad, g64["lengthscale"].grad)
        put("go", g32["outputscale"].grad, g64["outputscale"].grad)
        put("gx", g32["x"].grad, g64["x"].grad)
        # logdet with injected probes, sqrt_inv_matmul, the Lanczos root
        def probed(t):
            class Probed(AddedDiagLinearOperator):
                def _probe_vectors_and_norms(self):
                    n = t["Z"].norm(dim=-2, keepdim=True)
                    return t["Z"] / n, n

            return Probed(kernel_op(t), DiagLinearOperator(t["noise"]))

        with solver_settings(settings), settings.num_trace_samples(PROBES):
            _, ld32 = probed(t32).inv_quad_logdet(t32["rhs"], logdet=True)
            _, ld64 = probed(t64).inv_quad_logdet(t64["rhs"], logdet=True)
            A32 = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"]))
            torch.manual_seed(seed)
            sq = A32.sqrt_inv_matmul(t32["rhs"])
            R = A32.root_decomposition().root.to_dense()
        put("ld", ld32, ld64)
        out["ld_dense64"] = torch.logdet(A64).numpy()
        evals, evecs = torch.linalg.eigh(A64)
        put("sqrt", sq, evecs @ ((evecs.mT @ t64["rhs"]) / evals.sqrt().unsqueeze(-1)))
        out["root_err"] = rel(R.double() @ R.double().mT, A64)
        print(p, f"cond {out['cond']:.1f}", " ".join(f"{k[:-4]} {out[k]:.2e}" for k in sorted(out) if k.endswith("_err")),
              "ld", out["ld"], out["ld_dense64"])
        path = os.path.join(HERE, f"g38_kernel_op_{p}.npz")
        np.savez_compressed(path, **out)
        print("  ->", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
