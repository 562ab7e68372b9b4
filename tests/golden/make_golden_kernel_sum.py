#!/usr/bin/env python3
"""Generate tests/golden/g39_kernel_sum_<case>.npz by running the REAL reference: sums of its KernelLinearOperators over
this project's covariance functions (linear_operator_amd.covariance, handed to the reference as `covar_func`), added with
`+`, alone and inside AddedDiagLinearOperator(K_1 + .. + K_T, DiagLinearOperator(d)).  All terms of a case share one point
tensor.

Runs only where the reference is importable; only the .npz outputs are committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.  The protocol is that of
make_golden_kernel_op.py, whose helpers (rel, pivot_gaps, solver_settings, the constants) are imported, not copied.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_kernel_sum.py

Per case the file holds, for every quantity q, the reference's float32 CPU value (`q`), the dense float64 value (`q_64`)
and the reference's own relative error against it (`q_err`).  Quantities: mv ((sum_t K_t) V, 4 columns), solve
((K + D)^-1 rhs under SETTINGS), L / piv (pivoted_cholesky(RANK) of the sum), gl<t> / go<t> (gradients of inv_quad(rhs)
of K + D with respect to term t's lengthscale and outputscale), gx (with respect to the points, one leaf shared by all
terms and both sides) and ld (the logdet estimate of inv_quad_logdet with the probes Z injected through
_probe_vectors_and_norms; its float64 value is the reference's own run in float64 on the same probes).

The pivots are a fixture only where they are well determined, by the rule of make_golden_kernel_op.py: the float32 and
float64 runs of the reference agree, and in a float64 replay every step's best candidate leads the second by more than
PIVOT_GAP relative or ties with it exactly (step 0: a constant diagonal).  main() asserts both.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_kernel_op import (  # noqa: E402,F401
    ERR_FLOOR, PIVOT_GAP, PROBES, RANK, SETTINGS, pivot_gaps, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

# name -> (families in term order, B, N, D, ARD lengthscales?, seed)
CASES = {
    "rbf_m52": (("rbf", "matern52"), 3, 257, 3, True, 7210),
    "m12_m32_rbf": (("matern12", "matern32", "rbf"), 1, 300, 8, False, 7223),
}


def inputs(p):
    """Every input of case p, by name (the tests call this too): per term t `lengthscale<t>` and `outputscale<t>`."""
    families, B, N, D, ard, seed = CASES[p]
    g = rng(seed)
    d = {}
    d["x"] = g.random((B, N, D)).astype(np.float32)
    base = 0.35 * np.sqrt(D)
    for t in range(len(families)):  # a short and a long scale side by side: term t is (t + 1) / 2 of the base
        scale = base * 0.5 * (t + 1)
        d[f"lengthscale{t}"] = (scale * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
        d[f"outputscale{t}"] = (0.6 + 0.6 * g.random(B)).astype(np.float32)
    d["noise"] = (0.05 + 0.1 * g.random((B, N))).astype(np.float32)
    d["rhs"] = g.standard_normal((B, N, 1)).astype(np.float32)
    d["V"] = g.standard_normal((B, N, 4)).astype(np.float32)
    d["Z"] = g.standard_normal((B, N, PROBES)).astype(np.float32)
    return d


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

    from linear_operator_amd import covariance

    torch.set_default_dtype(torch.float32)
    for p, (families, B, N, D, ard, seed) in CASES.items():
        x = inputs(p)
        fns = [covariance.FAMILIES[f] for f in families]
        T = len(fns)
        out = {}

        def put(name, ref, exact):
            ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref)
            exact = exact.detach().numpy() if torch.is_tensor(exact) else np.asarray(exact)
            out[name], out[name + "_64"], out[name + "_err"] = ref, exact, rel(ref, exact)

        def tensors(dtype, grad=False):
            t = {k: torch.from_numpy(v).to(dtype) for k, v in x.items()}
            if grad:
                for k in t:
                    if k == "x" or k.startswith(("lengthscale", "outputscale")):
                        t[k].requires_grad_(True)
            return t

        def kernel_sum(t):
            ops = [KernelLinearOperator(t["x"], t["x"], fn, num_nonbatch_dimensions={"outputscale": 0},
                                        lengthscale=t[f"lengthscale{k}"], outputscale=t[f"outputscale{k}"])
                   for k, fn in enumerate(fns)]
            total = ops[0]
            for op in ops[1:]:
                total = total + op
            return total

        def dense(t):
            return sum(fn(t["x"], t["x"], t[f"lengthscale{k}"], t[f"outputscale{k}"]) for k, fn in enumerate(fns))

        t32, t64 = tensors(torch.float32), tensors(torch.float64)
        K64 = dense(t64)
        A64 = K64 + torch.diag_embed(t64["noise"])
        out["cond"] = float(torch.linalg.cond(A64).max())
        op = kernel_sum(t32)
        put("mv", op @ t32["V"], K64 @ t64["V"])
        with solver_settings(settings):
            sol = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"])).solve(t32["rhs"])
        put("solve", sol, torch.linalg.solve(A64, t64["rhs"]))
        # pivoted Cholesky: float32 and float64 runs of the reference, and the replay's gaps
        L32, piv32 = op.pivoted_cholesky(RANK, return_pivots=True)
        L64, piv64 = kernel_sum(t64).pivoted_cholesky(RANK, return_pivots=True)
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
            iq = AddedDiagLinearOperator(kernel_sum(g32), DiagLinearOperator(g32["noise"])).inv_quad(g32["rhs"])
        iq.sum().backward()
        g64 = tensors(torch.float64, grad=True)
        k = dense(g64) + torch.diag_embed(g64["noise"])
        (g64["rhs"] * torch.linalg.solve(k, g64["rhs"])).sum().backward()
        put("iq", iq, (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum((-2, -1)))
        for t in range(T):
            put(f"gl{t}", g32[f"lengthscale{t}"].grad, g64[f"lengthscale{t}"].grad)
            put(f"go{t}", g32[f"outputscale{t}"].grad, g64[f"outputscale{t}"].grad)
        put("gx", g32["x"].grad, g64["x"].grad)

        # logdet with injected probes
        def probed(t):
            class Probed(AddedDiagLinearOperator):
                def _probe_vectors_and_norms(self):
                    n = t["Z"].norm(dim=-2, keepdim=True)
                    return t["Z"] / n, n

            return Probed(kernel_sum(t), DiagLinearOperator(t["noise"]))

        with solver_settings(settings), settings.num_trace_samples(PROBES):
            _, ld32 = probed(t32).inv_quad_logdet(t32["rhs"], logdet=True)
            _, ld64 = probed(t64).inv_quad_logdet(t64["rhs"], logdet=True)
        put("ld", ld32, ld64)
        out["ld_dense64"] = torch.logdet(A64).numpy()
        print(p, f"cond {out['cond']:.1f}", " ".join(f"{k[:-4]} {out[k]:.2e}" for k in sorted(out) if k.endswith("_err")),
              "ld", out["ld"], out["ld_dense64"])
        path = os.path.join(HERE, f"g39_kernel_sum_{p}.npz")
        np.savez_compressed(path, **out)
        print("  ->", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
