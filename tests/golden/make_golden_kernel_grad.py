#!/usr/bin/env python3
"""Generate tests/golden/g41_kernel_grad_<case>.npz by running the REAL reference: the covariance of the values and the
D partial derivatives of an RBF GP, KernelLinearOperator(X, X, covariance.rbf_grad, num_outputs_per_input=(D + 1, D + 1))
over this project's covariance function (handed to the reference as `covar_func`), alone and inside
AddedDiagLinearOperator(op, DiagLinearOperator(d)).  Row and column index i (D + 1) + a (the data index slowest; a = 0
the value, a = 1 .. D the derivative in coordinate a - 1).

Runs only where the reference is importable; only the .npz outputs are committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.  The protocol is that of
make_golden_kernel_op.py, whose helpers (rel, pivot_gaps, solver_settings, the constants) are imported, not copied.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_kernel_grad.py

Per case the file holds, for every quantity q, the reference's float32 CPU value (`q`), the dense float64 value (`q_64`)
and the reference's own relative error against it (`q_err`).  Quantities: mv (K V, 4 columns), diag, solve ((K + D)^-1 rhs
under SETTINGS), iq (inv_quad(rhs)), L / piv (pivoted_cholesky(RANK) of K), gl / go (gradients of inv_quad(rhs) with
respect to the ARD lengthscale and the outputscale) and ld (the logdet estimate of inv_quad_logdet with the probes Z
injected through _probe_vectors_and_norms; its float64 value is the reference's own run in float64 on the same probes).
Every quantity came from the reference on the CPU.

Pivots.  The diagonal of K is outputscale^2 (1, 1 / l_1^2, .., 1 / l_D^2) at every point: at step 0 the entries of the
dimension with the smallest lengthscale tie exactly across the points and the lowest index wins, as in torch.argmax.
Later steps nearly tie for most seeds, so the seeds below were searched (search() prints, per shape, which of 60 seeds
from 9100 pass): the pivots are a fixture only where the float32 and float64 runs of the reference agree and in a float64
replay every step's best candidate leads the second by more than PIVOT_GAP relative or ties with it exactly.  main()
asserts both.  A shared lengthscale makes all derivative slots tie at every step: that case is covered by the dense
comparisons of the tests, not by a pivot fixture.
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

# name -> (B, n, D, seed)
CASES = {
    "a": (2, 70, 3, 9129),
    "b": (1, 129, 6, 9107),
}
GRAD_NAMES = ("lengthscale", "outputscale")


def points(B, n, D, seed):
    """x, the ARD lengthscale and the outputscale: the first draws of the seed (what the pivots depend on)."""
    g = rng(seed)
    d = {}
    d["x"] = g.random((B, n, D)).astype(np.float32)
    d["lengthscale"] = (0.35 * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D)))).astype(np.float32)
    d["outputscale"] = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    return d, g


def inputs(p):
    """Every input of case p, by name (the tests call this too)."""
    B, n, D, seed = CASES[p]
    d, g = points(B, n, D, seed)
    N = n * (D + 1)
    d["noise"] = (0.05 + 0.1 * g.random((B, N))).astype(np.float32)
    d["rhs"] = g.standard_normal((B, N, 1)).astype(np.float32)
    d["V"] = g.standard_normal((B, N, 4)).astype(np.float32)
    d["Z"] = g.standard_normal((B, N, PROBES)).astype(np.float32)
    return d


def pivots_well_determined(K64, first_diag_argmax):
    """The gap rule on one member's float64 matrix: (pivots, the near-tied steps)."""
    piv, gaps = pivot_gaps(K64, RANK)
    bad = [(m, gp) for m, gp in enumerate(gaps) if 1e-12 < gp <= PIVOT_GAP]
    if piv[0] != first_diag_argmax:
        bad.append((0, "step 0 is not the first largest diagonal entry"))
    return piv, bad


def search(shapes=((2, 70, 3), (1, 129, 6)), first=9100, count=60):
    """Which seeds give well-determined pivots (no reference needed)."""
    import torch

    from linear_operator_amd import covariance

    for B, n, D in shapes:
        good = []
        for seed in range(first, first + count):
            t = {k: torch.from_numpy(v).double() for k, v in points(B, n, D, seed)[0].items()}
            K64 = covariance.rbf_grad(t["x"], t["x"], t["lengthscale"], t["outputscale"])
            if all(not pivots_well_determined(K64[b].numpy(), int(K64[b].diagonal().argmax()))[1] for b in range(B)):
                good.append(seed)
        print((B, n, D), "seeds with well-determined pivots:", good)


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

    from linear_operator_amd import covariance

    torch.set_default_dtype(torch.float32)
    fn = covariance.rbf_grad
    for p, (B, n, D, seed) in CASES.items():
        x = inputs(p)
        out = {}

        def put(name, ref, exact):
            ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref)
            exact = exact.detach().numpy() if torch.is_tensor(exact) else np.asarray(exact)
            out[name], out[name + "_64"], out[name + "_err"] = ref, exact, rel(ref, exact)

        def tensors(dtype, grad=False):
            t = {k: torch.from_numpy(v).to(dtype) for k, v in x.items()}
            if grad:
                for k in GRAD_NAMES:
                    t[k].requires_grad_(True)
            return t

        def grad_op(t):
            return KernelLinearOperator(t["x"], t["x"], fn, num_outputs_per_input=(D + 1, D + 1),
                                        num_nonbatch_dimensions={"outputscale": 0}, lengthscale=t["lengthscale"],
                                        outputscale=t["outputscale"])

        def dense(t):
            return fn(t["x"], t["x"], t["lengthscale"], t["outputscale"])

        t32, t64 = tensors(torch.float32), tensors(torch.float64)
        K64 = dense(t64)
        A64 = K64 + torch.diag_embed(t64["noise"])
        out["cond"] = float(torch.linalg.cond(A64).max())
        op = grad_op(t32)
        assert op.shape == K64.shape
        put("mv", op @ t32["V"], K64 @ t64["V"])
        put("diag", op.diagonal(dim1=-1, dim2=-2), K64.diagonal(dim1=-1, dim2=-2))
        with solver_settings(settings):
            sol = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"])).solve(t32["rhs"])
        put("solve", sol, torch.linalg.solve(A64, t64["rhs"]))
        # pivoted Cholesky: float32 and float64 runs of the reference, and the replay's gaps
        L32, piv32 = op.pivoted_cholesky(RANK, return_pivots=True)
        L64, piv64 = grad_op(t64).pivoted_cholesky(RANK, return_pivots=True)
        assert torch.equal(piv32[..., :RANK], piv64[..., :RANK]), f"{p}: float32 and float64 pivots differ"
        for b in range(B):
            piv, bad = pivots_well_determined(K64[b].numpy(), int(K64[b].diagonal().argmax()))
            assert np.array_equal(piv, piv64[b, :RANK].numpy()), f"{p}[{b}]: the replay's pivots differ"
            assert not bad, f"{p}[{b}]: near-tied pivot candidates {bad}"
            # step 0: the derivative slot of the smallest lengthscale, tied exactly across the points, at point 0
            assert piv[0] == 1 + int(np.argmin(x["lengthscale"][b, 0])) and x["lengthscale"][b].min() < 1.0, f"{p}[{b}]"
        put("L", L32, L64)
        out["piv"] = piv32[..., :RANK].numpy()
        # gradients of inv_quad
        g32 = tensors(torch.float32, grad=True)
        with solver_settings(settings):
            iq = AddedDiagLinearOperator(grad_op(g32), DiagLinearOperator(g32["noise"])).inv_quad(g32["rhs"])
        iq.sum().backward()
        g64 = tensors(torch.float64, grad=True)
        k = dense(g64) + torch.diag_embed(g64["noise"])
        (g64["rhs"] * torch.linalg.solve(k, g64["rhs"])).sum().backward()
        put("iq", iq, (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum((-2, -1)))
        put("gl", g32["lengthscale"].grad, g64["lengthscale"].grad)
        put("go", g32["outputscale"].grad, g64["outputscale"].grad)

        # logdet with injected probes
        def probed(t):
            class Probed(AddedDiagLinearOperator):
                def _probe_vectors_and_norms(self):
                    nrm = t["Z"].norm(dim=-2, keepdim=True)
                    return t["Z"] / nrm, nrm

            return Probed(grad_op(t), DiagLinearOperator(t["noise"]))

        with solver_settings(settings), settings.num_trace_samples(PROBES):
            _, ld32 = probed(t32).inv_quad_logdet(t32["rhs"], logdet=True)
            _, ld64 = probed(t64).inv_quad_logdet(t64["rhs"], logdet=True)
        put("ld", ld32, ld64)
        out["ld_dense64"] = torch.logdet(A64).numpy()
        print(p, f"cond {out['cond']:.1f}", " ".join(f"{k[:-4]} {out[k]:.2e}" for k in sorted(out) if k.endswith("_err")),
              "ld", out["ld"], out["ld_dense64"])
        path = os.path.join(HERE, f"g41_kernel_grad_{p}.npz")
        np.savez_compressed(path, **out)
        print("  ->", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "search":
        search()
    else:
        main()
