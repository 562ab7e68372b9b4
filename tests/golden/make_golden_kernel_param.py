#!/usr/bin/env python3
"""Generate tests/golden/g47_kernel_param_<case>.npz by running the REAL reference: KernelLinearOperator(X, X,
covar_func=covariance.rq | covariance.periodic, lengthscale, outputscale, alpha | period_length) over this project's
covariance functions (handed to the reference as `covar_func`; the reference passes extra parameters through), alone and
inside AddedDiagLinearOperator(kernel, DiagLinearOperator(d)).

Runs only where the reference is importable; only the .npz outputs are committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.  The protocol, helpers and quantities
are those of make_golden_kernel_op.py / make_golden_kernel_task.py (rel, pivot_gaps, solver_settings, the constants),
imported, not copied.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_kernel_param.py

Per case the file holds, for every quantity q, the reference's float32 CPU value (`q`), the dense float64 value (`q_64`)
and the reference's own relative error against it (`q_err`).  Quantities: mv (K V, 4 columns), diag, solve ((K + D)^-1 rhs
under SETTINGS), iq (inv_quad(rhs)), L / piv (pivoted_cholesky(RANK) of the kernel operator), gl / go / gs / gx (gradients
of inv_quad(rhs) with respect to the lengthscale, the outputscale, the shape parameter -- alpha or period_length -- and
the points, one leaf for both sides) and ld (the logdet estimate of inv_quad_logdet with the probes Z injected through
_probe_vectors_and_norms; its float64 value is the reference's own run in float64 on the same probes).

The diagonal of K is outputscale^2 for every point: step 0 of the pivoted Cholesky ties exactly and the lowest index wins.
The pivots are a fixture only under the rule of make_golden_kernel_op.py: the float32 and float64 runs of the reference
agree, and in a float64 replay every step's best candidate leads the second by more than PIVOT_GAP relative or ties with
it exactly.  A hyperparameter's gradient of inv_quad is a sum over the pairs, sum_ij w_ij dK_ij / dp with w from the
solve; where it cancels by orders of magnitude its float32 error is set by the order in which a run happens to add (see
make_golden_kernel_lmc.py).  GRAD_COND caps that conditioning, sum |w dK| / |sum w dK|, computed in float64 with
forward-mode derivatives for every scalar parameter (`gcond`).  main() asserts all of it; the seeds and scales below are
ones for which the reference alone satisfies both.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_kernel_lmc import GRAD_COND  # noqa: E402
from make_golden_kernel_task import (  # noqa: E402,F401
    ERR_FLOOR, PIVOT_GAP, PROBES, RANK, SETTINGS, pivot_gaps, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

# name -> (B, n, D, seed); both cases have ARD lengthscales, the periodic one ARD periods too
CASES = {
    "rq": (2, 130, 3, 8471),
    "periodic": (1, 257, 2, 8472),
}
SHAPE = {"rq": "alpha", "periodic": "period_length"}  # the family's own parameter
WRAPS, PHASE = 5, 0.45  # periodic: the points lie in WRAPS periods per coordinate, at phases 0 .. PHASE of a period
SPAN = WRAPS - 1.0  # ... and so cover more than this many periods in every coordinate
# the noise diagonal as a multiple of g40's 0.05 .. 0.15: the smaller the noise, the more the solve oscillates and the more
# the gradient sums cancel (the second handle on GRAD_COND, as in make_golden_kernel_lmc.py)
NOISE = {"rq": 16.0, "periodic": 64.0}
LS_RQ = 0.35  # rq: the lengthscales are LS_RQ sqrt(D) (0.7 .. 1.3) on the unit cube (g40's scale: 0.35)
LS_PER = 1.4  # periodic: the lengthscales (0.8 .. 1.2 of it) in units of sin(pi phi), whose range is 1
RHS_MEAN = {"rq": 5.0, "periodic": 3.0}
NB = {"outputscale": 0, "alpha": 0}


def grad_names(p):
    return ("x", "lengthscale", "outputscale", SHAPE[p])


def inputs(p):
    """Every input of case p, by name (the tests call this too)."""
    B, n, D, seed = CASES[p]
    g = rng(seed)
    d = {}
    if p == "rq":
        d["x"] = g.random((B, n, D)).astype(np.float32)
        d["lengthscale"] = (LS_RQ * np.sqrt(D) * (0.7 + 0.6 * g.random((B, 1, D)))).astype(np.float32)
        d["alpha"] = (0.5 + 2.5 * g.random(B)).astype(np.float32)
    else:
        d["period_length"] = (0.8 + 0.4 * g.random((B, 1, D))).astype(np.float32)
        # whole periods 0 .. WRAPS - 1 plus a phase in [0, PHASE): modulo the period the points fill a corner of the torus,
        # where the kernel's residuals peak at the corner's edges as on a cube (over the whole torus they peak in its
        # interior, flat, and the pivot candidates tie)
        phase = PHASE * g.random((B, n, D)) + g.integers(0, WRAPS, (B, n, D))
        d["x"] = (phase * d["period_length"]).astype(np.float32)
        d["lengthscale"] = (LS_PER * (0.8 + 0.4 * g.random((B, 1, D)))).astype(np.float32)
    d["outputscale"] = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    d["noise"] = (NOISE[p] * (0.05 + 0.1 * g.random((B, n)))).astype(np.float32)
    d["rhs"] = (RHS_MEAN[p] + g.standard_normal((B, n, 1))).astype(np.float32)
    d["V"] = g.standard_normal((B, n, 4)).astype(np.float32)
    d["Z"] = g.standard_normal((B, n, PROBES)).astype(np.float32)
    return d


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    import torch.autograd.forward_ad as fwd
    from linear_operator import settings
    from linear_operator.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

    from linear_operator_amd import covariance

    torch.set_default_dtype(torch.float32)
    for p, (B, n, D, seed) in CASES.items():
        x = inputs(p)
        fn, shape = covariance.PARAM_FAMILIES[p], SHAPE[p]
        out = {}

        def put(name, ref, exact):
            ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref)
            exact = exact.detach().numpy() if torch.is_tensor(exact) else np.asarray(exact)
            out[name], out[name + "_64"], out[name + "_err"] = ref, exact, rel(ref, exact)

        def tensors(dtype, grad=False):
            t = {k: torch.from_numpy(v).to(dtype) for k, v in x.items()}
            if grad:
                for k in grad_names(p):
                    t[k].requires_grad_(True)
            return t

        def param_op(t):
            return KernelLinearOperator(t["x"], t["x"], fn, num_nonbatch_dimensions=NB, lengthscale=t["lengthscale"],
                                        outputscale=t["outputscale"], **{shape: t[shape]})

        def dense(t, **replace):
            a = {k: replace.get(k, t[k]) for k in ("lengthscale", "outputscale", shape)}
            return fn(t["x"], t["x"], a["lengthscale"], a["outputscale"], a[shape])

        t32, t64 = tensors(torch.float32), tensors(torch.float64)
        K64 = dense(t64)
        A64 = K64 + torch.diag_embed(t64["noise"])
        out["cond"] = float(torch.linalg.cond(A64).max())
        if p == "periodic":
            span = (x["x"].max(1) - x["x"].min(1)) / x["period_length"][:, 0]
            assert span.min() > SPAN, f"{p}: the points span only {span.min():.1f} periods"
        # the conditioning of every scalar parameter's gradient sum, in float64 (forward-mode dK / dp, all members at once)
        s = torch.linalg.solve(A64, t64["rhs"])
        w = s @ s.mT
        gcond = []
        for name in ("lengthscale", "outputscale", shape):
            for k in range(t64[name][0].numel()):
                tangent = torch.zeros_like(t64[name]).reshape(B, -1)
                tangent[:, k] = 1.0
                with fwd.dual_level():
                    dK = fwd.unpack_dual(dense(t64, **{name: fwd.make_dual(t64[name], tangent.reshape(t64[name].shape))})).tangent
                gcond.append(float(((w * dK).abs().sum((-2, -1)) / (w * dK).sum((-2, -1)).abs()).max()))
        assert max(gcond) <= GRAD_COND, f"{p}: a parameter's gradient sum cancels by {max(gcond):.0f}"
        out["gcond"] = np.asarray(gcond)
        op = param_op(t32)
        put("mv", op @ t32["V"], K64 @ t64["V"])
        put("diag", op.diagonal(dim1=-1, dim2=-2), K64.diagonal(dim1=-1, dim2=-2))
        with solver_settings(settings):
            sol = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"])).solve(t32["rhs"])
        put("solve", sol, torch.linalg.solve(A64, t64["rhs"]))
        # pivoted Cholesky: float32 and float64 runs of the reference, and the replay's gaps
        L32, piv32 = op.pivoted_cholesky(RANK, return_pivots=True)
        L64, piv64 = param_op(t64).pivoted_cholesky(RANK, return_pivots=True)
        assert torch.equal(piv32[..., :RANK], piv64[..., :RANK]), f"{p}: float32 and float64 pivots differ"
        for b in range(B):
            piv, gaps = pivot_gaps(K64[b].numpy(), RANK)
            assert np.array_equal(piv, piv64[b, :RANK].numpy()), f"{p}[{b}]: the replay's pivots differ"
            bad = [(m, gp) for m, gp in enumerate(gaps) if 1e-12 < gp <= PIVOT_GAP]
            assert not bad, f"{p}[{b}]: near-tied pivot candidates {bad}"
            assert gaps[0] <= 1e-12 and piv[0] == 0, f"{p}[{b}]: step 0"  # (a constant diagonal: the first point wins)
        put("L", L32, L64)
        out["piv"] = piv32[..., :RANK].numpy()
        # gradients of inv_quad
        g32 = tensors(torch.float32, grad=True)
        with solver_settings(settings):
            iq = AddedDiagLinearOperator(param_op(g32), DiagLinearOperator(g32["noise"])).inv_quad(g32["rhs"])
        iq.sum().backward()
        g64 = tensors(torch.float64, grad=True)
        k = dense(g64) + torch.diag_embed(g64["noise"])
        (g64["rhs"] * torch.linalg.solve(k, g64["rhs"])).sum().backward()
        put("iq", iq, (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum((-2, -1)))
        put("gl", g32["lengthscale"].grad, g64["lengthscale"].grad)
        put("go", g32["outputscale"].grad, g64["outputscale"].grad)
        put("gs", g32[shape].grad, g64[shape].grad)
        put("gx", g32["x"].grad, g64["x"].grad)

        # logdet with injected probes
        def probed(t):
            class Probed(AddedDiagLinearOperator):
                def _probe_vectors_and_norms(self):
                    nrm = t["Z"].norm(dim=-2, keepdim=True)
                    return t["Z"] / nrm, nrm

            return Probed(param_op(t), DiagLinearOperator(t["noise"]))

        with solver_settings(settings), settings.num_trace_samples(PROBES):
            _, ld32 = probed(t32).inv_quad_logdet(t32["rhs"], logdet=True)
            _, ld64 = probed(t64).inv_quad_logdet(t64["rhs"], logdet=True)
        put("ld", ld32, ld64)
        out["ld_dense64"] = torch.logdet(A64).numpy()
        print(p, f"cond {out['cond']:.1f} gcond {np.round(out['gcond'])}",
              " ".join(f"{k[:-4]} {out[k]:.2e}" for k in sorted(out) if k.endswith("_err")), "ld", out["ld"],
              out["ld_dense64"])
        path = os.path.join(HERE, f"g47_kernel_param_{p}.npz")
        np.savez_compressed(path, **out)
        print("  ->", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
