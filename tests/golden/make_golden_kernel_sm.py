#!/usr/bin/env python3
"""Generate tests/golden/g48_kernel_sm_<case>.npz by running the REAL reference: KernelLinearOperator(X, X,
covar_func=covariance.spectral_mixture, mixture_weights, mixture_means, mixture_scales,
num_nonbatch_dimensions={"mixture_weights": 1}) over this project's covariance function (handed to the reference as
`covar_func`; the reference passes the parameters through), alone and inside AddedDiagLinearOperator(kernel,
DiagLinearOperator(d)).

Runs only where the reference is importable; only the .npz outputs are committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.  The protocol, helpers and quantities
are those of make_golden_kernel_param.py (rel, pivot_gaps, solver_settings, the constants), imported, not copied.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_kernel_sm.py

Per case the file holds, for every quantity q, the reference's float32 CPU value (`q`), the dense float64 value (`q_64`)
and the reference's own relative error against it (`q_err`).  Quantities: mv (K V, 4 columns), diag, solve ((K + D)^-1 rhs
under SETTINGS), iq (inv_quad(rhs)), L / piv (pivoted_cholesky(RANK) of the kernel operator), gw / gm / gs / gx (gradients
of inv_quad(rhs) with respect to the weights, the means, the scales and the points, one leaf for both sides) and ld (the
logdet estimate of inv_quad_logdet with the probes Z injected through _probe_vectors_and_norms; its float64 value is the
reference's own run in float64 on the same probes).

Cases: `ts`, the time-series case (one input dimension, four mixtures, short correlation lengths, the points over 77 periods of the fastest mixture) and
`ard` (three input dimensions, two mixtures, two members).  The diagonal of K is sum_q w_q for every point: step 0 of the
pivoted Cholesky ties exactly and the lowest index wins.  The pivots are a fixture only under the rule of
make_golden_kernel_op.py (float32 and float64 runs of the reference agree; in a float64 replay every step leads by more
than PIVOT_GAP or ties exactly), and the gradient sums only under the GRAD_COND cap of make_golden_kernel_lmc.py, computed
here for every scalar parameter (`gcond`).  main() asserts both; the seeds, frequency ranges and noise multiples below are
ones for which the reference alone satisfies both.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_kernel_param import (  # noqa: E402,F401
    ERR_FLOOR, GRAD_COND, PIVOT_GAP, PROBES, RANK, pivot_gaps, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

# name -> (B, n, D, Q, seed)
CASES = {
    "ts": (1, 257, 1, 4, 8001),
    "ard": (2, 130, 3, 2, 8014),
}
SPAN = {"ts": 257.0, "ard": 1.0}  # the points are uniform on [0, SPAN]^D (ts: one sample per unit of time on average)
# the bandwidths sigma form a geometric ladder from the first to the second value over the mixtures, each jittered by
# 0.8 .. 1.2.  ard: correlation lengths 1 / (2 pi sigma) of the order of the cube, as g40 / g47 have them: the residuals of
# the pivoted Cholesky peak at the cube's corners and edges, apart.  ts: in ONE dimension 257 points lie so densely that a
# smooth residual's best and second-best candidate (neighbours, at a smooth maximum) differ quadratically little, whatever
# the seed; the rule holds only with correlation lengths of about a sample and below (1.0 .. 0.26 samples here), where the
# points no pivot has touched tie EXACTLY and the lowest index wins, as at step 0 -- and only for seeds where the float32
# and the float64 run of the reference agree on which points count as touched (about one seed in ten)
SCALES = {"ts": (0.156, 0.62), "ard": (0.2, 0.35)}
# the frequencies mu (cycles per unit) as multiples of the mixture's own bandwidth: mu = sigma * uniform(lo, hi)
MEANS = {"ts": (0.2, 1.0), "ard": (0.25, 1.0)}
# the noise diagonal as a multiple of g40's 0.05 .. 0.15: the smaller the noise, the more the solve oscillates and the more
# the gradient sums cancel (the handle on GRAD_COND, as in make_golden_kernel_param.py)
NOISE = {"ts": 16.0, "ard": 16.0}
RHS_MEAN = {"ts": 3.0, "ard": 5.0}
NB = {"mixture_weights": 1}
PARAMS = ("mixture_weights", "mixture_means", "mixture_scales")
GRADS = {"gx": "x", "gw": "mixture_weights", "gm": "mixture_means", "gs": "mixture_scales"}


def inputs(p):
    """Every input of case p, by name (the tests call this too)."""
    B, n, D, Q, seed = CASES[p]
    g = rng(seed)
    d = {}
    d["x"] = (SPAN[p] * g.random((B, n, D))).astype(np.float32)
    d["mixture_weights"] = (0.3 + 0.7 * g.random((B, Q))).astype(np.float32)
    lo, hi = SCALES[p]
    ladder = lo * (hi / lo) ** (np.arange(Q) / max(Q - 1, 1))
    d["mixture_scales"] = (ladder[None, :, None] * (0.8 + 0.4 * g.random((B, Q, D)))).astype(np.float32)
    lo, hi = MEANS[p]
    d["mixture_means"] = (d["mixture_scales"] * (lo + (hi - lo) * g.random((B, Q, D)))).astype(np.float32)
    d["noise"] = (NOISE[p] * (0.05 + 0.1 * g.random((B, n)))).astype(np.float32)
    d["rhs"] = (RHS_MEAN[p] + g.standard_normal((B, n, 1))).astype(np.float32)
    d["V"] = g.standard_normal((B, n, 4)).astype(np.float32)
    d["Z"] = g.standard_normal((B, n, PROBES)).astype(np.float32)
    return d


def conditions(p, x=None):
    """(the worst GRAD_COND ratio per scalar parameter, the near-tied pivot steps per member, the float64 pivots) of case p
    from the dense float64 matrix alone: what main() asserts, without the reference."""
    import torch
    import torch.autograd.forward_ad as fwd

    from linear_operator_amd import covariance

    B, n, D, Q, seed = CASES[p]
    x = inputs(p) if x is None else x
    t64 = {k: torch.from_numpy(v).double() for k, v in x.items()}

    def dense(**replace):
        return covariance.spectral_mixture(t64["x"], t64["x"], *(replace.get(k, t64[k]) for k in PARAMS))

    K64 = dense()
    A64 = K64 + torch.diag_embed(t64["noise"])
    s = torch.linalg.solve(A64, t64["rhs"])
    w = s @ s.mT
    gcond = []
    for name in PARAMS:
        for k in range(t64[name][0].numel()):
            tangent = torch.zeros_like(t64[name]).reshape(B, -1)
            tangent[:, k] = 1.0
            with fwd.dual_level():
                dK = fwd.unpack_dual(dense(**{name: fwd.make_dual(t64[name], tangent.reshape(t64[name].shape))})).tangent
            gcond.append(float(((w * dK).abs().sum((-2, -1)) / (w * dK).sum((-2, -1)).abs()).max()))
    bad, pivots = [], []
    for b in range(B):
        piv, gaps = pivot_gaps(K64[b].numpy(), RANK)
        pivots.append(piv)
        bad += [(b, m, gp) for m, gp in enumerate(gaps) if 1e-12 < gp <= PIVOT_GAP]
        if not (gaps[0] <= 1e-12 and piv[0] == 0):  # (a constant diagonal: the first point wins)
            bad.append((b, 0, gaps[0]))
    return np.asarray(gcond), bad, np.stack(pivots)


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

    from linear_operator_amd import covariance

    torch.set_default_dtype(torch.float32)
    fn = covariance.MIXTURE_FAMILIES["spectral_mixture"]
    for p, (B, n, D, Q, seed) in CASES.items():
        x = inputs(p)
        out = {}

        def put(name, ref, exact):
            ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref)
            exact = exact.detach().numpy() if torch.is_tensor(exact) else np.asarray(exact)
            out[name], out[name + "_64"], out[name + "_err"] = ref, exact, rel(ref, exact)

        def tensors(dtype, grad=False):
            t = {k: torch.from_numpy(v).to(dtype) for k, v in x.items()}
            if grad:
                for k in GRADS.values():
                    t[k].requires_grad_(True)
            return t

        def sm_op(t):
            return KernelLinearOperator(t["x"], t["x"], fn, num_nonbatch_dimensions=NB, **{k: t[k] for k in PARAMS})

        def dense(t):
            return fn(t["x"], t["x"], *(t[k] for k in PARAMS))

        t32, t64 = tensors(torch.float32), tensors(torch.float64)
        K64 = dense(t64)
        A64 = K64 + torch.diag_embed(t64["noise"])
        out["cond"] = float(torch.linalg.cond(A64).max())
        # the points cover this many periods of the fastest mixture (the range reduction is exercised by the fixture too)
        out["periods"] = float(((x["x"].max(1) - x["x"].min(1))[:, None, :] * x["mixture_means"]).max())
        gcond, bad, piv_replay = conditions(p, x)
        assert gcond.max() <= GRAD_COND, f"{p}: a parameter's gradient sum cancels by {gcond.max():.0f}"
        assert not bad, f"{p}: near-tied pivot candidates {bad}"
        out["gcond"] = gcond
        op = sm_op(t32)
        put("mv", op @ t32["V"], K64 @ t64["V"])
        put("diag", op.diagonal(dim1=-1, dim2=-2), K64.diagonal(dim1=-1, dim2=-2))
        with solver_settings(settings):
            sol = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"])).solve(t32["rhs"])
        put("solve", sol, torch.linalg.solve(A64, t64["rhs"]))
        # pivoted Cholesky: float32 and float64 runs of the reference, and the replay
        L32, piv32 = op.pivoted_cholesky(RANK, return_pivots=True)
        L64, piv64 = sm_op(t64).pivoted_cholesky(RANK, return_pivots=True)
        assert torch.equal(piv32[..., :RANK], piv64[..., :RANK]), f"{p}: float32 and float64 pivots differ"
        assert np.array_equal(piv_replay, piv64[..., :RANK].numpy()), f"{p}: the replay's pivots differ"
        put("L", L32, L64)
        out["piv"] = piv32[..., :RANK].numpy()
        # gradients of inv_quad
        g32 = tensors(torch.float32, grad=True)
        with solver_settings(settings):
            iq = AddedDiagLinearOperator(sm_op(g32), DiagLinearOperator(g32["noise"])).inv_quad(g32["rhs"])
        iq.sum().backward()
        g64 = tensors(torch.float64, grad=True)
        k = dense(g64) + torch.diag_embed(g64["noise"])
        (g64["rhs"] * torch.linalg.solve(k, g64["rhs"])).sum().backward()
        put("iq", iq, (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum((-2, -1)))
        for q, name in GRADS.items():
            put(q, g32[name].grad, g64[name].grad)

        # logdet with injected probes
        def probed(t):
            class Probed(AddedDiagLinearOperator):
                def _probe_vectors_and_norms(self):
                    nrm = t["Z"].norm(dim=-2, keepdim=True)
                    return t["Z"] / nrm, nrm

            return Probed(sm_op(t), DiagLinearOperator(t["noise"]))

        with solver_settings(settings), settings.num_trace_samples(PROBES):
            _, ld32 = probed(t32).inv_quad_logdet(t32["rhs"], logdet=True)
            _, ld64 = probed(t64).inv_quad_logdet(t64["rhs"], logdet=True)
        put("ld", ld32, ld64)
        out["ld_dense64"] = torch.logdet(A64).numpy()
        print(p, f"cond {out['cond']:.1f} periods {out['periods']:.1f} gcond {np.round(out['gcond'])}",
              " ".join(f"{k[:-4]} {out[k]:.2e}" for k in sorted(out) if k.endswith("_err")), "ld", out["ld"],
              out["ld_dense64"])
        path = os.path.join(HERE, f"g48_kernel_sm_{p}.npz")
        np.savez_compressed(path, **out)
        print("  ->", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
