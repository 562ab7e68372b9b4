#!/usr/bin/env python3
"""Generate tests/golden/g46_kernel_lmc_<case>.npz by running the REAL reference: the linear model of coregionalisation
SumLinearOperator(KroneckerProductLinearOperator(KernelLinearOperator_q(X, X), DenseLinearOperator(B_q)), q < Q) over this
project's covariance functions (linear_operator_amd.covariance, handed to the reference as `covar_func`), alone and
inside AddedDiagLinearOperator(sum, DiagLinearOperator(d)).  Row and column index i T + t (the data index slowest).

Runs only where the reference is importable; only the .npz outputs are committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.  The protocol is that of
make_golden_kernel_kron.py, whose helpers (dense_kron and, through it, rel, pivot_gaps, solver_settings, the constants)
are imported, not copied.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_kernel_lmc.py

Per case the file holds, for every quantity q, the reference's float32 CPU value (`q`), the dense float64 value (`q_64`)
and the reference's own relative error against it (`q_err`).  Quantities as in g40: mv (4 columns), diag, solve (under
SETTINGS), iq, L / piv (pivoted_cholesky(RANK) of the sum), ld (inv_quad_logdet with the probes Z injected; its float64
value is the reference's own run in float64 on the same probes) and the gradients of inv_quad(rhs): gx (the points, one
leaf for every term and both sides) and, per term q, gl<q> (lengthscale), go<q> (outputscale), gB<q> (task matrix).

Every B_q is symmetric, strictly diagonally dominant with distinct diagonal entries, task 0 largest in every term: the
diagonal of the sum is sum_q outputscale_q^2 B_q[t, t], so the first pivots are decided by the task matrices.  The pivots
are a fixture only under the rule of make_golden_kernel_op.py: the float32 and float64 runs of the reference agree, and in
a float64 replay every step's best candidate leads the second by more than PIVOT_GAP relative or ties with it exactly.
main() asserts both; the seeds below are ones for which they hold.

The terms' lengthscales run from 0.3 to 0.75 of g40's scale, term by term (0.5 and 0.75 in three dimensions, where a
shorter one leaves the kernel so near the identity that the pivot candidates tie).  A term's hyperparameter gradient of inv_quad
is a sum over the pairs, sum_ij w_ij k_q,ij with w from the solve; for a term that is nearly constant over the data it
cancels by orders of magnitude (conditioning sum |w k| / |sum w k| of 1e4 and more at twice g40's scale), and its float32
error is then set by the order in which a run happens to add, not by the solve tolerance every float32 run shares -- a
reference error recorded from ONE such run bounds nothing (float32 rounding times a conditioning of 1e3 is 6e-5, above
the gradient errors the reference records, 1e-5 .. 1e-4).  GRAD_COND caps that conditioning, computed in float64 by
main() for every term (`gcond`), so that the recorded gradient errors are the solve's; NOISE below is the second handle.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_kernel_kron import (  # noqa: E402,F401
    ERR_FLOOR, PIVOT_GAP, PROBES, RANK, SETTINGS, dense_kron, pivot_gaps, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

# name -> (per term (family, ARD lengthscale?, lengthscale as a multiple of g40's 0.35 sqrt(D)), B, n, D, T, seed)
CASES = {
    "q2": ((("rbf", True, 0.5), ("matern52", False, 0.75)), 2, 130, 3, 2, 10508),
    "q4": ((("rbf", True, 0.3), ("matern12", False, 0.45), ("matern32", True, 0.6), ("matern52", False, 0.75)),
           1, 257, 8, 3, 8037),
}


GRAD_COND = 750.0  # sum |w k| / |sum w k| of a term's outputscale gradient, at the most
# the noise diagonal as a multiple of g40's 0.05 .. 0.15: the smaller the noise, the more the solve oscillates and the more
# the gradient sums cancel.  In three dimensions lengthscales short enough for GRAD_COND make the pivot candidates tie, so
# q2 keeps the longer ones and meets GRAD_COND through the noise (0.4 .. 1.2 against a prior variance near 1.5)
NOISE = {"q2": 8.0, "q4": 1.0}


def grad_names(p):
    """The leaves inv_quad is differentiated by: the points and every term's lengthscale, outputscale and task matrix."""
    Q = len(CASES[p][0])
    return ("x",) + tuple(f"{k}{q}" for q in range(Q) for k in ("lengthscale", "outputscale", "task"))


def grad_keys(p):
    """leaf name -> the fixture's key of its gradient"""
    short = {"lengthscale": "gl", "outputscale": "go", "task": "gB"}
    return {name: ("gx" if name == "x" else short[name[:-1]] + name[-1]) for name in grad_names(p)}


def inputs(p):
    """Every input of case p, by name (the tests call this too)."""
    terms, B, n, D, T, seed = CASES[p]
    g = rng(seed)
    N = n * T
    d = {}
    d["x"] = g.random((B, n, D)).astype(np.float32)
    for q, (family, ard, scale) in enumerate(terms):
        base = 0.35 * np.sqrt(D) * scale  # term q's own scale: from local to smooth, none near-constant
        d[f"lengthscale{q}"] = (base * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
        d[f"outputscale{q}"] = (0.6 + 0.5 * g.random(B)).astype(np.float32)
        off = (0.5 + 0.4 * g.random((B, T, T))) / max(T - 1, 1)
        off = 0.5 * (off + off.transpose(0, 2, 1))
        task = off * (1.0 - np.eye(T)) + np.eye(T) * (1.0 + 0.35 * np.arange(T)[::-1] + 0.05 * q)
        d[f"task{q}"] = task.astype(np.float32)
    d["noise"] = (NOISE[p] * (0.05 + 0.1 * g.random((B, N)))).astype(np.float32)
    d["rhs"] = g.standard_normal((B, N, 1)).astype(np.float32)
    d["V"] = g.standard_normal((B, N, 4)).astype(np.float32)
    d["Z"] = g.standard_normal((B, N, PROBES)).astype(np.float32)
    return d


def dense_lmc(p, t, families):
    """sum_q K_q (x) B_q with index i T + t as a torch tensor, from the tensors t of inputs(p); `families`: name -> the
    covariance function."""
    return sum(dense_kron(families[family](t["x"], t["x"], t[f"lengthscale{q}"], t[f"outputscale{q}"]), t[f"task{q}"])
               for q, (family, _, _) in enumerate(CASES[p][0]))


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.operators import (AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator,
                                           KernelLinearOperator, KroneckerProductLinearOperator, SumLinearOperator)

    from linear_operator_amd import covariance

    torch.set_default_dtype(torch.float32)
    for p, (terms, B, n, D, T, seed) in CASES.items():
        x = inputs(p)
        names, keys = grad_names(p), grad_keys(p)
        out = {}

        def put(name, ref, exact):
            ref = ref.detach().numpy() if torch.is_tensor(ref) else np.asarray(ref)
            exact = exact.detach().numpy() if torch.is_tensor(exact) else np.asarray(exact)
            out[name], out[name + "_64"], out[name + "_err"] = ref, exact, rel(ref, exact)

        def tensors(dtype, grad=False):
            t = {k: torch.from_numpy(v).to(dtype) for k, v in x.items()}
            if grad:
                for k in names:
                    t[k].requires_grad_(True)
            return t

        def lmc_op(t):
            ops = []
            for q, (family, _, _) in enumerate(terms):
                kern = KernelLinearOperator(t["x"], t["x"], covariance.FAMILIES[family],
                                            num_nonbatch_dimensions={"outputscale": 0},
                                            lengthscale=t[f"lengthscale{q}"], outputscale=t[f"outputscale{q}"])
                ops.append(KroneckerProductLinearOperator(kern, DenseLinearOperator(t[f"task{q}"])))
            return SumLinearOperator(*ops)

        t32, t64 = tensors(torch.float32), tensors(torch.float64)
        K64 = dense_lmc(p, t64, covariance.FAMILIES)
        A64 = K64 + torch.diag_embed(t64["noise"])
        for q in range(len(terms)):
            assert float(torch.linalg.eigvalsh(t64[f"task{q}"]).min()) > 0.05, f"{p}: B_{q} is not safely positive definite"
        out["cond"] = float(torch.linalg.cond(A64).max())
        s4 = torch.linalg.solve(A64, t64["rhs"]).reshape(B, n, T)
        gcond = []
        for q, (family, _, _) in enumerate(terms):
            Kq = covariance.FAMILIES[family](t64["x"], t64["x"], t64[f"lengthscale{q}"], t64[f"outputscale{q}"])
            w = torch.einsum("bit,bts,bjs->bij", s4, t64[f"task{q}"], s4) * Kq
            gcond.append(float(w.abs().sum() / w.sum().abs()))
        assert max(gcond) <= GRAD_COND, f"{p}: a term's gradient sum cancels by {max(gcond):.0f}"
        out["gcond"] = np.asarray(gcond)
        op = lmc_op(t32)
        put("mv", op @ t32["V"], K64 @ t64["V"])
        put("diag", op.diagonal(dim1=-1, dim2=-2), K64.diagonal(dim1=-1, dim2=-2))
        with solver_settings(settings):
            sol = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"])).solve(t32["rhs"])
        put("solve", sol, torch.linalg.solve(A64, t64["rhs"]))
        # pivoted Cholesky: float32 and float64 runs of the reference, and the replay's gaps
        L32, piv32 = op.pivoted_cholesky(RANK, return_pivots=True)
        L64, piv64 = lmc_op(t64).pivoted_cholesky(RANK, return_pivots=True)
        assert torch.equal(piv32[..., :RANK], piv64[..., :RANK]), f"{p}: float32 and float64 pivots differ"
        for b in range(B):
            piv, gaps = pivot_gaps(K64[b].numpy(), RANK)
            assert np.array_equal(piv, piv64[b, :RANK].numpy()), f"{p}[{b}]: the replay's pivots differ"
            bad = [(m, gp) for m, gp in enumerate(gaps) if 1e-12 < gp <= PIVOT_GAP]
            assert not bad, f"{p}[{b}]: near-tied pivot candidates {bad}"
            assert piv[0] == 0, f"{p}[{b}]: step 0"  # (task 0 has the largest diagonal; its data points tie, the first wins)
        put("L", L32, L64)
        out["piv"] = piv32[..., :RANK].numpy()
        # gradients of inv_quad
        g32 = tensors(torch.float32, grad=True)
        with solver_settings(settings):
            iq = AddedDiagLinearOperator(lmc_op(g32), DiagLinearOperator(g32["noise"])).inv_quad(g32["rhs"])
        iq.sum().backward()
        g64 = tensors(torch.float64, grad=True)
        k = dense_lmc(p, g64, covariance.FAMILIES) + torch.diag_embed(g64["noise"])
        (g64["rhs"] * torch.linalg.solve(k, g64["rhs"])).sum().backward()
        put("iq", iq, (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum((-2, -1)))
        for name in names:
            put(keys[name], g32[name].grad, g64[name].grad)

        # logdet with injected probes
        def probed(t):
            class Probed(AddedDiagLinearOperator):
                def _probe_vectors_and_norms(self):
                    nrm = t["Z"].norm(dim=-2, keepdim=True)
                    return t["Z"] / nrm, nrm

            return Probed(lmc_op(t), DiagLinearOperator(t["noise"]))

        with solver_settings(settings), settings.num_trace_samples(PROBES):
            _, ld32 = probed(t32).inv_quad_logdet(t32["rhs"], logdet=True)
            _, ld64 = probed(t64).inv_quad_logdet(t64["rhs"], logdet=True)
        put("ld", ld32, ld64)
        out["ld_dense64"] = torch.logdet(A64).numpy()
        print(p, f"cond {out['cond']:.1f} gcond {np.round(out['gcond'])}", " ".join(f"{k[:-4]} {out[k]:.2e}" for k in sorted(out) if k.endswith("_err")),
              "ld", out["ld"], out["ld_dense64"])
        path = os.path.join(HERE, f"g46_kernel_lmc_{p}.npz")
        np.savez_compressed(path, **out)
        print("  ->", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
