#!/usr/bin/env python3
"""Generate tests/golden/g43_kernel_task_<case>.npz by running the REAL reference: the task-indexed ("Hadamard")
multitask covariance KernelLinearOperator(X, X, covar_func=covariance.<family>_task, lengthscale, outputscale, task_covar)
over this project's covariance functions (handed to the reference as `covar_func`), alone and inside
AddedDiagLinearOperator(kernel, DiagLinearOperator(d)).  A point is D coordinates and then the task id of the observation;
the tasks have uneven numbers of points.

Runs only where the reference is importable; only the .npz outputs are committed.  Inputs come from inputs() below (numpy
PCG64, seeded; no reference needed): the tests rebuild them from the same function.  The protocol, helpers and quantities
are those of make_golden_kernel_kron.py / make_golden_kernel_op.py (rel, pivot_gaps, solver_settings, the constants),
imported, not copied.
Usage:  [LINEAR_OPERATOR_REFERENCE=<checkout of the reference>] python tests/golden/make_golden_kernel_task.py

Per case the file holds, for every quantity q, the reference's float32 CPU value (`q`), the dense float64 value (`q_64`)
and the reference's own relative error against it (`q_err`).  Quantities: mv (K V, 4 columns), diag, solve ((K + D)^-1 rhs
under SETTINGS), iq (inv_quad(rhs)), L / piv (pivoted_cholesky(RANK) of the kernel operator), gl / go / gx / gB (gradients
of inv_quad(rhs) with respect to the lengthscale, the outputscale, the points -- one leaf for both sides, its task column
has gradient 0 -- and task_covar) and ld (the logdet estimate of inv_quad_logdet with the probes Z injected through
_probe_vectors_and_norms; its float64 value is the reference's own run in float64 on the same probes).

task_covar is symmetric, strictly diagonally dominant with distinct diagonal entries: the diagonal of K is
outputscale^2 task_covar[t_i, t_i], so the first pivot is decided by task_covar (the points of the winning task tie
exactly and the lowest index wins, as in torch.argmax).  The pivots are a fixture only where they are well determined, by
the rule of make_golden_kernel_op.py: the float32 and float64 runs of the reference agree, and in a float64 replay every
step's best candidate leads the second by more than PIVOT_GAP relative or ties with it exactly.  main() asserts both.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_kernel_kron import (  # noqa: E402,F401
    ERR_FLOOR, PIVOT_GAP, PROBES, RANK, SETTINGS, pivot_gaps, rel, solver_settings)
from make_golden_ski import rng  # noqa: E402

# name -> (family, B, n, D, T, ARD lengthscale?, seed)
CASES = {
    "rbf": ("rbf", 2, 130, 3, 2, True, 8435),
    "m52": ("matern52", 1, 257, 8, 3, False, 8471),
}
GRAD_NAMES = ("x", "lengthscale", "outputscale", "task_covar")


def task_ids(g, B, n, T):
    """Ids 0 .. T - 1 with uneven counts (task t is drawn with weight t + 1), every task present in every member."""
    w = np.arange(1, T + 1, dtype=np.float64)
    ids = g.choice(T, size=(B, n), p=w / w.sum())
    ids[:, :T] = np.arange(T)[None, :]
    return ids


def inputs(p):
    """Every input of case p, by name (the tests call this too)."""
    family, B, n, D, T, ard, seed = CASES[p]
    g = rng(seed)
    d = {}
    coords = g.random((B, n, D))
    d["x"] = np.concatenate([coords, task_ids(g, B, n, T)[..., None]], -1).astype(np.float32)
    base = 0.35 * np.sqrt(D)
    d["lengthscale"] = (base * (0.7 + 0.6 * g.random((B, 1, D if ard else 1)))).astype(np.float32)
    d["outputscale"] = (0.8 + 0.7 * g.random(B)).astype(np.float32)
    # off the diagonal 0.5 .. 0.9 split over the other tasks: a row's sum stays below the smallest diagonal entry (1.0)
    off = (0.5 + 0.4 * g.random((B, T, T))) / max(T - 1, 1)
    off = 0.5 * (off + off.transpose(0, 2, 1))
    task = off * (1.0 - np.eye(T)) + np.eye(T) * (1.0 + 0.35 * np.arange(T)[::-1])  # distinct diagonal, task 0 largest
    d["task_covar"] = task.astype(np.float32)
    d["noise"] = (0.05 + 0.1 * g.random((B, n))).astype(np.float32)
    d["rhs"] = g.standard_normal((B, n, 1)).astype(np.float32)
    d["V"] = g.standard_normal((B, n, 4)).astype(np.float32)
    d["Z"] = g.standard_normal((B, n, PROBES)).astype(np.float32)
    return d


def main():
    if os.environ.get("LINEAR_OPERATOR_REFERENCE"):  # a checkout of the reference that is not installed
        sys.path.insert(0, os.environ["LINEAR_OPERATOR_REFERENCE"])
    import torch
    from linear_operator import settings
    from linear_operator.operators import AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator

    from linear_operator_amd import covariance

    torch.set_default_dtype(torch.float32)
    for p, (family, B, n, D, T, ard, seed) in CASES.items():
        x = inputs(p)
        fn = covariance.TASK_FAMILIES[family + "_task"]
        out = {}
        counts = [np.bincount(x["x"][b, :, D].astype(np.int64), minlength=T) for b in range(B)]
        assert all(c.min() > 0 and len(set(c.tolist())) == T for c in counts), f"{p}: task counts {counts}"

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

        def task_op(t):
            return KernelLinearOperator(t["x"], t["x"], fn, num_nonbatch_dimensions={"outputscale": 0},
                                        lengthscale=t["lengthscale"], outputscale=t["outputscale"],
                                        task_covar=t["task_covar"])

        def dense(t):
            return fn(t["x"], t["x"], t["lengthscale"], t["outputscale"], t["task_covar"])

        t32, t64 = tensors(torch.float32), tensors(torch.float64)
        K64 = dense(t64)
        A64 = K64 + torch.diag_embed(t64["noise"])
        assert float(torch.linalg.eigvalsh(t64["task_covar"]).min()) > 0.05, f"{p}: task_covar is not safely positive definite"
        out["cond"] = float(torch.linalg.cond(A64).max())
        op = task_op(t32)
        put("mv", op @ t32["V"], K64 @ t64["V"])
        put("diag", op.diagonal(dim1=-1, dim2=-2), K64.diagonal(dim1=-1, dim2=-2))
        with solver_settings(settings):
            sol = AddedDiagLinearOperator(op, DiagLinearOperator(t32["noise"])).solve(t32["rhs"])
        put("solve", sol, torch.linalg.solve(A64, t64["rhs"]))
        # pivoted Cholesky: float32 and float64 runs of the reference, and the replay's gaps
        L32, piv32 = op.pivoted_cholesky(RANK, return_pivots=True)
        L64, piv64 = task_op(t64).pivoted_cholesky(RANK, return_pivots=True)
        assert torch.equal(piv32[..., :RANK], piv64[..., :RANK]), f"{p}: float32 and float64 pivots differ"
        for b in range(B):
            piv, gaps = pivot_gaps(K64[b].numpy(), RANK)
            assert np.array_equal(piv, piv64[b, :RANK].numpy()), f"{p}[{b}]: the replay's pivots differ"
            bad = [(m, gp) for m, gp in enumerate(gaps) if 1e-12 < gp <= PIVOT_GAP]
            assert not bad, f"{p}[{b}]: near-tied pivot candidates {bad}"
            # step 0: the points of the task with the largest task_covar[t, t] tie exactly, the first of them wins
            best = int(np.argmax(x["task_covar"][b].diagonal()))
            first = int(np.argmax(x["x"][b, :, D].astype(np.int64) == best))
            assert gaps[0] <= 1e-12 and piv[0] == first, f"{p}[{b}]: step 0"
        put("L", L32, L64)
        out["piv"] = piv32[..., :RANK].numpy()
        # gradients of inv_quad
        g32 = tensors(torch.float32, grad=True)
        with solver_settings(settings):
            iq = AddedDiagLinearOperator(task_op(g32), DiagLinearOperator(g32["noise"])).inv_quad(g32["rhs"])
        iq.sum().backward()
        g64 = tensors(torch.float64, grad=True)
        k = dense(g64) + torch.diag_embed(g64["noise"])
        (g64["rhs"] * torch.linalg.solve(k, g64["rhs"])).sum().backward()
        put("iq", iq, (t64["rhs"] * torch.linalg.solve(A64, t64["rhs"])).sum((-2, -1)))
        put("gl", g32["lengthscale"].grad, g64["lengthscale"].grad)
        put("go", g32["outputscale"].grad, g64["outputscale"].grad)
        put("gx", g32["x"].grad, g64["x"].grad)
        put("gB", g32["task_covar"].grad, g64["task_covar"].grad)
        assert not g32["x"].grad[..., D].any() and not g64["x"].grad[..., D].any(), f"{p}: the task column has a gradient"

        # logdet with injected probes
        def probed(t):
            class Probed(AddedDiagLinearOperator):
                def _probe_vectors_and_norms(self):
                    nrm = t["Z"].norm(dim=-2, keepdim=True)
                    return t["Z"] / nrm, nrm

            return Probed(task_op(t), DiagLinearOperator(t["noise"]))

        with solver_settings(settings), settings.num_trace_samples(PROBES):
            _, ld32 = probed(t32).inv_quad_logdet(t32["rhs"], logdet=True)
            _, ld64 = probed(t64).inv_quad_logdet(t64["rhs"], logdet=True)
        put("ld", ld32, ld64)
        out["ld_dense64"] = torch.logdet(A64).numpy()
        print(p, f"cond {out['cond']:.1f}", " ".join(f"{k[:-4]} {out[k]:.2e}" for k in sorted(out) if k.endswith("_err")),
              "ld", out["ld"], out["ld_dense64"])
        path = os.path.join(HERE, f"g43_kernel_task_{p}.npz")
        np.savez_compressed(path, **out)
        print("  ->", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
