#!/usr/bin/env python3
"""Generate the additive SKI golden vectors tests/golden/g45_ski_sum_*.npz by running the REAL reference:
SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator)), the additive KISS-GP model.

Runs only where the reference is importable (pass its directory as the first argument, or set LO_REFERENCE); only the
.npz outputs are committed.  Inputs come from tests/ski_sum_cases.py (seeded): the tests rebuild them from there.
Usage:  python tests/golden/make_golden_ski_sum.py <directory of the reference>

Fixture sizes: no file is larger than g29_ski_solve.npz.  to_dense() is therefore kept at DENSE_ROWS rows per member
and the interpolation-value gradients of the solve case at every GRAD_ROW_STEP-th row (ski_sum_cases.py).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ski_sum_cases as S  # noqa: E402

PIVOT_GAP = 1e-4  # relative gap every float64 pivot step must show, so that float32 rounding cannot change a pivot


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("LO_REFERENCE")
    if ref:
        sys.path.insert(0, ref)
    import torch
    from linear_operator import settings
    from linear_operator.functions import pivoted_cholesky
    from linear_operator.operators import (AddedDiagLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
                                           SumBatchLinearOperator, ToeplitzLinearOperator)

    torch.set_default_dtype(torch.float32)
    x = S.ski_sum_inputs()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731

    def op(col, li, lv, ri, rv):
        return SumBatchLinearOperator(InterpolatedLinearOperator(ToeplitzLinearOperator(col), li, lv, ri, rv))

    files = {}
    for name in ("a", "b"):
        out = {}
        A = op(*(T(x[f"{name}_{k}"]) for k in ("col", "li", "lv", "ri", "rv")))
        for c in S.COLS:
            out[f"matmul{c}"] = A.matmul(T(x[f"{name}_rhs{c}"]))
        N = S.SHAPES[name][2]
        out["dense_rows"] = A.to_dense()[..., torch.from_numpy(S.dense_rows(N)), :]
        out["diag"] = A._diagonal()
        files["g45_ski_sum_" + name] = out
        # pivoted Cholesky of the symmetric operator (W_r = W_l), pivots checked in float64
        pc = {}
        col, li, lv = x[f"p{name}_col"], x[f"p{name}_li"], x[f"p{name}_lv"]
        Ap = op(T(col), T(li), T(lv), T(li), T(lv))
        L, piv = pivoted_cholesky(Ap, S.PIVCHOL_RANK, error_tol=S.PIVCHOL_TOL, return_pivots=True)
        A64 = op(T(col).double(), T(li), T(lv).double(), T(li), T(lv).double())
        L64, piv64 = pivoted_cholesky(A64, S.PIVCHOL_RANK, error_tol=S.PIVCHOL_TOL, return_pivots=True)
        m = L.shape[-1]
        assert L64.shape[-1] == m and torch.equal(piv[..., :m], piv64[..., :m]), "float32 and float64 pivots differ"
        K64 = S.dense64(col, li, lv, li, lv)
        for b in range(K64.shape[0]):
            p64, gaps = S.pivoted_cholesky64(K64[b], m)
            assert np.array_equal(p64, piv64[b, :m].numpy()), (name, b, p64, piv64[b, :m])
            assert gaps.min() > PIVOT_GAP, f"{name} member {b}: pivot gap {gaps.min():.2e}: pick another seed"
            print(f"pivchol {name} member {b}: smallest relative pivot gap {gaps.min():.2e}")
        pc["L"], pc["piv"], pc["diag"] = L, piv, Ap._diagonal()
        files["g45_ski_sum_pivchol_" + name] = pc

    # AddedDiag(SumBatch(...), Diag) at N = 2048 (preconditioned): solve, inv_quad_logdet, gradients; probes fixed the
    # way g29_ski_solve fixes them
    Z = T(x["big_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    sol, grads = {}, {}
    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6):
        col, dd, lv, li = T(x["big_col"]), T(x["big_d"]), T(x["big_lv"]), T(x["big_li"])
        A = AddedDiagLinearOperator(op(col, li, lv, li, lv), DiagLinearOperator(dd))
        sol["solve"] = A.solve(T(x["big_rhs"]))
        dense = S.dense64(x["big_col"], x["big_li"], x["big_lv"], x["big_li"], x["big_lv"])
        dense += np.stack([np.diag(r) for r in x["big_d"].astype(np.float64)])
        exact = np.linalg.solve(dense, x["big_rhs"].astype(np.float64))
        print("solve against the float64 dense solve:", np.abs(sol["solve"].numpy() - exact).max() / np.abs(exact).max())
        colg, ddg, lvl, lvr = (t.clone().requires_grad_(True) for t in (col, dd, lv, lv))
        A = Probed(op(colg, li, lvl, li, lvr), DiagLinearOperator(ddg))
        iq, ld = A.inv_quad_logdet(T(x["big_rhs"]), logdet=True)
        (iq.sum() + ld.sum()).backward()
        sol["iq"], sol["ld"], sol["dcol"], sol["dd"] = iq, ld, colg.grad, ddg.grad
        grads["dlv"], grads["drv"] = lvl.grad[..., ::S.GRAD_ROW_STEP, :], lvr.grad[..., ::S.GRAD_ROW_STEP, :]
    files["g45_ski_sum_solve"], files["g45_ski_sum_grads"] = sol, grads

    limit = os.path.getsize(os.path.join(HERE, "g29_ski_solve.npz"))
    for fname, out in files.items():
        out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
        path = os.path.join(HERE, fname + ".npz")
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        print(fname, sorted(out), size)
        assert size <= limit, (fname, size, limit)


if __name__ == "__main__":
    main()
