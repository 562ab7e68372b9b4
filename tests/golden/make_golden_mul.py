#!/usr/bin/env python3
"""Generate the golden vectors tests/golden/g30_mul_*.npz of `mul`, `prod`, MulLinearOperator and
ConstantMulLinearOperator by running the REAL reference.

Runs only where the reference is importable (like make_golden_ski.py); only the .npz outputs are committed.  Inputs
come from mul_inputs() below (numpy PCG64, seeded) and the operator cases from mul_routing_cases(); the tests call
both with this package's operators.
Usage:  python tests/golden/make_golden_mul.py [path of the reference checkout]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MV_RANKS = ((1, 1), (7, 5), (32, 32), (100, 60))


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def normal(seed, *shape, scale=1.0):
    return (scale * rng(seed).standard_normal(shape)).astype(np.float32)


def mul_inputs():
    """Every input of the fixtures, by name (the tests call this too)."""
    d = {}
    for p, q in MV_RANKS:
        k = f"mv{p}x{q}"
        d[k + "_F"] = normal(3000 + p, 2, 203, p, scale=p ** -0.5)
        d[k + "_G"] = normal(3100 + q, 2, 203, q, scale=q ** -0.5)
        for t in (1, 17):
            d[f"{k}_rhs{t}"] = normal(3200 + p + t, 2, 203, t)
    d["cm_K"] = normal(3301, 2, 40, 40)
    d["cm_K1"] = normal(3302, 2, 5, 5)
    d["cm_K2"] = normal(3303, 2, 8, 8)
    d["cm_R"] = normal(3304, 2, 40, 6)
    d["cm_c"] = np.array([1.7, 0.3], np.float32)
    d["cm_rhs"] = normal(3305, 2, 40, 3)
    d["ix_rows"] = np.array([0, 5, 202, 42, 7], np.int64)
    d["ix_cols"] = np.array([3, 5, 0, 77, 7], np.int64)
    d["ix_batch"] = np.array([0, 1, 1, 0, 1], np.int64)
    d["pc_F"] = normal(3401, 2, 300, 8)
    d["pc_G"] = normal(3402, 2, 300, 6)
    d["pr2_R"] = normal(3501, 2, 24, 5)
    d["pr4_R"] = normal(3502, 4, 24, 5)
    d["so_F"] = normal(3601, 2, 2048, 8, scale=8 ** -0.5)
    d["so_G"] = normal(3602, 2, 2048, 6, scale=6 ** -0.5)
    d["so_c"] = np.array(1.3, np.float32)
    d["so_d"] = (0.5 + 0.5 * rng(3603).random((2, 2048))).astype(np.float32)
    d["so_rhs"] = normal(3604, 2, 2048, 2)
    d["so_Z"] = normal(3605, 2, 2048, 6)
    d["rt_R"] = normal(3701, 2, 16, 3)
    d["rt_S"] = normal(3702, 2, 16, 4)
    d["rt_K"] = normal(3703, 2, 16, 16)
    d["rt_d"] = (1.0 + rng(3704).random((2, 16))).astype(np.float32)
    d["rt_c"] = normal(3705, 2, 1, 1)
    return d


def mul_routing_cases(ops, torch, x):
    """(name, thunk) pairs: each thunk builds operators from `ops` (a module with the operator classes) and calls the
    routing under test; the fixture records the class name of the result (or the name of the exception)."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    R, S, Kd, dg, c = T(x["rt_R"]), T(x["rt_S"]), T(x["rt_K"]), T(x["rt_d"]), T(x["rt_c"])
    Ksym = Kd @ Kd.mT
    K1, K2 = T(x["cm_K1"])[:, :4, :4], T(x["cm_K2"])[:, :4, :4]
    K1, K2 = K1 @ K1.mT, K2 @ K2.mT
    make = {
        "dense": lambda: ops.DenseLinearOperator(Ksym),
        "diag": lambda: ops.DiagLinearOperator(dg),
        "constdiag": lambda: ops.ConstantDiagLinearOperator(dg[..., :1], diag_shape=16),
        "root": lambda: ops.RootLinearOperator(R),
        "lowrankroot": lambda: ops.LowRankRootLinearOperator(R),
        "kron": lambda: ops.KroneckerProductLinearOperator(ops.DenseLinearOperator(K1), ops.DenseLinearOperator(K2)),
        "kron_diag": lambda: ops.KroneckerProductDiagLinearOperator(ops.DiagLinearOperator(dg[..., :4]),
                                                                    ops.DiagLinearOperator(dg[..., 4:8])),
        "added_diag": lambda: ops.AddedDiagLinearOperator(ops.RootLinearOperator(R), ops.DiagLinearOperator(dg)),
        "sum": lambda: ops.SumLinearOperator(ops.RootLinearOperator(R), ops.RootLinearOperator(S)),
        "mul": lambda: ops.MulLinearOperator(ops.RootLinearOperator(R), ops.RootLinearOperator(S)),
        "constmul": lambda: ops.ConstantMulLinearOperator(ops.RootLinearOperator(R), T(np.array([2.0, 3.0], np.float32))),
        "lowrank_added_diag": lambda: ops.LowRankRootLinearOperator(R).add_diagonal(dg),
    }
    cases = []
    for name, mk in make.items():
        cases.append((f"{name}*2.0", lambda mk=mk: mk() * 2.0))
        cases.append((f"{name}*-1.5", lambda mk=mk: mk() * -1.5))
        cases.append((f"torch.mul({name},c)", lambda mk=mk: torch.mul(mk(), c)))
        cases.append((f"{name}/4", lambda mk=mk: mk() / 4.0))
        cases.append((f"{name}.mul(root)", lambda mk=mk: mk().mul(ops.RootLinearOperator(S))))
        cases.append((f"{name}.mul(dense)", lambda mk=mk: mk().mul(Ksym)))
        cases.append((f"{name}.mul(bad)", lambda mk=mk: mk().mul(torch.ones(3, 5, 5))))
    cases.append(("root.prod(-3)", lambda: ops.RootLinearOperator(R).prod(-3)))
    cases.append(("diag.prod(-3)", lambda: ops.DiagLinearOperator(dg).prod(-3)))
    cases.append(("root.prod(-1)", lambda: ops.RootLinearOperator(R).prod(-1)))
    return cases


def run_routing(ops, torch, x):
    names = []
    for name, thunk in mul_routing_cases(ops, torch, x):
        try:
            names.append(f"{name}={type(thunk()).__name__}")
        except Exception as e:  # noqa: BLE001 -- the class of the error is part of the fixture
            names.append(f"{name}=raise:{type(e).__name__}")
    return names


def main():
    if len(sys.argv) > 1:  # a checkout of the reference that is not installed
        sys.path.insert(0, sys.argv[1])
    import torch
    import linear_operator.operators as ops
    from linear_operator import settings
    from linear_operator.functions import pivoted_cholesky
    from linear_operator.operators import (AddedDiagLinearOperator, ConstantMulLinearOperator, DenseLinearOperator,
                                           DiagLinearOperator, KroneckerProductLinearOperator, MulLinearOperator,
                                           RootLinearOperator)

    torch.set_default_dtype(torch.float32)
    torch.set_num_threads(1)  # (bitwise reproducible CPU reductions)
    x = mul_inputs()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    out = {}
    for p, q in MV_RANKS:
        k = f"mv{p}x{q}"
        A = MulLinearOperator(RootLinearOperator(T(x[k + "_F"])), RootLinearOperator(T(x[k + "_G"])))
        for t in (1, 17):
            out[f"{k}_y{t}"] = A._matmul(T(x[f"{k}_rhs{t}"]))
    c, rhs = T(x["cm_c"]), T(x["cm_rhs"])
    bases = {"dense": DenseLinearOperator(T(x["cm_K"])),
             "kron": KroneckerProductLinearOperator(DenseLinearOperator(T(x["cm_K1"])),
                                                    DenseLinearOperator(T(x["cm_K2"]))),
             "root": RootLinearOperator(T(x["cm_R"]))}
    for name, base in bases.items():
        out[f"cm_{name}_y"] = ConstantMulLinearOperator(base, c)._matmul(rhs)
        out[f"cm_{name}_y_scalar"] = ConstantMulLinearOperator(base, c[0])._matmul(rhs)
    A = MulLinearOperator(RootLinearOperator(T(x["mv7x5_F"])), RootLinearOperator(T(x["mv7x5_G"])))
    out["ix_diag"] = A._diagonal()
    out["ix_vals"] = A._get_indices(T(x["ix_rows"]), T(x["ix_cols"]), T(x["ix_batch"]))
    A = MulLinearOperator(RootLinearOperator(T(x["pc_F"])), RootLinearOperator(T(x["pc_G"])))
    out["pc_L"], out["pc_piv"] = pivoted_cholesky(A, 12, error_tol=1e-8, return_pivots=True)
    for k in ("pr2", "pr4"):
        out[k + "_dense"] = RootLinearOperator(T(x[k + "_R"])).prod(-3).to_dense()
    # AddedDiag(c Mul(Root(F), Root(G)), Diag(d)) at N = 2048 (preconditioned): solve, inv_quad_logdet, gradients
    Z = T(x["so_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    with settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6):
        F, G, cc, dd = (T(x["so_" + k]) for k in ("F", "G", "c", "d"))
        A = AddedDiagLinearOperator(MulLinearOperator(RootLinearOperator(F), RootLinearOperator(G)).mul(cc),
                                    DiagLinearOperator(dd))
        out["so_solve"] = A.solve(T(x["so_rhs"]))
        Fg, Gg, cg, dg = (t.clone().requires_grad_(True) for t in (F, G, cc, dd))
        A = Probed(MulLinearOperator(RootLinearOperator(Fg), RootLinearOperator(Gg)).mul(cg), DiagLinearOperator(dg))
        iq, ld = A.inv_quad_logdet(T(x["so_rhs"]), logdet=True)
        (iq.sum() + ld.sum()).backward()
        out["so_iq"], out["so_ld"] = iq, ld
        out["so_dF"], out["so_dG"], out["so_dc"], out["so_dd"] = Fg.grad, Gg.grad, cg.grad, dg.grad
    out["rt_names"] = np.array(run_routing(ops, torch, x))
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}
    groups = {"g30_mul_matvec": ("mv", "cm_", "ix_"), "g30_mul_pivchol": ("pc_", "pr"), "g30_mul_solve": ("so_",),
              "g30_mul_routing": ("rt_",)}
    for name, pre in groups.items():
        sel = {k: v for k, v in out.items() if k.startswith(pre)}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **sel)
        print(name, sorted(sel))


if __name__ == "__main__":
    main()
