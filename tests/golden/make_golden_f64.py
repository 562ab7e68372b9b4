#!/usr/bin/env python3
"""Generate tests/golden/g34_fp64_structured.npz: the REAL reference's float64 solvers on structured operators, on the CPU.

Runs only where the reference is importable (like make_golden_masked.py); only the .npz output is committed.  The
inputs come from f64_inputs() below (generators of cases.py with dtype=np.float64); the tests call it and build the same
operators from this package.  Three cases, each a batch of two members:
  lowrank   LowRankRoot(C [600, 8]) + Diag(d)
  kron      Kron(K1 [12, 12], K2 [25, 25]) + sigma^2 I          (constant diagonal)
  sum       LowRankRoot(C [300, 4]) + Dense(K [300, 300]) + Diag(d)
For every case: linear_cg with the reference's pivoted-Cholesky preconditioner closure, n_tridiag = 2 (x_*, t_*), the
number of products it asked for (matvecs_*; iterations = matvecs - 1) and the cached pair (Q_*, noise_*) the closure was
made of, so that the oracle and the kernels apply the very same preconditioner.  Shifted MINRES (3 shifts) on the
Kronecker case and lanczos_tridiag (4 start vectors, 12 steps) on the low-rank case.
The iteration count is decided by convergence, not by a floor, in the Kronecker (19 iterations) and sum (16) cases:
the preconditioner has rank PRECOND_RANK = 3, below every root's rank, and the tridiagonals stop at 8 steps, so the
reference's stop rule is free from iteration 10 on; the low-rank case (rank 8 root) converges before that and ends on the
floor of 11 with a 7 x 7 tridiagonal taken along the recurrence.
The members are well conditioned (sigma^2 = 1 on the Kronecker case): with sigma^2 = 0.1 the reference's CG took 49
iterations and two correct float64 implementations -- the reference and the numpy oracle -- already differed by 2e-7 in
the solution, so a 1e-9 comparison would have measured the rounding of the recurrence, not the operator.
Usage:  python tests/golden/make_golden_f64.py [path of the reference checkout]
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cases  # noqa: E402

CASES = ("lowrank", "kron", "sum")
CG = dict(n_tridiag=2, tolerance=1e-5, max_iter=300, max_tridiag_iter=8)
PRECOND_RANK = 3
MINRES_SHIFTS = np.array([0.1, 1.0, 10.0])
MINRES_TOL = 1e-6
LANCZOS_STEPS = 12


def f64_inputs(case):
    """The float64 tensors of one case by name."""
    d = {}
    if case == "lowrank":
        d["C"], d["d"], d["rhs"] = cases.lowrank_diag(3401, 2, 600, 8, 3, dtype=np.float64)
        d["init"] = cases.randn(3402, 2, 600, 4, dtype=np.float64)  # Lanczos start vectors
    elif case == "kron":
        d["K1"], d["K2"], d["sigma2"], d["rhs"] = cases.kron_factors(3411, 2, 12, 25, 3, sigma=1.0, dtype=np.float64)
    else:
        d["C"], d["d"], d["rhs"] = cases.lowrank_diag(3421, 2, 300, 4, 3, dtype=np.float64)
        d["K"], _, _ = cases.dense_diag(3422, 2, 300, 1, dtype=np.float64)
    return d


def build(ops, case, t):
    """(operator without its diagonal, its diagonal operator) of a case from tensors `t`, with the classes of `ops`."""
    if case == "lowrank":
        return ops.LowRankRootLinearOperator(t["C"]), ops.DiagLinearOperator(t["d"])
    if case == "kron":
        n = t["K1"].shape[-1] * t["K2"].shape[-1]
        return (ops.KroneckerProductLinearOperator(ops.DenseLinearOperator(t["K1"]), ops.DenseLinearOperator(t["K2"])),
                ops.ConstantDiagLinearOperator(t["sigma2"], diag_shape=n))
    return (ops.SumLinearOperator(ops.LowRankRootLinearOperator(t["C"]), ops.DenseLinearOperator(t["K"])),
            ops.DiagLinearOperator(t["d"]))


def main():
    if len(sys.argv) > 1:  # a checkout of the reference that is not installed
        sys.path.insert(0, sys.argv[1])
    import torch
    import linear_operator.operators as ops
    from linear_operator import settings
    from linear_operator.utils.lanczos import lanczos_tridiag
    from linear_operator.utils.linear_cg import linear_cg
    from linear_operator.utils.minres import minres

    out = {}
    for case in CASES:
        t = {k: torch.from_numpy(v) for k, v in f64_inputs(case).items()}
        base, diag = build(ops, case, t)
        A = ops.AddedDiagLinearOperator(base, diag)
        calls = [0]

        def matmul(v, A=A, calls=calls):
            calls[0] += 1
            return A._matmul(v)

        with settings.min_preconditioning_size(100), settings.max_preconditioner_size(PRECOND_RANK):
            closure, _, _ = A._preconditioner()
            assert closure is not None
            x, tm = linear_cg(matmul, t["rhs"], preconditioner=closure, **CG)
        exact = torch.linalg.solve(A.to_dense(), t["rhs"])
        assert float((x - exact).norm() / exact.norm()) < 1e-4, case
        out[f"x_{case}"], out[f"t_{case}"], out[f"matvecs_{case}"] = x.numpy(), tm.numpy(), np.int64(calls[0])
        out[f"Q_{case}"] = A._q_cache.numpy()
        out[f"noise_{case}"] = A._noise.numpy()[..., 0]  # [2, N] or [2, 1]
        out[f"constant_{case}"] = np.bool_(A._constant_diag)
        assert calls[0] - 1 < CG["max_iter"], case
        if case == "kron":
            with settings.minres_tolerance(MINRES_TOL):
                out["x_minres"] = minres(A._matmul, t["rhs"], shifts=torch.from_numpy(MINRES_SHIFTS)).numpy()
        if case == "lowrank":
            q, tl = lanczos_tridiag(A._matmul, LANCZOS_STEPS, dtype=torch.float64, device=torch.device("cpu"),
                                    matrix_shape=A.shape[-2:], batch_shape=A.batch_shape, init_vecs=t["init"])
            out["lanczos_t"], out["lanczos_q0"] = tl.numpy(), q[0].numpy()  # (q of the first start vector only: size)
    path = os.path.join(HERE, "g34_fp64_structured.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), {k: getattr(v, "shape", None) for k, v in out.items()})


if __name__ == "__main__":
    main()
