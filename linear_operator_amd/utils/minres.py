"""minres with the reference's signature and semantics (linear_operator/utils/minres.py:10-207), executed by
liblo_amd's shifted-MINRES engine (csrc/lo_minres.hip).  Closure handling is the one of utils/linear_cg.py: operator
`_matmul`s that lower to a kernel descriptor run entirely on the device, other callables are called back for the
product only; the Woodbury preconditioner closure of AddedDiagLinearOperator is applied natively.  HIP tensors only --
there is no CPU implementation; float64 operands (the reference's own test recipes) take csrc/lo_minres_f64.hip."""
from __future__ import annotations

import torch

from .. import kernels as K
from .. import settings
# (_lower_f64: tests/test_gpu_f64_desc.py switches the lowering off in every front end)
from .linear_cg import _f32_precond, _f64_operands, _lower_f64, _lower_matmul_closure  # noqa: F401


def minres(matmul_closure, rhs, eps=1e-25, shifts=None, value=None, max_iter=None, preconditioner=None):
    r"""Solutions of :math:`(\alpha K + \sigma_q I) x_q = b` for all shifts :math:`\sigma_q` at once (``value`` is
    :math:`\alpha`).  Returns ``[Q, *batch, N, c]`` -- without the leading dimension when there is a single shift."""
    if not torch.is_tensor(matmul_closure) and not callable(matmul_closure):
        raise RuntimeError("matmul_closure must be a tensor, or a callable object!")
    if shifts is None:  # :43-44
        shifts = torch.tensor(0.0, dtype=rhs.dtype, device=rhs.device)
    squeeze = rhs.dim() == 1  # :47-50
    if squeeze:
        rhs = rhs.unsqueeze(-1)
    if max_iter is None:  # :58-60
        max_iter = settings.max_cg_iterations.value()
    max_iter = min(max_iter, rhs.size(-2) + 1)

    # batch shape of the products (the reference learns it from one product, :64)
    owner = getattr(matmul_closure, "__self__", None)
    if torch.is_tensor(matmul_closure):
        op_batch = matmul_closure.shape[:-2]
    elif owner is not None and hasattr(owner, "batch_shape"):
        op_batch = owner.batch_shape
    else:
        op_batch = matmul_closure(rhs).shape[:-2]
    batch_shape = torch.broadcast_shapes(op_batch, rhs.shape[:-2])
    rhs_b = rhs.expand(*batch_shape, *rhs.shape[-2:]).contiguous()

    sh = shifts.reshape(1) if shifts.dim() == 0 else shifts
    if rhs.dtype == torch.float64:
        # the reference's fp64 recipes (test/utils/test_minres.py), operands by _f64_operands (csrc/lo_minres_f64.hip)
        dense, operands = _f64_operands(matmul_closure, preconditioner, batch_shape, rhs_b.shape[-1], rhs_b.is_cuda)
        res = K.minres_solve_f64(
            dense, rhs_b, sh, value=value, **operands, max_iter=max_iter,
            tolerance=float(settings.minres_tolerance.value()), eps=float(eps),
        )
    else:
        desc = _lower_matmul_closure(matmul_closure, batch_shape)
        closure = None
        if desc is None:
            closure = matmul_closure.matmul if torch.is_tensor(matmul_closure) else matmul_closure
        woodbury, precond_closure = _f32_precond(preconditioner, batch_shape)
        if settings.verbose_linalg.on():
            settings.verbose_linalg.logger.debug(
                f"Running MINRES on a {rhs.shape} RHS for {max_iter} iterations "
                f"(tol={settings.minres_tolerance.value()}). Output: {(sh.shape[0], *rhs_b.shape)}."
            )
        res = K.minres_solve(
            desc, rhs_b, sh, value=value, precond=woodbury, matvec_closure=closure, precond_closure=precond_closure,
            max_iter=max_iter, tolerance=float(settings.minres_tolerance.value()), eps=float(eps),
        )
    solution = res.x
    if squeeze:  # :203-206
        solution = solution.squeeze(-1)
    if shifts.numel() == 1:  # :208-210
        solution = solution.squeeze(0)
    return solution


__all__ = ["minres"]
