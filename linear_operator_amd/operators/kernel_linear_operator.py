"""KernelLinearOperator: the covariance matrix K(x1, x2) of a kernel function held as its inputs -- the points and the
hyperparameters, N D numbers instead of N^2 (the reference's operators/kernel_linear_operator.py, same constructor and
results).  `covar_func(x1, x2, **params)` may be any callable; it is evaluated densely whenever the matrix itself is
needed (the general path, as in the reference, on any device and in any dtype).

Native path.  When `covar_func` carries a `native_family` (linear_operator_amd.covariance: rbf, matern12, matern32,
matern52), there is one output per input, the tensors are float32 on the device, D <= LO_KERNEL_MAX_DIM and the
parameters are exactly `lengthscale` [*b, 1, D] or [*b, 1, 1] and `outputscale` [*b], the matrix is NEVER formed:

  _matmul / _t_matmul   the on-the-fly product lo_kernel_mv_f32 (csrc/lo_kernel_op.hip), rectangular x1 / x2 included
  _kernel_descriptor    x1 and x2 the same points: the kind LO_OP_KERNEL_DIAG, so that AddedDiag(Kernel, Diag) runs CG,
                        Lanczos, MINRES and the pivoted Cholesky on the device with no Python call per iteration
  _diagonal             outputscale^2, no launch;  _get_indices / _get_rows evaluate only the requested entries
  _bilinear_derivative  lengthscale and outputscale from lo_kernel_bilinear_f32; the points' gradients, when asked for,
                        from lo_kernel_points_grad_f32: one call per side that needs one, the x2 side as the x1 side of
                        the transposed problem.  covar_func is not called and nothing of size M N is allocated

Gradient kernels.  `covariance.rbf_grad` (`native_outputs == "grad"`) with num_outputs_per_input = (D + 1, D + 1), D <=
LO_KERNEL_GRAD_MAX_DIM and the same parameters has a gate of its own, `_native_grad_refusal`; `_native_refusal` keeps
answering "more than one output per input", so every caller that assumes one output per input stays out.  Inside it:

  _matmul / _t_matmul   lo_kernel_grad_mv_f32 (csrc/lo_kernel_grad.hip), always: its purpose is memory
  _kernel_descriptor    x1 and x2 the same points: the kind LO_OP_KERNEL_GRAD_DIAG
  _diagonal             outputscale^2 (1, 1 / l_1^2, .., 1 / l_D^2) per point, no launch, no covar_func
  _bilinear_derivative  lo_kernel_grad_bilinear_f32 when neither points tensor asks for a gradient (else the general path)
  _getitem              slices of whole points rebuild the operator over the sliced points; anything else indexes densely

Task-indexed multitask kernels.  `covariance.rbf_task` .. `matern52_task` (`native_outputs == "task"`): the points carry
the task id of the observation in their last column, the parameters are `lengthscale`, `outputscale` and `task_covar`
[*b, T, T], T <= LO_KERNEL_TASK_MAX_TASKS, and K_ij = outputscale^2 g(r_ij) task_covar[t_i, t_j].  The gate is
`_native_task_refusal`; `_native_refusal` keeps answering "parameters other than lengthscale and outputscale", so the
Sum and Kronecker fusion gates never take such an operator.  Inside it:

  _matmul / _t_matmul   lo_kernel_task_mv_f32 (csrc/lo_kernel_task.hip), always, rectangular included: its purpose is memory
  _kernel_descriptor    x1 and x2 the same points: the kind LO_OP_KERNEL_TASK_DIAG
  _diagonal             outputscale^2 task_covar[t_i, t_i] by a gather, no covar_func
  _bilinear_derivative  lengthscale, outputscale and task_covar from lo_kernel_task_bilinear_f32, the points' gradients
                        from lo_kernel_task_points_grad_f32 (the task column's gradient is 0)

The operator treats task_covar as symmetric: `_transpose_nonbatch` swaps the points and keeps the parameters, as it does
for any covar_func.  Ids outside [0, T) are the caller's error: the gate does not synchronise to look, the kernels clamp.

Families with a shape parameter.  `covariance.rq` (parameters `lengthscale`, `outputscale`, `alpha` [*b]) and
`covariance.periodic` (`lengthscale`, `outputscale`, `period_length` [*b, 1, D] or [*b, 1, 1]) carry `native_outputs ==
"param"` and family codes outside those of the four families above; D <= LO_KERNEL_PARAM_MAX_DIM.  The gate is
`_native_param_refusal`; `_native_refusal` keeps answering "parameters other than lengthscale and outputscale", so the Sum,
Kronecker and LMC fusion gates never take such an operator.  Inside it:

  _matmul / _t_matmul   lo_kernel_param_mv_f32 (csrc/lo_kernel_param.hip), always, rectangular included: its purpose is memory
  _kernel_descriptor    x1 and x2 the same points: the kind LO_OP_KERNEL_PARAM_DIAG, also a term of a lowered sum
                        (periodic + rbf + noise is one LO_OP_SUM)
  _diagonal             outputscale^2, no launch
  _bilinear_derivative  lengthscale, outputscale and alpha or period_length from lo_kernel_param_bilinear_f32 (d l = -theta^2
                        d theta, d os = 2 os d os^2, d p = -nu^2 d nu, a shared l or p summed over D), the points' gradients
                        from lo_kernel_param_points_grad_f32.  covar_func is not called, nothing of size M N is allocated

Float64.  The four one-output families with every tensor float64 on the device have a gate of their own,
`_native_f64_refusal` (the conditions of `_native_refusal` with float64 in place of float32); `_native_refusal` keeps
answering "not float32", so the fp32 fusion gates of the Sum and Kronecker operators never see such an operator.  Inside it,
with a float64 device right-hand side:

  _matmul / _t_matmul   lo_kernel_mv_f64 (csrc/lo_kernel_op_f64.hip), always, rectangular x1 / x2 included
  _kernel_descriptor_f64  x1 and x2 the same points: the float64 LO_OP_KERNEL_DIAG descriptor, which AddedDiag and Sum
                        lower through (_attach_diag, utils.linear_cg._lower_f64), so that the float64 CG, MINRES and
                        Lanczos multiply by lo_matvec_f64 with no Python call per product.  `_kernel_descriptor()` of the
                        operator on its own stays None for float64, as it always was
  _diagonal             outputscale^2, no launch
  _bilinear_derivative  lo_kernel_bilinear_f64 and lo_kernel_points_grad_f64, the same theta -> lengthscale / outputscale
                        mapping as in float32

Anything outside the gates (D > 32, mixed element types, CPU, several outputs per input of another kind, other
parameters) takes the general path, and so does a float32 right-hand side against a float64 operator or the reverse.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Callable, Optional

import torch
from torch import Tensor

from ._linear_operator import LinearOperator, to_dense

_NOOP = slice(None, None, None)


def _two():
    return 2


def _same_tensor(a: Tensor, b: Tensor) -> bool:
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()
                      and a.dtype == b.dtype and a.device == b.device)


class KernelLinearOperator(LinearOperator):
    def __init__(self, x1: Tensor, x2: Tensor, covar_func: Callable, num_outputs_per_input=(1, 1),
                 num_nonbatch_dimensions: Optional[dict] = None, **params):
        nonbatch = defaultdict(_two)
        if num_nonbatch_dimensions is not None:
            nonbatch.update(num_nonbatch_dimensions)
        tensor_params = {k: v for k, v in params.items() if torch.is_tensor(v)}
        other_params = {k: v for k, v in params.items() if not torch.is_tensor(v)}
        batch_of, tail_of = {}, {}
        for name, val in tensor_params.items():
            nb = nonbatch[name]
            batch_of[name] = val.shape[: val.dim() - nb] if nb else val.shape
            tail_of[name] = val.shape[val.dim() - nb:] if nb else torch.Size([])
        try:
            batch = torch.broadcast_shapes(x1.shape[:-2], x2.shape[:-2], *batch_of.values())
        except RuntimeError:
            try:  # the data alone: batch dimensions and the number of input dimensions
                torch.broadcast_shapes(torch.Size([*x1.shape[:-2], 1, x1.shape[-1]]),
                                       torch.Size([*x2.shape[:-2], 1, x2.shape[-1]]))
            except RuntimeError:
                raise RuntimeError(
                    "Incompatible data shapes for a kernel matrix: "
                    f"x1.shape={tuple(x1.shape)}, x2.shape={tuple(x2.shape)}."
                )
            raise RuntimeError(
                "Shape of kernel parameters "
                f"({', '.join([str(tuple(param.shape)) for param in tensor_params.values()])}) "
                f"is incompatible with data shapes x1.shape={tuple(x1.shape)}, x2.shape={tuple(x2.shape)}.\n"
                "Recall that parameters passed to KernelLinearOperator should have dimensionality compatible "
                "with the data (see documentation)."
            )
        if len(batch):  # every tensor carries the whole batch shape from here on
            same = _same_tensor(x1, x2)
            if x1.shape[:-2] != batch:
                x1 = x1.expand(*batch, *x1.shape[-2:]).contiguous()
            x2 = x1 if same else (x2 if x2.shape[:-2] == batch else x2.expand(*batch, *x2.shape[-2:]).contiguous())
            tensor_params = {name: (val if batch_of[name] == batch else val.expand(*batch, *tail_of[name]))
                             for name, val in tensor_params.items()}
        super().__init__(x1, x2, covar_func=covar_func, num_outputs_per_input=num_outputs_per_input,
                         num_nonbatch_dimensions=nonbatch, **tensor_params, **other_params)
        self.batch_broadcast_shape = torch.Size(batch)
        self.x1, self.x2 = x1, x2
        self.tensor_params, self.nontensor_params = tensor_params, other_params
        self.covar_func = covar_func
        self.num_outputs_per_input = tuple(num_outputs_per_input)
        self.num_nonbatch_dimensions = nonbatch

    def _rebuild(self, x1, x2, tensor_params):
        return self.__class__(x1, x2, covar_func=self.covar_func, num_outputs_per_input=self.num_outputs_per_input,
                              num_nonbatch_dimensions=self.num_nonbatch_dimensions, **tensor_params,
                              **self.nontensor_params)

    # ------------------------------------------------------------------ the gate of the native path
    def _native_refusal(self, check_device: bool = True) -> Optional[str]:
        """None when the native kernels take this operator, else the reason they do not.  `check_device=False` leaves
        out the float32-on-the-device condition (what the rest of the gate decides can then be asked on any machine)."""
        from .. import _hip

        if getattr(self.covar_func, "native_family", None) is None:
            return "covar_func has no native_family"
        if self.num_outputs_per_input != (1, 1):
            return "more than one output per input"
        if self.nontensor_params or set(self.tensor_params) != {"lengthscale", "outputscale"}:
            return "parameters other than lengthscale and outputscale"
        D = self.x1.shape[-1]
        if D > _hip.LO_KERNEL_MAX_DIM or D < 1 or self.x2.shape[-1] != D:
            return f"D = {D} beyond LO_KERNEL_MAX_DIM"
        ls, os_ = self.tensor_params["lengthscale"], self.tensor_params["outputscale"]
        batch = self.batch_broadcast_shape
        if self.num_nonbatch_dimensions["lengthscale"] != 2 or ls.shape not in ((*batch, 1, D), (*batch, 1, 1)):
            return f"lengthscale of shape {tuple(ls.shape)}"
        if self.num_nonbatch_dimensions["outputscale"] != 0 or os_.shape != batch:
            return f"outputscale of shape {tuple(os_.shape)}"
        tensors = (self.x1, self.x2, ls, os_)
        if any(t.dtype != torch.float32 for t in tensors):
            return "not float32"
        if check_device and not all(t.is_cuda for t in tensors):
            return "not on the device"
        return None

    def _is_native(self) -> bool:
        return self._native_refusal() is None

    def _native_grad_refusal(self, check_device: bool = True) -> Optional[str]:
        """The gate of the gradient kernel (D + 1 outputs per input, csrc/lo_kernel_grad.hip): None when the native
        kernels take this operator, else the reason they do not.  `check_device=False` leaves out the device condition."""
        from .. import _hip

        if getattr(self.covar_func, "native_outputs", None) != "grad":
            return "covar_func has no native_outputs == 'grad'"
        if getattr(self.covar_func, "native_family", None) != _hip.LO_KERNEL_RBF:
            return "a gradient kernel of a family other than RBF"
        D = self.x1.shape[-1]
        if D < 1 or self.x2.shape[-1] != D or D > _hip.LO_KERNEL_GRAD_MAX_DIM:
            return f"D = {D} beyond LO_KERNEL_GRAD_MAX_DIM"
        if self.num_outputs_per_input != (D + 1, D + 1):
            return f"num_outputs_per_input is not ({D + 1}, {D + 1})"
        if self.nontensor_params or set(self.tensor_params) != {"lengthscale", "outputscale"}:
            return "parameters other than lengthscale and outputscale"
        ls, os_ = self.tensor_params["lengthscale"], self.tensor_params["outputscale"]
        batch = self.batch_broadcast_shape
        if self.num_nonbatch_dimensions["lengthscale"] != 2 or ls.shape not in ((*batch, 1, D), (*batch, 1, 1)):
            return f"lengthscale of shape {tuple(ls.shape)}"
        if self.num_nonbatch_dimensions["outputscale"] != 0 or os_.shape != batch:
            return f"outputscale of shape {tuple(os_.shape)}"
        tensors = (self.x1, self.x2, ls, os_)
        if any(t.dtype != torch.float32 for t in tensors):
            return "not float32"
        if check_device and not all(t.is_cuda for t in tensors):
            return "not on the device"
        return None

    def _is_native_grad(self) -> bool:
        return self._native_grad_refusal() is None

    def _native_task_refusal(self, check_device: bool = True) -> Optional[str]:
        """The gate of the task-indexed multitask kernels (csrc/lo_kernel_task.hip): None when the native kernels take
        this operator, else the reason they do not.  `check_device=False` leaves out the device condition."""
        from .. import _hip

        if getattr(self.covar_func, "native_outputs", None) != "task":
            return "covar_func has no native_outputs == 'task'"
        if getattr(self.covar_func, "native_family", None) is None:
            return "covar_func has no native_family"
        if self.num_outputs_per_input != (1, 1):
            return "more than one output per input"
        if self.nontensor_params or set(self.tensor_params) != {"lengthscale", "outputscale", "task_covar"}:
            return "parameters other than lengthscale, outputscale and task_covar"
        D = self.x1.shape[-1] - 1
        if D < 1 or self.x2.shape[-1] != D + 1 or D + 1 > _hip.LO_KERNEL_MAX_DIM:
            return f"D = {D} outside 1 .. LO_KERNEL_MAX_DIM - 1"
        ls, os_, Bt = (self.tensor_params[k] for k in ("lengthscale", "outputscale", "task_covar"))
        batch = self.batch_broadcast_shape
        if self.num_nonbatch_dimensions["lengthscale"] != 2 or ls.shape not in ((*batch, 1, D), (*batch, 1, 1)):
            return f"lengthscale of shape {tuple(ls.shape)}"
        if self.num_nonbatch_dimensions["outputscale"] != 0 or os_.shape != batch:
            return f"outputscale of shape {tuple(os_.shape)}"
        T = Bt.shape[-1]
        if self.num_nonbatch_dimensions["task_covar"] != 2 or Bt.shape != (*batch, T, T) or T < 1:
            return f"task_covar of shape {tuple(Bt.shape)}"
        if T > _hip.LO_KERNEL_TASK_MAX_TASKS:
            return f"T = {T} beyond LO_KERNEL_TASK_MAX_TASKS"
        tensors = (self.x1, self.x2, ls, os_, Bt)
        if any(t.dtype != torch.float32 for t in tensors):
            return "not float32"
        if check_device and not all(t.is_cuda for t in tensors):
            return "not on the device"
        return None

    def _is_native_task(self) -> bool:
        return self._native_task_refusal() is None

    def _native_param_refusal(self, check_device: bool = True) -> Optional[str]:
        """The gate of the families with a shape parameter, rational quadratic and periodic (csrc/lo_kernel_param.hip):
        None when the native kernels take this operator, else the reason they do not.  `check_device=False` leaves out
        the device condition."""
        from .. import _hip

        if getattr(self.covar_func, "native_outputs", None) != "param":
            return "covar_func has no native_outputs == 'param'"
        family = getattr(self.covar_func, "native_family", None)
        extra = {_hip.LO_KERNEL_RQ: "alpha", _hip.LO_KERNEL_PERIODIC: "period_length"}.get(family)
        if extra is None:
            return "covar_func has no native_family among LO_KERNEL_RQ, LO_KERNEL_PERIODIC"
        if self.num_outputs_per_input != (1, 1):
            return "more than one output per input"
        if self.nontensor_params or set(self.tensor_params) != {"lengthscale", "outputscale", extra}:
            return f"parameters other than lengthscale, outputscale and {extra}"
        D = self.x1.shape[-1]
        if D > _hip.LO_KERNEL_PARAM_MAX_DIM or D < 1 or self.x2.shape[-1] != D:
            return f"D = {D} beyond LO_KERNEL_PARAM_MAX_DIM"
        ls, os_, sh = (self.tensor_params[k] for k in ("lengthscale", "outputscale", extra))
        batch = self.batch_broadcast_shape
        if self.num_nonbatch_dimensions["lengthscale"] != 2 or ls.shape not in ((*batch, 1, D), (*batch, 1, 1)):
            return f"lengthscale of shape {tuple(ls.shape)}"
        if self.num_nonbatch_dimensions["outputscale"] != 0 or os_.shape != batch:
            return f"outputscale of shape {tuple(os_.shape)}"
        if extra == "alpha":
            if self.num_nonbatch_dimensions["alpha"] != 0 or sh.shape != batch:
                return f"alpha of shape {tuple(sh.shape)}"
        elif self.num_nonbatch_dimensions["period_length"] != 2 or sh.shape not in ((*batch, 1, D), (*batch, 1, 1)):
            return f"period_length of shape {tuple(sh.shape)}"
        tensors = (self.x1, self.x2, ls, os_, sh)
        if any(t.dtype != torch.float32 for t in tensors):
            return "not float32"
        if check_device and not all(t.is_cuda for t in tensors):
            return "not on the device"
        return None

    def _is_native_param(self) -> bool:
        return self._native_param_refusal() is None

    def _native_f64_refusal(self, check_device: bool = True) -> Optional[str]:
        """The gate of the float64 kernels (csrc/lo_kernel_op_f64.hip): None when they take this operator, else the
        reason they do not -- the conditions of `_native_refusal` with every tensor float64.  `check_device=False`
        leaves out the device condition."""
        from .. import _hip

        if getattr(self.covar_func, "native_family", None) is None:
            return "covar_func has no native_family"
        if self.num_outputs_per_input != (1, 1):
            return "more than one output per input"
        if self.nontensor_params or set(self.tensor_params) != {"lengthscale", "outputscale"}:
            return "parameters other than lengthscale and outputscale"
        D = self.x1.shape[-1]
        if D > _hip.LO_KERNEL_MAX_DIM or D < 1 or self.x2.shape[-1] != D:
            return f"D = {D} beyond LO_KERNEL_MAX_DIM"
        ls, os_ = self.tensor_params["lengthscale"], self.tensor_params["outputscale"]
        batch = self.batch_broadcast_shape
        if self.num_nonbatch_dimensions["lengthscale"] != 2 or ls.shape not in ((*batch, 1, D), (*batch, 1, 1)):
            return f"lengthscale of shape {tuple(ls.shape)}"
        if self.num_nonbatch_dimensions["outputscale"] != 0 or os_.shape != batch:
            return f"outputscale of shape {tuple(os_.shape)}"
        tensors = (self.x1, self.x2, ls, os_)
        if any(t.dtype != torch.float64 for t in tensors):
            return "not float64"
        if check_device and not all(t.is_cuda for t in tensors):
            return "not on the device"
        return None

    def _is_native_f64(self) -> bool:
        return self._native_f64_refusal() is None

    def _same_points(self) -> bool:
        return _same_tensor(self.x1, self.x2)

    def _theta(self, batch, dtype=torch.float32):
        from .. import kernels as K

        return K.kernel_theta(self.tensor_params["lengthscale"], self.tensor_params["outputscale"], batch,
                              self.x1.shape[-1], dtype=dtype)

    def _task_operands(self, batch):
        """Inside the task gate: theta [B, D + 1] over the D coordinates and task_covar as Bt [B, T, T], for `batch`."""
        from .. import kernels as K

        Bt = self.tensor_params["task_covar"].detach()
        T = Bt.shape[-1]
        theta = K.kernel_theta(self.tensor_params["lengthscale"], self.tensor_params["outputscale"], batch,
                               self.x1.shape[-1] - 1)
        return theta, Bt.expand(*batch, T, T).reshape(-1, T, T)

    def _param_theta(self, batch):
        """Inside the param gate: theta [B, 2 D + 2] for `batch` (kernels.kernel_param_theta)."""
        from .. import kernels as K

        p = self.tensor_params
        return K.kernel_param_theta(p["lengthscale"], p["outputscale"], batch, self.x1.shape[-1], alpha=p.get("alpha"),
                                    period_length=p.get("period_length"))

    def _kernel_descriptor_f64(self, batch_shape=None):
        """The float64 LO_OP_KERNEL_DIAG descriptor inside the float64 gate when x1 and x2 are one tensor, else None."""
        if not (self._is_native_f64() and self._same_points()):
            return None
        from .. import kernels as K

        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        X = self.x1.detach()
        X = X if X.shape[:-2] == bs else X.expand(*bs, *X.shape[-2:])
        return K.kernel_diag_descriptor(X, self._theta(bs, torch.float64), self.covar_func.native_family,
                                        dtype=torch.float64)

    def _kernel_descriptor(self, batch_shape=None):
        grad, task, param = self._is_native_grad(), self._is_native_task(), self._is_native_param()
        if not ((grad or task or param or self._is_native()) and self._same_points()):
            return None
        from .. import kernels as K

        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        X = self.x1.detach()
        X = X if X.shape[:-2] == bs else X.expand(*bs, *X.shape[-2:])
        if task:
            theta, Bt = self._task_operands(bs)
            return K.kernel_task_diag_descriptor(X, theta, self.covar_func.native_family, Bt.reshape(*bs, *Bt.shape[-2:]))
        if param:
            return K.kernel_param_diag_descriptor(X, self._param_theta(bs), self.covar_func.native_family)
        build = K.kernel_grad_diag_descriptor if grad else K.kernel_diag_descriptor
        return build(X, self._theta(bs), self.covar_func.native_family)

    # ------------------------------------------------------------------ dense evaluation (the general path)
    def _dense_covar(self):
        """covar_func on all of x1 and x2: the [*batch, M, N] matrix (or operator).  The native path never calls it."""
        return self.covar_func(self.x1, self.x2, **self.tensor_params, **self.nontensor_params)

    @property
    def covar_mat(self):
        return self._dense_covar()

    def to_dense(self) -> Tensor:
        return to_dense(self._dense_covar())

    # ------------------------------------------------------------------ operator protocol
    def _size(self) -> torch.Size:
        p, q = self.num_outputs_per_input
        return torch.Size([*self.batch_broadcast_shape, self.x1.shape[-2] * p, self.x2.shape[-2] * q])

    def _transpose_nonbatch(self):
        return self._rebuild(self.x2, self.x1, self.tensor_params)

    def _matmul(self, rhs: Tensor) -> Tensor:
        vec = rhs.dim() == 1
        cols = rhs.unsqueeze(-1) if vec else rhs
        if cols.is_cuda and cols.dtype == torch.float32 and self._is_native_grad():
            from .. import kernels as K

            M, D = self.x1.shape[-2:]
            N, c = self.x2.shape[-2], cols.shape[-1]
            bs = torch.broadcast_shapes(self.batch_shape, cols.shape[:-2])
            x1 = self.x1.detach().expand(*bs, M, D).reshape(-1, M, D)
            x2 = x1 if self._same_points() else self.x2.detach().expand(*bs, N, D).reshape(-1, N, D)
            y = K.kernel_grad_mv(x1, x2, self._theta(bs), self.covar_func.native_family,
                                 cols.detach().expand(*bs, N * (D + 1), c).reshape(-1, N * (D + 1), c))
            y = y.reshape(*bs, M * (D + 1), c)
        elif cols.is_cuda and cols.dtype == torch.float32 and self._is_native_task():
            from .. import kernels as K

            M, DX = self.x1.shape[-2:]
            N, c = cols.shape[-2:]
            bs = torch.broadcast_shapes(self.batch_shape, cols.shape[:-2])
            x1 = self.x1.detach().expand(*bs, M, DX).reshape(-1, M, DX)
            x2 = x1 if self._same_points() else self.x2.detach().expand(*bs, N, DX).reshape(-1, N, DX)
            theta, Bt = self._task_operands(bs)
            y = K.kernel_task_mv(x1, x2, theta, Bt, self.covar_func.native_family,
                                 cols.detach().expand(*bs, N, c).reshape(-1, N, c))
            y = y.reshape(*bs, M, c)
        elif cols.is_cuda and cols.dtype == torch.float32 and self._is_native_param():
            from .. import kernels as K

            M, D = self.x1.shape[-2:]
            N, c = cols.shape[-2:]
            bs = torch.broadcast_shapes(self.batch_shape, cols.shape[:-2])
            x1 = self.x1.detach().expand(*bs, M, D).reshape(-1, M, D)
            x2 = x1 if self._same_points() else self.x2.detach().expand(*bs, N, D).reshape(-1, N, D)
            y = K.kernel_param_mv(x1, x2, self._param_theta(bs), self.covar_func.native_family,
                                  cols.detach().expand(*bs, N, c).reshape(-1, N, c))
            y = y.reshape(*bs, M, c)
        elif cols.is_cuda and ((cols.dtype == torch.float32 and self._is_native())
                               or (cols.dtype == torch.float64 and self._is_native_f64())):
            from .. import kernels as K

            M, D = self.x1.shape[-2:]
            N, c = cols.shape[-2:]
            bs = torch.broadcast_shapes(self.batch_shape, cols.shape[:-2])
            x1 = self.x1.detach().expand(*bs, M, D).reshape(-1, M, D)
            x2 = x1 if self._same_points() else self.x2.detach().expand(*bs, N, D).reshape(-1, N, D)
            y = K.kernel_mv(x1, x2, self._theta(bs, cols.dtype), self.covar_func.native_family,
                            cols.detach().expand(*bs, N, c).reshape(-1, N, c))
            y = y.reshape(*bs, M, c)
        else:
            y = self._dense_covar() @ cols.contiguous()
        return y[..., 0] if vec else y

    def _expand_batch(self, batch_shape):
        batch_shape = torch.Size(batch_shape)
        x1 = self.x1.expand(*batch_shape, *self.x1.shape[-2:])
        x2 = x1 if self._same_points() else self.x2.expand(*batch_shape, *self.x2.shape[-2:])
        params = {}
        for name, val in self.tensor_params.items():
            nb = self.num_nonbatch_dimensions[name]
            params[name] = val.expand(*batch_shape, *(val.shape[val.dim() - nb:] if nb else ()))
        return self._rebuild(x1, x2, params)

    def _permute_batch(self, *dims: int):
        x1 = self.x1.permute(*dims, -2, -1)
        x2 = x1 if self._same_points() else self.x2.permute(*dims, -2, -1)
        params = {name: val.permute(*dims, *range(len(dims), val.dim())) for name, val in self.tensor_params.items()}
        return self._rebuild(x1, x2, params)

    def _unsqueeze_batch(self, dim: int):
        x1 = self.x1.unsqueeze(dim)
        x2 = x1 if self._same_points() else self.x2.unsqueeze(dim)
        return self._rebuild(x1, x2, {name: val.unsqueeze(dim) for name, val in self.tensor_params.items()})

    # ------------------------------------------------------------------ entries
    def _diagonal(self) -> Tensor:
        p, q = self.num_outputs_per_input
        n = self.x1.shape[-2]
        if ((self._native_refusal(check_device=False) is None or self._native_f64_refusal(check_device=False) is None
             or self._native_param_refusal(check_device=False) is None) and self._same_points()):
            # g(0) = 1 for every native family: the diagonal is outputscale^2, no kernel launch
            return self.tensor_params["outputscale"].square().unsqueeze(-1).expand(*self.batch_broadcast_shape, n)
        if self._native_task_refusal(check_device=False) is None and self._same_points():
            # g(0) = 1: outputscale^2 task_covar[t_i, t_i], the table's diagonal gathered at the ids; no covar_func
            batch = self.batch_broadcast_shape
            ids = self.x1[..., -1].long().expand(*batch, n)
            own = self.tensor_params["task_covar"].diagonal(dim1=-2, dim2=-1).expand(*batch, -1).gather(-1, ids)
            return self.tensor_params["outputscale"].square().unsqueeze(-1) * own
        if self._native_grad_refusal(check_device=False) is None and self._same_points():
            # the block of a point with itself is outputscale^2 diag(1, 1 / l_1^2, .., 1 / l_D^2): no launch, no covar_func
            D = self.x1.shape[-1]
            batch = self.batch_broadcast_shape
            inv2 = (1.0 / self.tensor_params["lengthscale"]).square().expand(*batch, 1, D)[..., 0, :]
            os2 = self.tensor_params["outputscale"].square().unsqueeze(-1)
            per = torch.cat((torch.ones_like(inv2[..., :1]), inv2), -1) * os2
            return per.unsqueeze(-2).expand(*batch, n, D + 1).reshape(*batch, n * (D + 1))
        # the pairs (x1_i, x2_i) as a leading batch dimension of 1 x 1 (or p x q) kernel matrices
        a = self.x1.movedim(-2, 0).unsqueeze(-2)
        b = self.x2.movedim(-2, 0).unsqueeze(-2)
        params = {name: val.unsqueeze(0) for name, val in self.tensor_params.items()}
        blocks = to_dense(self.covar_func(a, b, **params, **self.nontensor_params)).movedim(0, -3)  # [*b, n, p, q]
        assert blocks.shape[-2:] == torch.Size((p, q))
        if (p, q) == (1, 1):
            return blocks[..., 0, 0]
        return blocks.diagonal(dim1=-2, dim2=-1).reshape(*blocks.shape[:-3], -1)

    def _get_indices(self, row_index: Tensor, col_index: Tensor, *batch_indices: Tensor) -> Tensor:
        p, q = self.num_outputs_per_input
        shape = torch.broadcast_shapes(row_index.shape, col_index.shape, *(i.shape for i in batch_indices))
        row = row_index.expand(shape).reshape(-1)
        col = col_index.expand(shape).reshape(-1)
        bidx = tuple(i.expand(shape).reshape(-1) for i in batch_indices)
        # one 1 x 1 (or p x q) kernel matrix per requested entry: only those entries are evaluated
        a = self.x1[(*bidx, row.div(p, rounding_mode="floor"))].unsqueeze(-2)
        b = self.x2[(*bidx, col.div(q, rounding_mode="floor"))].unsqueeze(-2)
        params = {name: val[bidx] for name, val in self.tensor_params.items()}
        blocks = to_dense(self.covar_func(a, b, **params, **self.nontensor_params))
        assert blocks.shape[-2:] == torch.Size((p, q))
        if (p, q) == (1, 1):
            return blocks[..., 0, 0].reshape(shape)
        lead = blocks.reshape(-1, p, q)
        pick = torch.arange(lead.shape[0], device=lead.device)
        return lead[pick, (row % p).expand(lead.shape[0]), (col % q).expand(lead.shape[0])].reshape(shape)

    def _getitem(self, row_index, col_index, *batch_indices):
        if self.num_outputs_per_input != (1, 1):
            points = self._whole_point_slices(row_index, col_index)
            if points is None:
                return super()._getitem(row_index, col_index, *batch_indices)  # (indexed densely)
            row_index, col_index = points
        x1 = self.x1[(*batch_indices, row_index, _NOOP)]
        same = self._same_points() and isinstance(row_index, slice) and row_index == col_index
        x2 = x1 if same else self.x2[(*batch_indices, col_index, _NOOP)]
        params = {name: val[(*batch_indices, *([_NOOP] * self.num_nonbatch_dimensions[name]))]
                  for name, val in self.tensor_params.items()}
        return self._rebuild(x1, x2, params)

    def _whole_point_slices(self, row_index, col_index):
        """Inside the gradient gate: the slices over the POINTS that two step-free slices of whole points select
        (kernel_linear_operator.py:300-340 of the reference divides such slices by the outputs per input); None for
        anything else, which is indexed densely."""
        if self._native_grad_refusal(check_device=False) is not None:
            return None
        out = []
        for index, size, per in zip((row_index, col_index), self.shape[-2:], self.num_outputs_per_input):
            if not isinstance(index, slice):
                return None
            start, stop, step = index.indices(size)
            if step != 1 or start % per or stop % per or stop <= start:
                return None
            out.append(slice(start // per, stop // per, None))
        return tuple(out)

    # ------------------------------------------------------------------ derivatives
    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """d / d(x1, x2, parameters in sorted order) of sum_s u_s^T K v_s; None for a tensor that asks for no gradient."""
        if left_vecs.dim() == 1:
            left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
        names = list(self._differentiable_kwargs)
        if left_vecs.is_cuda and left_vecs.dtype == torch.float32 and self._is_native():
            return self._bilinear_derivative_native(left_vecs, right_vecs, names)
        if (left_vecs.is_cuda and left_vecs.dtype == torch.float64 and right_vecs.dtype == torch.float64
                and self._is_native_f64()):
            return self._bilinear_derivative_native(left_vecs, right_vecs, names)
        if left_vecs.is_cuda and left_vecs.dtype == torch.float32 and self._is_native_task():
            return self._bilinear_derivative_task(left_vecs, right_vecs, names)
        if left_vecs.is_cuda and left_vecs.dtype == torch.float32 and self._is_native_param():
            return self._bilinear_derivative_param(left_vecs, right_vecs, names)
        if (left_vecs.is_cuda and left_vecs.dtype == torch.float32 and self._is_native_grad()
                and not (self.x1.requires_grad or self.x2.requires_grad)):
            # (native gradients of the points are not built for this kind: such a call takes the general path whole)
            return self._bilinear_derivative_native(left_vecs, right_vecs, names, grad=True)
        tensors = [self.x1, self.x2] + [self.tensor_params[n] for n in names]
        leaves = [t.detach().requires_grad_(True) if t.requires_grad and t.dtype.is_floating_point else t.detach()
                  for t in tensors]
        need = [t for t in leaves if t.requires_grad]
        if not need:
            return (None,) * len(tensors)
        with torch.enable_grad():
            dense = to_dense(self.covar_func(leaves[0], leaves[1], **dict(zip(names, leaves[2:])),
                                             **self.nontensor_params))
            loss = (left_vecs * (dense @ right_vecs)).sum()
            grads = list(torch.autograd.grad(loss, need, allow_unused=True))
        return tuple(grads.pop(0) if t.requires_grad else None for t in leaves)

    def _theta_to_params(self, g: Tensor, theta: Tensor, D: int, bs, out: dict) -> None:
        """d / d theta [B, D + 1] as the gradients of the lengthscale and outputscale tensors, where they ask for one."""
        ls, os_ = self.tensor_params["lengthscale"], self.tensor_params["outputscale"]
        if ls.requires_grad:  # theta_d = 1 / l_d: d / d l_d = -theta_d^2 d / d theta_d; a shared l sums over d
            d_ls = (-(theta[:, :D] ** 2) * g[:, :D]).reshape(*bs, 1, D)
            if ls.shape[-1] == 1 and D > 1:
                d_ls = d_ls.sum(-1, keepdim=True)
            out["lengthscale"] = d_ls.sum_to_size(ls.shape)
        if os_.requires_grad:  # theta_D = os^2: d / d os = 2 os d / d theta_D
            out["outputscale"] = (2.0 * torch.broadcast_to(os_.detach(), tuple(bs)) * g[:, D].reshape(tuple(bs))).sum_to_size(os_.shape)

    def _bilinear_derivative_task(self, left_vecs: Tensor, right_vecs: Tensor, names):
        """Inside the task gate: every gradient from the native kernels, nothing of size M N allocated."""
        from .. import kernels as K

        ls, os_, Bt = (self.tensor_params[k] for k in ("lengthscale", "outputscale", "task_covar"))
        M, DX = self.x1.shape[-2:]
        N, t = self.x2.shape[-2], right_vecs.shape[-1]
        T = Bt.shape[-1]
        bs = torch.broadcast_shapes(self.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
        out = {"x1": None, "x2": None, "lengthscale": None, "outputscale": None, "task_covar": None}
        if not any(p.requires_grad for p in (self.x1, self.x2, ls, os_, Bt)):
            return (None, None) + (None,) * len(names)
        family = self.covar_func.native_family
        x1 = self.x1.detach().expand(*bs, M, DX).reshape(-1, M, DX)
        x2 = x1 if self._same_points() else self.x2.detach().expand(*bs, N, DX).reshape(-1, N, DX)
        theta, task = self._task_operands(bs)
        U = left_vecs.detach().expand(*bs, M, t).reshape(-1, M, t)
        V = right_vecs.detach().expand(*bs, N, t).reshape(-1, N, t)
        if ls.requires_grad or os_.requires_grad or Bt.requires_grad:
            g, g_task = K.kernel_task_bilinear(x1, x2, theta, task, family, U, V)
            self._theta_to_params(g, theta, DX - 1, bs, out)
            if Bt.requires_grad:
                out["task_covar"] = g_task.reshape(*bs, T, T).sum_to_size(Bt.shape)
        # the x2 side is the x1 side of the transposed problem: x1 <-> x2, U <-> V, Bt transposed
        if self.x1.requires_grad:
            out["x1"] = K.kernel_task_points_grad(x1, x2, theta, task, family, U, V).reshape(*bs, M, DX).sum_to_size(self.x1.shape)
        if self.x2.requires_grad:
            out["x2"] = K.kernel_task_points_grad(x2, x1, theta, task.mT, family, V, U).reshape(*bs, N, DX).sum_to_size(self.x2.shape)
        return (out["x1"], out["x2"]) + tuple(out[n] for n in names)

    def _bilinear_derivative_param(self, left_vecs: Tensor, right_vecs: Tensor, names):
        """Inside the param gate: every gradient from the native kernels, nothing of size M N allocated."""
        from .. import kernels as K

        extra = "alpha" if "alpha" in self.tensor_params else "period_length"
        ls, os_, sh = (self.tensor_params[k] for k in ("lengthscale", "outputscale", extra))
        M, D = self.x1.shape[-2:]
        N, t = self.x2.shape[-2], right_vecs.shape[-1]
        bs = torch.broadcast_shapes(self.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
        out = {"x1": None, "x2": None, "lengthscale": None, "outputscale": None, extra: None}
        if not any(p.requires_grad for p in (self.x1, self.x2, ls, os_, sh)):
            return (None, None) + (None,) * len(names)
        family = self.covar_func.native_family
        x1 = self.x1.detach().expand(*bs, M, D).reshape(-1, M, D)
        x2 = x1 if self._same_points() else self.x2.detach().expand(*bs, N, D).reshape(-1, N, D)
        theta = self._param_theta(bs)
        U = left_vecs.detach().expand(*bs, M, t).reshape(-1, M, t)
        V = right_vecs.detach().expand(*bs, N, t).reshape(-1, N, t)
        if ls.requires_grad or os_.requires_grad or sh.requires_grad:
            g = K.kernel_param_bilinear(x1, x2, theta, family, U, V)  # [B, 2 D + 2], d / d theta
            self._theta_to_params(g, theta, D, bs, out)
            if sh.requires_grad and extra == "alpha":
                out[extra] = g[:, D + 1].reshape(tuple(bs)).sum_to_size(sh.shape)
            elif sh.requires_grad:  # nu_k = 1 / p_k: d / d p_k = -nu_k^2 d / d nu_k; a shared p sums over k
                d_p = (-(theta[:, D + 2:] ** 2) * g[:, D + 2:]).reshape(*bs, 1, D)
                if sh.shape[-1] == 1 and D > 1:
                    d_p = d_p.sum(-1, keepdim=True)
                out[extra] = d_p.sum_to_size(sh.shape)
        # the x2 side is the x1 side of the transposed problem (x1 <-> x2, U <-> V)
        if self.x1.requires_grad:
            out["x1"] = K.kernel_param_points_grad(x1, x2, theta, family, U, V).reshape(*bs, M, D).sum_to_size(self.x1.shape)
        if self.x2.requires_grad:
            out["x2"] = K.kernel_param_points_grad(x2, x1, theta, family, V, U).reshape(*bs, N, D).sum_to_size(self.x2.shape)
        return (out["x1"], out["x2"]) + tuple(out[n] for n in names)

    def _bilinear_derivative_native(self, left_vecs: Tensor, right_vecs: Tensor, names, grad: bool = False):
        """grad: the gradient kernel (the vectors have D + 1 rows per point; the caller saw that no points tensor asks
        for a gradient)."""
        from .. import kernels as K

        ls, os_ = self.tensor_params["lengthscale"], self.tensor_params["outputscale"]
        M, D = self.x1.shape[-2:]
        N, t = self.x2.shape[-2], right_vecs.shape[-1]
        p = D + 1 if grad else 1
        bs = torch.broadcast_shapes(self.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
        out = {"x1": None, "x2": None, "lengthscale": None, "outputscale": None}
        if not any(p.requires_grad for p in (self.x1, self.x2, ls, os_)):
            return (None, None) + (None,) * len(names)
        family = self.covar_func.native_family
        x1 = self.x1.detach().expand(*bs, M, D).reshape(-1, M, D)
        x2 = x1 if self._same_points() else self.x2.detach().expand(*bs, N, D).reshape(-1, N, D)
        theta = self._theta(bs, left_vecs.dtype)
        U = left_vecs.detach().expand(*bs, M * p, t).reshape(-1, M * p, t)
        V = right_vecs.detach().expand(*bs, N * p, t).reshape(-1, N * p, t)
        if ls.requires_grad or os_.requires_grad:
            bilinear = K.kernel_grad_bilinear if grad else K.kernel_bilinear
            g = bilinear(x1, x2, theta, family, U, V)  # [B, D + 1], d / d theta
            self._theta_to_params(g, theta, D, bs, out)
        # each side with the other held fixed; x1 and x2 the same leaf: autograd adds the two.  The x2 side is the x1 side
        # of the transposed problem (x1 <-> x2, U <-> V).
        if self.x1.requires_grad:
            out["x1"] = K.kernel_points_grad(x1, x2, theta, family, U, V).reshape(*bs, M, D).sum_to_size(self.x1.shape)
        if self.x2.requires_grad:
            out["x2"] = K.kernel_points_grad(x2, x1, theta, family, V, U).reshape(*bs, N, D).sum_to_size(self.x2.shape)
        return (out["x1"], out["x2"]) + tuple(out[n] for n in names)


__all__ = ["KernelLinearOperator"]
