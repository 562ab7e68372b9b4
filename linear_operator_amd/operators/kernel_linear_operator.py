"""KernelLinearOperator: the covariance matrix K(x1, x2) of a kernel function held as its inputs -- the points and the
hyperparameters, N D numbers instead of N^2 (the reference's operators/kernel_linear_operator.py, same constructor and
results).  `covar_func(x1, x2, **params)` may be any callable; it is evaluated densely whenever the matrix itself is
needed (the general path, as in the reference, on any device and in any dtype).

Native path.  `VARIANTS` below describes every kind of operator the HIP kernels take, one row each: what `covar_func`
must carry (linear_operator_amd.covariance), the parameters with their shapes, the limit on D and the kernels.py
wrappers.  One gate body (`_variant_refusal`) reads a row; `_native_refusal`, `_native_f64_refusal`,
`_native_grad_refusal`, `_native_task_refusal` and `_native_param_refusal` are its five views (`_native_sm_refusal` a sixth,
over `MIXTURE_VARIANTS`), and `_native_variant`
returns the one row whose gate passes (no operator passes two).  Inside a gate the matrix is NEVER formed and
covar_func is not called:

  _matmul / _t_matmul   the row's product, rectangular x1 / x2 included, for a device right-hand side of the row's dtype
  _kernel_descriptor    x1 and x2 the same points: the row's LO_OP_KERNEL_*_DIAG kind, so that AddedDiag(Kernel, Diag)
                        runs CG, Lanczos, MINRES and the pivoted Cholesky on the device with no Python call per iteration
  _diagonal             from the parameters alone, no launch;  _get_indices / _get_rows evaluate only the requested entries
  _bilinear_derivative  the parameters from the row's bilinear wrapper through theta (d l = -theta^2 d theta, d os = 2 os
                        d os^2, a shared l summed over D), the points from its points-gradient wrapper: one call per side
                        that needs one, the x2 side as the x1 side of the transposed problem

  plain   rbf, matern12/32/52, float32: csrc/lo_kernel_op.hip, LO_OP_KERNEL_DIAG; the diagonal is outputscale^2
  f64     the same with every tensor float64: csrc/lo_kernel_op_f64.hip.  Its descriptor comes from
          `_kernel_descriptor_f64` (AddedDiag and Sum lower through it: _attach_diag, utils.linear_cg._lower_f64);
          `_kernel_descriptor()` stays None for float64, as it always was
  grad    rbf_grad with num_outputs_per_input (D + 1, D + 1): csrc/lo_kernel_grad.hip, LO_OP_KERNEL_GRAD_DIAG; the
          diagonal is outputscale^2 (1, 1 / l_1^2, .., 1 / l_D^2) per point.  No native gradients of the points: a
          derivative call that asks for them takes the general path whole.  `_getitem` rebuilds the operator over
          slices of whole points and indexes anything else densely
  task    *_task, the points carry the task id in their last column, `task_covar` [*b, T, T] (treated as symmetric:
          `_transpose_nonbatch` swaps the points and keeps the parameters): csrc/lo_kernel_task.hip,
          LO_OP_KERNEL_TASK_DIAG; the diagonal is outputscale^2 task_covar[t_i, t_i].  Ids outside [0, T) are the
          caller's error: the gate does not synchronise to look, the kernels clamp
  param   rq (`alpha` [*b]) and periodic (`period_length` [*b, 1, D] or [*b, 1, 1]): csrc/lo_kernel_param.hip,
          LO_OP_KERNEL_PARAM_DIAG, also a term of a lowered sum; d p = -nu^2 d nu; the diagonal is outputscale^2

  sm      spectral_mixture, the row of `MIXTURE_VARIANTS` (kept apart: `VARIANTS` holds the rows whose covar_func carries a
          native_family, this one carries none): `mixture_weights` [*b, Q], `mixture_means` and `mixture_scales`
          [*b, Q, D], no lengthscale and no outputscale, D and Q at most 16: csrc/lo_kernel_sm.hip,
          LO_OP_KERNEL_SM_DIAG, also a term of a lowered sum; the sixth gate `_native_sm_refusal`; theta holds the raw
          values, so d / d theta IS the parameters' gradient; the diagonal is sum_q w_q.  Inside the gate the kernel is
          always taken, no threshold: its purpose is memory (the dense function forms a [Q, M, N, D] temporary).  The
          five gates above refuse it with "covar_func has no native_family" / "no native_outputs == '..'", so the Sum
          fusion, Kronecker and LMC kinds never take one

`_native_refusal` answers a grad, task, param or float64 operator with "more than one output per input", "parameters
other than lengthscale and outputscale" or "not float32", so the fp32 fusion gates of the Sum, Kronecker and LMC
operators never take one.  Anything outside the gates (D beyond the limit, mixed element types, CPU, other parameters)
takes the general path, and so does a right-hand side of the other float type.
"""
from __future__ import annotations

from collections import defaultdict
from typing import Callable, NamedTuple, Optional

import torch
from torch import Tensor

from .. import _hip
from .. import kernels as K
from ._linear_operator import LinearOperator, to_dense

_NOOP = slice(None, None, None)


class _Extra(NamedTuple):
    """A variant's parameter beyond lengthscale and outputscale."""
    name: str
    rule: str  # its shape: "scalar" [*b], "ard" [*b, 1, D] or [*b, 1, 1], "table" [*b, T, T]
    col: int   # theta holds it in column D + col (scalar) or, as 1 / p, in the D columns from D + col on (ard); table: unused


class _Variant(NamedTuple):
    """One kind of operator the native kernels take.  The wrappers are names in kernels.py, looked up per call."""
    gate: str                   # the operator's method that answers for it
    tag: Optional[str]          # covar_func.native_outputs it answers to
    dtype: torch.dtype          # of every tensor, the vectors included
    families: Optional[tuple]   # the admissible covar_func.native_family codes; None: any
    no_family: str              # the gate's answer to another one
    extras: dict                # native_family -> _Extra (None: every family)
    ids: int                    # id columns of the points behind the D coordinates
    block: bool                 # D + 1 rows per point instead of 1
    max_dim: str                # the _hip limit on the points' columns
    theta: str
    mv: str
    bilinear: str
    points_grad: Optional[str]  # None: no native gradients of the points
    descriptor: str
    # a row whose parameters are not lengthscale / outputscale (+ extras): name -> non-batch dimensions, in the order the
    # theta builder takes them.  Such a row needs no native_family: its wrappers take (points, theta, vectors)
    params: Optional[dict] = None
    max_mix: Optional[str] = None  # the _hip limit on the leading non-batch dimension of the parameters (the mixtures Q)


_PLAIN = _Variant("_native_refusal", None, torch.float32, None, "covar_func has no native_family", {}, 0, False, "LO_KERNEL_MAX_DIM",
                  "kernel_theta", "kernel_mv", "kernel_bilinear", "kernel_points_grad", "kernel_diag_descriptor")
_F64 = _PLAIN._replace(gate="_native_f64_refusal", dtype=torch.float64)
_GRAD = _PLAIN._replace(gate="_native_grad_refusal", tag="grad", families=(_hip.LO_KERNEL_RBF,),
                        no_family="a gradient kernel of a family other than RBF", block=True,
                        max_dim="LO_KERNEL_GRAD_MAX_DIM", mv="kernel_grad_mv", bilinear="kernel_grad_bilinear",
                        points_grad=None, descriptor="kernel_grad_diag_descriptor")
_TASK = _PLAIN._replace(gate="_native_task_refusal", tag="task", extras={None: _Extra("task_covar", "table", 0)}, ids=1,
                        mv="kernel_task_mv", bilinear="kernel_task_bilinear", points_grad="kernel_task_points_grad",
                        descriptor="kernel_task_diag_descriptor")
_PARAM = _PLAIN._replace(gate="_native_param_refusal", tag="param", families=(_hip.LO_KERNEL_RQ, _hip.LO_KERNEL_PERIODIC),
                         no_family="covar_func has no native_family among LO_KERNEL_RQ, LO_KERNEL_PERIODIC",
                         extras={_hip.LO_KERNEL_RQ: _Extra("alpha", "scalar", 1),
                                 _hip.LO_KERNEL_PERIODIC: _Extra("period_length", "ard", 2)},
                         max_dim="LO_KERNEL_PARAM_MAX_DIM", theta="kernel_param_theta", mv="kernel_param_mv",
                         bilinear="kernel_param_bilinear", points_grad="kernel_param_points_grad",
                         descriptor="kernel_param_diag_descriptor")
VARIANTS = (_PLAIN, _F64, _GRAD, _TASK, _PARAM)
_SM = _Variant("_native_sm_refusal", "sm", torch.float32, None, "", {}, 0, False, "LO_KERNEL_SM_MAX_DIM", "kernel_sm_theta",
               "kernel_sm_mv", "kernel_sm_bilinear", "kernel_sm_points_grad", "kernel_sm_diag_descriptor",
               params={"mixture_weights": 1, "mixture_means": 2, "mixture_scales": 2}, max_mix="LO_KERNEL_SM_MAX_MIX")
MIXTURE_VARIANTS = (_SM,)
_TAGGED = {v.tag: v for v in (*VARIANTS, *MIXTURE_VARIANTS) if v.tag is not None}


def _flat(t: Tensor, bs) -> Tensor:
    """t [*b, R, C] detached, broadcast to the batch `bs` and flattened to [B, R, C]."""
    R, C = t.shape[-2:]
    return t.detach().expand(*bs, R, C).reshape(-1, R, C)


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

    # ------------------------------------------------------------------ the gates of the native path
    def _extra(self, v: _Variant) -> Optional[_Extra]:
        return v.extras.get(self.covar_func.native_family, v.extras.get(None))

    def _variant_refusal(self, v: _Variant, check_device: bool = True) -> Optional[str]:
        """None when the native kernels of the variant `v` take this operator, else the reason they do not.
        `check_device=False` leaves out the device condition (what the rest of the gate decides can then be asked on any
        machine)."""
        if v.tag is not None and getattr(self.covar_func, "native_outputs", None) != v.tag:
            return f"covar_func has no native_outputs == '{v.tag}'"
        if v.params is not None:
            return self._mixture_refusal(v, check_device)
        family = getattr(self.covar_func, "native_family", None)
        if family is None or (v.families is not None and family not in v.families):
            return v.no_family
        DX = self.x1.shape[-1]
        D = DX - v.ids
        dim = None
        if D < 1 or self.x2.shape[-1] != DX or DX > getattr(_hip, v.max_dim):
            dim = f"D = {D} outside 1 .. {v.max_dim} - 1" if v.ids else f"D = {D} beyond {v.max_dim}"
        if v.block:  # (the outputs per input are stated in D)
            if dim is not None:
                return dim
            if self.num_outputs_per_input != (D + 1, D + 1):
                return f"num_outputs_per_input is not ({D + 1}, {D + 1})"
        elif self.num_outputs_per_input != (1, 1):
            return "more than one output per input"
        extra = self._extra(v)
        names = {"lengthscale", "outputscale"} if extra is None else {"lengthscale", "outputscale", extra.name}
        if self.nontensor_params or set(self.tensor_params) != names:
            return "parameters other than " + ("lengthscale and outputscale" if extra is None
                                               else f"lengthscale, outputscale and {extra.name}")
        if dim is not None:
            return dim
        ls, os_ = self.tensor_params["lengthscale"], self.tensor_params["outputscale"]
        batch, nonbatch = self.batch_broadcast_shape, self.num_nonbatch_dimensions
        ard = ((*batch, 1, D), (*batch, 1, 1))
        if nonbatch["lengthscale"] != 2 or ls.shape not in ard:
            return f"lengthscale of shape {tuple(ls.shape)}"
        if nonbatch["outputscale"] != 0 or os_.shape != batch:
            return f"outputscale of shape {tuple(os_.shape)}"
        tensors = [self.x1, self.x2, ls, os_]
        if extra is not None:
            p = self.tensor_params[extra.name]
            if extra.rule == "table":
                T = p.shape[-1]
                fits = nonbatch[extra.name] == 2 and p.shape == (*batch, T, T) and T >= 1
            elif extra.rule == "ard":
                fits = nonbatch[extra.name] == 2 and p.shape in ard
            else:
                fits = nonbatch[extra.name] == 0 and p.shape == batch
            if not fits:
                return f"{extra.name} of shape {tuple(p.shape)}"
            if extra.rule == "table" and T > _hip.LO_KERNEL_TASK_MAX_TASKS:
                return f"T = {T} beyond LO_KERNEL_TASK_MAX_TASKS"
            tensors.append(p)
        if any(t.dtype != v.dtype for t in tensors):
            return "not float32" if v.dtype == torch.float32 else "not float64"
        if check_device and not all(t.is_cuda for t in tensors):
            return "not on the device"
        return None

    def _mixture_refusal(self, v: _Variant, check_device: bool) -> Optional[str]:
        """The rest of the gate of a row with parameters of its own (`v.params`): weights [*b, Q] and per-mixture tables
        [*b, Q, D], exactly those."""
        if self.num_outputs_per_input != (1, 1):
            return "more than one output per input"
        names = list(v.params)
        if self.nontensor_params or set(self.tensor_params) != set(names):
            return "parameters other than " + ", ".join(names[:-1]) + " and " + names[-1]
        D = self.x1.shape[-1]
        if D < 1 or self.x2.shape[-1] != D or D > getattr(_hip, v.max_dim):
            return f"D = {D} beyond {v.max_dim}"
        batch, nonbatch = self.batch_broadcast_shape, self.num_nonbatch_dimensions
        Q = self.tensor_params[names[0]].shape[-1]
        for name, nb in v.params.items():
            p = self.tensor_params[name]
            if nonbatch[name] != nb or p.shape != ((*batch, Q) if nb == 1 else (*batch, Q, D)) or Q < 1:
                return f"{name} of shape {tuple(p.shape)}"
        if Q > getattr(_hip, v.max_mix):
            return f"Q = {Q} beyond {v.max_mix}"
        tensors = [self.x1, self.x2, *(self.tensor_params[name] for name in names)]
        if any(t.dtype != v.dtype for t in tensors):
            return "not float32"
        if check_device and not all(t.is_cuda for t in tensors):
            return "not on the device"
        return None

    def _native_variant(self, check_device: bool = True) -> Optional[_Variant]:
        """The variant whose gate passes, or None.  No operator passes two gates (grad needs D + 1 outputs per input,
        task and param a third parameter, f64 float64), so one candidate is asked, through its public gate: the row of
        covar_func.native_outputs, and the one-output row of the points' dtype where covar_func carries no tag or its
        row refuses."""
        tagged = _TAGGED.get(getattr(self.covar_func, "native_outputs", None))
        if tagged is not None and getattr(self, tagged.gate)(check_device) is None:
            return tagged
        plain = _F64 if self.x1.dtype == torch.float64 else _PLAIN
        return plain if getattr(self, plain.gate)(check_device) is None else None

    def _native_refusal(self, check_device: bool = True) -> Optional[str]:
        return self._variant_refusal(_PLAIN, check_device)

    def _native_f64_refusal(self, check_device: bool = True) -> Optional[str]:
        return self._variant_refusal(_F64, check_device)

    def _native_grad_refusal(self, check_device: bool = True) -> Optional[str]:
        return self._variant_refusal(_GRAD, check_device)

    def _native_task_refusal(self, check_device: bool = True) -> Optional[str]:
        return self._variant_refusal(_TASK, check_device)

    def _native_param_refusal(self, check_device: bool = True) -> Optional[str]:
        return self._variant_refusal(_PARAM, check_device)

    def _native_sm_refusal(self, check_device: bool = True) -> Optional[str]:
        return self._variant_refusal(_SM, check_device)

    def _is_native(self) -> bool:
        return self._native_refusal() is None

    def _is_native_f64(self) -> bool:
        return self._native_f64_refusal() is None

    def _is_native_grad(self) -> bool:
        return self._native_grad_refusal() is None

    def _is_native_task(self) -> bool:
        return self._native_task_refusal() is None

    def _is_native_param(self) -> bool:
        return self._native_param_refusal() is None

    def _is_native_sm(self) -> bool:
        return self._native_sm_refusal() is None

    def _same_points(self) -> bool:
        return _same_tensor(self.x1, self.x2)

    def _theta(self, v: _Variant, bs):
        """Inside the gate of `v`, for the batch `bs`: (theta of the variant's entry points, the operands between theta
        and the family: (Bt [B, T, T],) of the task variant, else ())."""
        if v.params is not None:
            return getattr(K, v.theta)(*(self.tensor_params[name] for name in v.params), bs, self.x1.shape[-1]), ()
        p, extra = self.tensor_params, self._extra(v)
        kw = {} if v.dtype == torch.float32 else {"dtype": v.dtype}
        if extra is not None and extra.rule != "table":
            kw[extra.name] = p[extra.name]
        theta = getattr(K, v.theta)(p["lengthscale"], p["outputscale"], bs, self.x1.shape[-1] - v.ids, **kw)
        return theta, ((_flat(p[extra.name], bs),) if extra is not None and extra.rule == "table" else ())

    def _lead(self, v: _Variant, theta, task=()):
        """What the wrappers of `v` take between the points and the vectors: theta (, Bt), the family code -- theta alone
        for a row with parameters of its own."""
        return (theta,) if v.params is not None else (theta, *task, self.covar_func.native_family)

    def _points(self, bs):
        """(x1 [B, M, DX], x2 [B, N, DX]) for the batch `bs`; one tensor when x1 and x2 are the same points."""
        x1 = _flat(self.x1, bs)
        return x1, (x1 if self._same_points() else _flat(self.x2, bs))

    def _descriptor(self, v: _Variant, batch_shape):
        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        X = self.x1.detach()
        X = X if X.shape[:-2] == bs else X.expand(*bs, *X.shape[-2:])
        theta, task = self._theta(v, bs)
        if v.params is not None:
            return getattr(K, v.descriptor)(X, theta)
        kw = {} if v.dtype == torch.float32 else {"dtype": v.dtype}
        return getattr(K, v.descriptor)(X, theta, self.covar_func.native_family,
                                        *(t.reshape(*bs, *t.shape[-2:]) for t in task), **kw)

    def _kernel_descriptor_f64(self, batch_shape=None):
        """The float64 LO_OP_KERNEL_DIAG descriptor inside the float64 gate when x1 and x2 are one tensor, else None."""
        if not (self._is_native_f64() and self._same_points()):
            return None
        return self._descriptor(_F64, batch_shape)

    def _kernel_descriptor(self, batch_shape=None):
        v = self._native_variant()
        if v is None or v is _F64 or not self._same_points():
            return None
        return self._descriptor(v, batch_shape)

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
        v = self._native_variant() if cols.is_cuda else None
        if v is not None and cols.dtype == v.dtype:
            bs = torch.broadcast_shapes(self.batch_shape, cols.shape[:-2])
            theta, task = self._theta(v, bs)
            y = getattr(K, v.mv)(*self._points(bs), *self._lead(v, theta, task), _flat(cols, bs))
            y = y.reshape(*bs, *y.shape[-2:])
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
        v = self._native_variant(check_device=False) if self._same_points() else None
        if v is not None:  # g(0) = 1 for every native family: from the parameters alone, no kernel launch, no covar_func
            batch = self.batch_broadcast_shape
            if v.params is not None:  # every mixture is its weight at tau = 0: sum_q w_q
                return self.tensor_params[next(iter(v.params))].sum(-1, keepdim=True).expand(*batch, n)
            os2 = self.tensor_params["outputscale"].square().unsqueeze(-1)
            if v.block:  # the block of a point with itself is outputscale^2 diag(1, 1 / l_1^2, .., 1 / l_D^2)
                D = self.x1.shape[-1]
                inv2 = (1.0 / self.tensor_params["lengthscale"]).square().expand(*batch, 1, D)[..., 0, :]
                per = torch.cat((torch.ones_like(inv2[..., :1]), inv2), -1) * os2
                return per.unsqueeze(-2).expand(*batch, n, D + 1).reshape(*batch, n * (D + 1))
            if v.ids:  # outputscale^2 task_covar[t_i, t_i], the table's diagonal gathered at the ids
                ids = self.x1[..., -1].long().expand(*batch, n)
                table = self.tensor_params[self._extra(v).name]
                return os2 * table.diagonal(dim1=-2, dim2=-1).expand(*batch, -1).gather(-1, ids)
            return os2.expand(*batch, n)
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
        v = self._native_variant() if left_vecs.is_cuda else None
        # (no native gradients of the points in the grad variant: such a call takes the general path whole)
        if (v is not None and left_vecs.dtype == v.dtype and (right_vecs.dtype == v.dtype or v.dtype == torch.float32)
                and (v.points_grad is not None or not (self.x1.requires_grad or self.x2.requires_grad))):
            return self._bilinear_derivative_native(left_vecs, right_vecs, names, v)
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

    def _theta_to_params(self, v: _Variant, g, theta: Tensor, bs, out: dict) -> None:
        """d / d theta (`g`; the task variant: with d / d Bt) as the gradients of the parameter tensors that ask for one."""
        D = self.x1.shape[-1] - v.ids
        if v.params is not None:  # theta [B, Q, 2 D + 1] holds the raw values: column 0, then D columns per table
            lo = 0
            for name, nb in v.params.items():
                p, width = self.tensor_params[name], 1 if nb == 1 else D
                if p.requires_grad:
                    d_p = g[:, :, lo] if nb == 1 else g[:, :, lo:lo + width]
                    out[name] = d_p.reshape(*bs, *d_p.shape[1:]).sum_to_size(p.shape)
                lo += width
            return
        extra = self._extra(v)
        if extra is not None and extra.rule == "table":
            g, g_table = g

        def inverse(lo: int, p: Tensor) -> Tensor:
            # theta_d = 1 / p_d: d / d p_d = -theta_d^2 d / d theta_d; a shared p sums over d
            d_p = (-(theta[:, lo:lo + D] ** 2) * g[:, lo:lo + D]).reshape(*bs, 1, D)
            if p.shape[-1] == 1 and D > 1:
                d_p = d_p.sum(-1, keepdim=True)
            return d_p.sum_to_size(p.shape)

        ls, os_ = self.tensor_params["lengthscale"], self.tensor_params["outputscale"]
        if ls.requires_grad:
            out["lengthscale"] = inverse(0, ls)
        if os_.requires_grad:  # theta_D = os^2: d / d os = 2 os d / d theta_D
            d_os = 2.0 * torch.broadcast_to(os_.detach(), tuple(bs)) * g[:, D].reshape(tuple(bs))
            out["outputscale"] = d_os.sum_to_size(os_.shape)
        p = None if extra is None else self.tensor_params[extra.name]
        if p is None or not p.requires_grad:
            return
        if extra.rule == "table":
            out[extra.name] = g_table.reshape(*bs, *p.shape[-2:]).sum_to_size(p.shape)
        elif extra.rule == "ard":
            out[extra.name] = inverse(D + extra.col, p)
        else:
            out[extra.name] = g[:, D + extra.col].reshape(tuple(bs)).sum_to_size(p.shape)

    def _bilinear_derivative_native(self, left_vecs: Tensor, right_vecs: Tensor, names, v: _Variant):
        """Inside the gate of `v` (the grad variant: the caller saw that no points tensor asks for a gradient): every
        gradient from the native kernels, nothing of size M N allocated."""
        params = [self.tensor_params[n] for n in names]
        if not any(t.requires_grad for t in (self.x1, self.x2, *params)):
            return (None, None) + (None,) * len(names)
        bs = torch.broadcast_shapes(self.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
        x1, x2 = self._points(bs)
        theta, task = self._theta(v, bs)
        U, V = _flat(left_vecs, bs), _flat(right_vecs, bs)
        out = dict.fromkeys(("x1", "x2", *names))
        if any(t.requires_grad for t in params):
            self._theta_to_params(v, getattr(K, v.bilinear)(x1, x2, *self._lead(v, theta, task), U, V), theta, bs, out)
        # each side with the other held fixed; x1 and x2 the same leaf: autograd adds the two.  The x2 side is the x1 side
        # of the transposed problem (x1 <-> x2, U <-> V, Bt transposed).
        if self.x1.requires_grad:
            g = getattr(K, v.points_grad)(x1, x2, *self._lead(v, theta, task), U, V)
            out["x1"] = g.reshape(*bs, *g.shape[-2:]).sum_to_size(self.x1.shape)
        if self.x2.requires_grad:
            g = getattr(K, v.points_grad)(x2, x1, *self._lead(v, theta, tuple(t.mT for t in task)), V, U)
            out["x2"] = g.reshape(*bs, *g.shape[-2:]).sum_to_size(self.x2.shape)
        return (out["x1"], out["x2"]) + tuple(out[n] for n in names)


__all__ = ["KernelLinearOperator"]
