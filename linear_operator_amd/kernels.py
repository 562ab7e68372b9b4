"""Tensor-level wrappers over the C ABI (include/lo_amd.h): shape checks, batch flattening, workspaces.

Everything here takes contiguous fp32 HIP tensors and launches hand-written gfx950 kernels on the
current stream; there is no other implementation behind these functions.
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
import math
import os
import threading
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Callable, Optional

import torch

from . import _hip


@dataclass
class OperatorDescriptor:
    """Lowered form of an operator tree (the operators' `_kernel_descriptor()`): what the kernels need."""

    kind: int
    B: int
    N: int
    A0: Optional[torch.Tensor] = None  # C [B,N,R] | K [B,N,N] | K1 [B,n1,n1]
    # K2 [B,n2,n2] | G [B,N,q] (Hadamard: A0 = F [B,N,p]) | theta [B,D+1] (Kernel: A0 = X [B,N,D], R = D, n2 = family)
    # | theta [B,T,D+1] (KernelSum: A0 = X, R = D, n2 = the packed families, kernel_terms = T)
    # | theta [B,D+1] (KernelKron: A0 = X [B,n,D], R = D, n2 = family, kernel_terms = T, task = Bt, N = n T)
    # | theta [B,D+1] (KernelTask: A0 = X [B,N,D+1] with the task id last, R = D, n2 = family, kernel_terms = T, task = Bt)
    # | theta [B,Q,D+1] (KernelLmc: A0 = X [B,n,D], R = D, n2 = the packed families with Q in bits 16 .. 19 (kernel_lmc_terms),
    #   kernel_terms = T, task = Bt [B,Q,T,T], N = n T)
    # | theta [B,2D+2] (KernelParam: A0 = X [B,N,D], R = D, n2 = LO_KERNEL_RQ / LO_KERNEL_PERIODIC; kernel_param_theta)
    # | theta [B,Q,2D+1] (KernelSm: A0 = X [B,N,D], R = D, n2 = Q; kernel_sm_theta)
    A1: Optional[torch.Tensor] = None
    d: Optional[torch.Tensor] = None  # [B,N] (FULL) or [B] (CONST)
    diag_mode: int = _hip.LO_DIAG_NONE
    R: int = 0
    n2: int = 0
    batch_shape: torch.Size = torch.Size()
    terms: tuple = ()  # LO_OP_SUM: the summed structured terms (descriptors without a diagonal), left to right
    interp: tuple = ()  # LO_OP_SKI_DIAG: (left_idx, left_vals, right_idx, right_vals), [B, N, J] int64 / fp32
    interp_plan: Optional[torch.Tensor] = None  # LO_OP_SKI_DIAG: grid-major copy of W_r kept across calls (interp_plan)
    mask: tuple = ()  # LO_OP_MASKED: (descriptor of the base operator, idx int64 [M] of the selected rows)
    # LO_OP_SKI_GRID_DIAG, LO_OP_TOEPLITZ_KRON_DIAG: the grid shape (M_1, .., M_D); A0 = the factors' columns
    # [B, M_1 + .. + M_D]
    grid: tuple = ()
    # element type of A0 / A1 / d.  The C struct does not record it: float64 descriptors (low-rank / dense / Kronecker /
    # sums of those) go to lo_matvec_f64 and the float64 solvers only, and c_struct() refuses to hand one to an entry
    # point that reads `float*`
    dtype: torch.dtype = torch.float32
    # LO_OP_KERNEL_SUM_DIAG: T, the struct's `nterms` (the kind has no `terms`); LO_OP_KERNEL_KRON_DIAG,
    # LO_OP_KERNEL_TASK_DIAG, LO_OP_KERNEL_LMC_DIAG: the tasks T; LO_OP_SKI_SUM_DIAG: the P summed terms (A0 [B, P, M],
    # interp [B, P, N, J])
    kernel_terms: int = 0
    # LO_OP_KERNEL_KRON_DIAG, LO_OP_KERNEL_TASK_DIAG: Bt [B, T, T], LO_OP_KERNEL_LMC_DIAG: Bt [B, Q, T, T]: the union slot
    # `task` (a DEVICE pointer)
    task: Optional[torch.Tensor] = None

    @property
    def device(self):
        for t in (self.A0, self.A1, self.d):
            if t is not None:
                return t.device
        for term in self.terms:
            return term.device
        for t in self.interp:
            return t.device
        if self.mask:
            return self.mask[1].device
        raise ValueError("empty descriptor")

    def c_struct(self, dtype: torch.dtype = torch.float32) -> _hip.OpDesc:
        """The lo_op_desc for an entry point that reads the operands as `dtype`; any other descriptor is refused."""
        if self.dtype != dtype:
            raise _hip.HipExtensionError(
                f"a {self.dtype} operator descriptor was handed to a {dtype} entry point of liblo_amd (float64 "
                "descriptors are taken by matvec and the float64 solvers only)")
        s = _hip.OpDesc()
        s.kind, s.diag_mode, s.B, s.N, s.R, s.n2 = self.kind, self.diag_mode, self.B, self.N, self.R, self.n2
        s.A0 = None if self.A0 is None else self.A0.data_ptr()
        s.A1 = None if self.A1 is None else self.A1.data_ptr()
        s.d = None if self.d is None else self.d.data_ptr()
        s.nterms = len(self.terms) or self.kernel_terms
        if self.terms:  # host array of term descriptors; kept alive by the returned struct
            arr = (_hip.OpDesc * len(self.terms))(*[t.c_struct(dtype) for t in self.terms])
            s.terms = C.cast(arr, C.POINTER(_hip.OpDesc))
            s._terms_keepalive = arr
        if self.interp:  # the union slot `interp`: a host struct of the four device pointers
            w = _hip.InterpDesc(*[t.data_ptr() for t in self.interp],
                                None if self.interp_plan is None else self.interp_plan.data_ptr())
            if self.grid:
                w.grid_ndim = len(self.grid)
                w.grid_m = (C.c_int64 * 3)(*self.grid)
            s.terms = C.cast(C.pointer(w), C.POINTER(_hip.OpDesc))
            s._interp_keepalive = w
        if self.kind == _hip.LO_OP_TOEPLITZ_KRON_DIAG:  # the union slot `grid`: a host struct of the grid shape
            g = _hip.GridDesc(len(self.grid), 0, (C.c_int64 * 3)(*self.grid))
            s.terms = C.cast(C.pointer(g), C.POINTER(_hip.OpDesc))
            s._grid_keepalive = g
        if self.task is not None:  # the union slot `task`: the device pointer itself
            s.terms = C.cast(C.c_void_p(self.task.data_ptr()), C.POINTER(_hip.OpDesc))
        if self.mask:  # the union slot `mask`: a host struct of the base's host descriptor and the device index list
            base = self.mask[0].c_struct()
            m = _hip.MaskDesc(C.pointer(base), self.mask[1].data_ptr(), self.mask[1].numel())
            s.terms = C.cast(C.pointer(m), C.POINTER(_hip.OpDesc))
            s._mask_keepalive = (base, m)
        return s

    def without_diag(self) -> "OperatorDescriptor":
        return OperatorDescriptor(self.kind, self.B, self.N, self.A0, self.A1, None, _hip.LO_DIAG_NONE, self.R,
                                  self.n2, self.batch_shape, self.terms, self.interp, self.interp_plan, self.mask,
                                  self.grid, self.dtype, self.kernel_terms, self.task)


def _check_dtype(dtype, *tensors):
    """The descriptor builders' element type: float32 (every engine) or, on request, float64 (matvec and the float64
    solvers); all tensors of one descriptor share it."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"operator descriptors are float32 or float64, not {dtype}")
    if dtype == torch.float64:
        for t in tensors:
            if t is not None and t.dtype != dtype:
                raise _hip.HipExtensionError(f"a float64 operator descriptor takes float64 tensors only; got {t.dtype}")


def sum_descriptor(terms, d: Optional[torch.Tensor] = None, const_diag: bool = False, dtype=torch.float32):
    """SumLinearOperator(A_1, ..., A_n) (+ one diagonal): y = sum_i A_i v + d o v (sum_linear_operator.py:47-51).
    `terms`: 2 .. LO_MAX_TERMS descriptors of kind low-rank / dense / Kronecker / matrix-free kernel (LO_OP_KERNEL_DIAG;
    float32 sums also LO_OP_KERNEL_SUM_DIAG, LO_OP_KERNEL_PARAM_DIAG and LO_OP_KERNEL_SM_DIAG) WITHOUT a diagonal, same batch
    and N, all of the element type `dtype`."""
    terms = tuple(terms)
    for t in terms:
        if t.dtype != dtype:
            raise _hip.HipExtensionError(f"a {dtype} sum descriptor takes {dtype} terms only; got {t.dtype}")
    _check_dtype(dtype, d)
    if not 2 <= len(terms) <= _hip.LO_MAX_TERMS:
        raise ValueError(f"a lowered sum holds 2 .. {_hip.LO_MAX_TERMS} terms, got {len(terms)}")
    t0 = terms[0]
    for t in terms:
        if t.kind == _hip.LO_OP_SUM or t.diag_mode != _hip.LO_DIAG_NONE or (t.B, t.N) != (t0.B, t0.N):
            raise ValueError("sum terms must be plain structured operators of one batch and size")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_SUM, t0.B, t0.N, batch_shape=t0.batch_shape, terms=terms,
                                         dtype=dtype), d, const_diag)


def _flat(t: torch.Tensor, keep: int) -> torch.Tensor:
    """[*batch, <keep trailing dims>] -> contiguous [B, ...]."""
    t = t.contiguous()
    return t.reshape(-1, *t.shape[t.dim() - keep:])


def _byref(s):
    return None if s is None else C.byref(s)


def _launch(name: str, dev, *args, ws_bytes: Optional[int] = None, info=None, errors=()):
    """Enqueue the entry point `name` on the current stream of `dev`: tensors go as device pointers, `ws_bytes` adds the
    (workspace, its size) pair and `info` the result struct of a solver, which the entry points take in this order
    before the stream.  `errors`: what the Python callbacks of this call caught (_wrap_closure); such an exception is
    raised in place of the library's return code."""
    args = [_hip.ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    if ws_bytes is not None:
        ws = _hip.workspace(ws_bytes, dev)
        args += [_hip.ptr(ws), ws.numel()]
    if info is not None:
        args.append(C.byref(info))
    try:
        _hip.call(name, *args, _hip.stream_ptr(dev))
    finally:
        _reraise(*errors)


_NO_CLOSURE = (_hip.MATVEC_CB(), ())  # the NULL callback and the exceptions it caught


def _wrap_closure(fn: Callable, device, batch_shape, typestr: str = "<f4"):
    """Python closure (tensor [*batch_shape, N, c] -> tensor) as an lo_matvec_cb (`typestr` "<f8": lo_matvec_cb_f64)
    and the list its exceptions are kept in for _reraise."""
    err = []

    def cb(user, v_ptr, y_ptr, B, N, c, stream):
        try:
            v = _hip.as_tensor(v_ptr, (B, N, c), device, typestr)
            y = _hip.as_tensor(y_ptr, (B, N, c), device, typestr)
            y.copy_(fn(v.reshape(*batch_shape, N, c)).reshape(B, N, c))
            return 0
        except BaseException as e:  # noqa: BLE001 -- must not unwind through C
            err.append(e)
            return 1

    return _hip.MATVEC_CB(cb), err


def _reraise(*error_lists):
    """After a call that took Python callbacks: raise the first exception one of them caught."""
    for err in error_lists:
        for e in err:
            raise e


def _callback_desc(B: int, N: int) -> _hip.OpDesc:
    """The descriptor of an operator that is only a matvec callback."""
    s = _hip.OpDesc()
    s.kind, s.diag_mode, s.B, s.N, s.R, s.n2 = _hip.LO_OP_CALLBACK, _hip.LO_DIAG_NONE, B, N, 0, 0
    return s


def _dense_f64(A, diag, matvec_closure, batch_shape, B: int, N: int):
    """The dense operand (A [B, N, N], diag [B, N] or None) of the fp64 entry points; (None, None): the closure."""
    if A is not None:
        return (A.expand(*batch_shape, N, N).reshape(B, N, N).contiguous(),
                None if diag is None else diag.expand(*batch_shape, N).reshape(B, N).contiguous())
    if matvec_closure is None:
        raise ValueError("need a dense fp64 operator or a matvec closure")
    return None, None


def _f64_operator(lib, desc: "OperatorDescriptor", B: int, N: int, c: int, dev):
    """A float64 descriptor as the `matvec` of a float64 solver: (lo_matvec_desc_cb_f64 itself, its lo_f64_op_ctx as the
    user pointer, what has to stay alive for the call).  No Python runs per product."""
    if desc.B != B or desc.N != N:
        raise RuntimeError(f"the right-hand side (batch {B}, N {N}) does not match operator batch {desc.B}, N {desc.N}")
    s = desc.c_struct(torch.float64)
    ws = _hip.workspace(lib.lo_matvec_f64_workspace_bytes(C.byref(s), c), dev)
    ctx = _hip.F64OpCtx(C.pointer(s), ws.data_ptr(), ws.numel())
    return C.cast(lib.lo_matvec_desc_cb_f64, _hip.MATVEC_CB), C.cast(C.pointer(ctx), C.c_void_p), (s, ws, ctx)


def _f64_precond(lib, precond, batch_shape, B: int, N: int, c: int, dev):
    """The cached pair (Q [*b, N, k], noise [*b, N] | [*b, 1] | [*b], constant_diag) of the float64 Woodbury
    preconditioner as the `precond_cb` of a float64 solver (lo_precond_desc_cb_f64 and its lo_f64_precond_ctx)."""
    Q, noise, constant = precond
    _hip.require_hip(Q, noise, dtype=torch.float64)
    k = Q.shape[-1]
    Q3 = Q.expand(*batch_shape, N, k).reshape(B, N, k).contiguous()
    if constant:
        n2 = noise.reshape(*noise.shape, 1) if noise.dim() == len(Q.shape) - 2 else noise
        n2 = n2.expand(*batch_shape, 1).reshape(B).contiguous()
    else:
        n2 = noise.expand(*batch_shape, N).reshape(B, N).contiguous()
    ws = _hip.workspace(lib.lo_precond_f64_workspace_bytes(B, N, k, c), dev)
    ctx = _hip.F64PrecondCtx(Q3.data_ptr(), n2.data_ptr(), _hip.LO_DIAG_CONST if constant else _hip.LO_DIAG_FULL, k,
                             ws.data_ptr(), ws.numel())
    return C.cast(lib.lo_precond_desc_cb_f64, _hip.MATVEC_CB), C.cast(C.pointer(ctx), C.c_void_p), (Q3, n2, ws, ctx)


def _f64_operands(lib, A, diag, desc, matvec_closure, precond, precond_closure, bshape, B: int, N: int, c: int, dev):
    """The operator and the preconditioner of a float64 solver call, the one rule of cg_solve_f64, minres_solve_f64 and
    lanczos_tridiag_f64.  Operator: the float64 descriptor `desc` (lo_matvec_desc_cb_f64, inside the library), else the
    dense `A` (+ `diag`), else `matvec_closure`.  Preconditioner: the native pair `precond` (lo_precond_desc_cb_f64),
    else `precond_closure`, else none.  Returns (A3, d2, mv_cb, mv_user, pc_cb, pc_user, the error lists for _launch,
    what has to stay alive until the solver returns)."""
    A3 = d2 = mv_user = pc_user = mv_keep = pc_keep = None
    mv_err, (pc_cb, pc_err) = (), _NO_CLOSURE
    if desc is not None:
        mv_cb, mv_user, mv_keep = _f64_operator(lib, desc, B, N, c, dev)
    else:
        A3, d2 = _dense_f64(A, diag, matvec_closure, bshape, B, N)
        mv_cb, mv_err = _wrap_closure(matvec_closure, dev, bshape, "<f8") if A3 is None else _NO_CLOSURE
    if precond is not None:
        pc_cb, pc_user, pc_keep = _f64_precond(lib, precond, bshape, B, N, c, dev)
    elif precond_closure is not None:
        pc_cb, pc_err = _wrap_closure(precond_closure, dev, bshape, "<f8")
    return A3, d2, mv_cb, mv_user, pc_cb, pc_user, (mv_err, pc_err), (mv_keep, pc_keep)


def _f32_operator(desc: Optional["OperatorDescriptor"], matvec_closure, bshape, B: int, N: int, dev):
    """The operator of a float32 solver that takes a descriptor or a closure (MINRES, Lanczos): (the struct of `desc`,
    else of the callback descriptor; the closure's callback; the list its exceptions are kept in)."""
    if desc is not None:
        return (desc.c_struct(), *_NO_CLOSURE)
    if matvec_closure is None:
        raise ValueError("need an operator descriptor or a matvec closure")
    return (_callback_desc(B, N), *_wrap_closure(matvec_closure, dev, bshape))


def precond_apply_f64(Q: torch.Tensor, noise: torch.Tensor, constant_diag: bool, r: torch.Tensor) -> torch.Tensor:
    """z = r / d - Q (Q^T r) (or (r - Q Q^T r) / sigma, constant_diag) in float64: one call of lo_precond_desc_cb_f64, the
    function the float64 solvers call per iteration.  r [*batch, N, c]."""
    lib = _hip.load()
    _hip.require_hip(r, dtype=torch.float64)
    N, c = r.shape[-2:]
    r3 = _flat(r, 2)
    B = r3.shape[0]
    cb, user, keep = _f64_precond(lib, (Q, noise, constant_diag), tuple(r.shape[:-2]), B, N, c, r.device)
    z = torch.empty_like(r3)
    _hip.check(lib.lo_precond_desc_cb_f64(user, _hip.ptr(r3), _hip.ptr(z), B, N, c, _hip.stream_ptr(r.device)),
               "lo_precond_desc_cb_f64")
    del keep
    return z.reshape(r.shape)


def _diag_operand(d: torch.Tensor, B: int, N: int, const_diag: bool, want_dinv: bool = False):
    """(d flattened to [B] (constant) or [B, N], its LO_DIAG_* mode, an empty buffer of that shape for 1 / d or None)."""
    if const_diag:
        d2, mode = d.contiguous().reshape(-1), _hip.LO_DIAG_CONST
        assert d2.numel() == B, "constant diagonal must hold one value per batch member"
    else:
        d2, mode = _flat(d, 1), _hip.LO_DIAG_FULL
        assert d2.shape == (B, N)
    return d2, mode, (torch.empty_like(d2, dtype=torch.float32) if want_dinv else None)


def _row_strides(L3: torch.Tensor):
    """(member, row, column) strides of the factor L3 [B, N, k]; one member has no member stride."""
    sm, sr, sc = L3.stride()
    if L3.shape[0] == 1:
        sm = 0
    return sm, sr, sc


def lowrank_diag_descriptor(Croot: torch.Tensor, d: Optional[torch.Tensor], const_diag: bool = False,
                            dtype=torch.float32):
    _check_dtype(dtype, Croot, d)
    _hip.require_hip(Croot, d, dtype=dtype)
    batch = Croot.shape[:-2]
    N, R = Croot.shape[-2:]
    C3 = _flat(Croot, 2)
    return _with_diag(OperatorDescriptor(_hip.LO_OP_LOWRANK_DIAG, C3.shape[0], N, A0=C3, R=R, batch_shape=batch,
                                         dtype=dtype), d, const_diag)


def dense_diag_descriptor(K: torch.Tensor, d: Optional[torch.Tensor], const_diag: bool = False, dtype=torch.float32):
    _check_dtype(dtype, K, d)
    _hip.require_hip(K, d, dtype=dtype)
    batch = K.shape[:-2]
    N = K.shape[-1]
    K3 = _flat(K, 2)
    return _with_diag(OperatorDescriptor(_hip.LO_OP_DENSE_DIAG, K3.shape[0], N, A0=K3, batch_shape=batch, dtype=dtype),
                      d, const_diag)


def kron_diag_descriptor(K1: torch.Tensor, K2: torch.Tensor, d: Optional[torch.Tensor], const_diag: bool = False,
                         dtype=torch.float32):
    _check_dtype(dtype, K1, K2, d)
    _hip.require_hip(K1, K2, d, dtype=dtype)
    batch = K1.shape[:-2]
    n1, n2 = K1.shape[-1], K2.shape[-1]
    A = _flat(K1, 2)
    Bm = _flat(K2, 2)
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KRON_DIAG, A.shape[0], n1 * n2, A0=A, A1=Bm, R=n1, n2=n2,
                                         batch_shape=batch, dtype=dtype), d, const_diag)


def toeplitz_diag_descriptor(column: torch.Tensor, d: Optional[torch.Tensor], const_diag: bool = False):
    """AddedDiag(Toeplitz(column), Diag(d)) (or the Toeplitz operator alone): y = T v + d o v, column [*batch, M].
    None when M exceeds the native Toeplitz product's LO_TOEPLITZ_MAX_M (the caller takes the torch composition)."""
    _hip.require_hip(column, d)
    M = column.shape[-1]
    if M > _hip.LO_TOEPLITZ_MAX_M:
        return None
    col = _flat(column, 1)
    return _with_diag(OperatorDescriptor(_hip.LO_OP_TOEPLITZ_DIAG, col.shape[0], M, A0=col, R=M,
                                         batch_shape=column.shape[:-1]), d, const_diag)


def ski_diag_descriptor(column: torch.Tensor, left_idx: torch.Tensor, left_vals: torch.Tensor,
                        right_idx: torch.Tensor, right_vals: torch.Tensor, d: Optional[torch.Tensor],
                        const_diag: bool = False, right_plan: Optional[torch.Tensor] = None):
    """AddedDiag(Interpolated(Toeplitz(column), W_l, W_r), Diag(d)): y = W_l T W_r^T v + d o v.  column [*batch, M],
    indices int64 / values fp32 [*batch, N, J] (one batch shape for all, square: both sides N rows).  None when the
    shapes are outside what the kind takes.  `right_plan`: interp_plan(right_idx, M) of the same batch, kept by the
    caller (else every matvec / solve builds the grid-major copy of W_r itself)."""
    _hip.require_hip(column, left_vals, right_vals, d)
    batch = column.shape[:-1]
    M = column.shape[-1]
    N, J = left_idx.shape[-2:]
    if (M > _hip.LO_TOEPLITZ_MAX_M or right_idx.shape[-2:] != (N, J) or left_idx.dtype != torch.int64
            or right_idx.dtype != torch.int64 or not left_idx.is_cuda or not right_idx.is_cuda):
        return None
    col = _flat(column, 1)
    B = col.shape[0]

    def flat(t):
        return t.expand(*batch, N, J).contiguous().reshape(B, N, J)

    li, lv = flat(left_idx), flat(left_vals)
    shared = right_idx is left_idx and right_vals is left_vals  # (one copy: the kernels read the same arrays twice)
    ri, rv = (li, lv) if shared else (flat(right_idx), flat(right_vals))
    return _with_diag(OperatorDescriptor(_hip.LO_OP_SKI_DIAG, B, N, A0=col, R=M, n2=J, batch_shape=batch,
                                         interp=(li, lv, ri, rv), interp_plan=right_plan), d, const_diag)


def ski_sum_diag_descriptor(cols: torch.Tensor, left_idx: torch.Tensor, left_vals: torch.Tensor,
                            right_idx: torch.Tensor, right_vals: torch.Tensor, d: Optional[torch.Tensor],
                            const_diag: bool = False, right_plan: Optional[torch.Tensor] = None):
    """AddedDiag(SumBatch(Interpolated(Toeplitz(cols), W_l, W_r)), Diag(d)), the additive SKI model:
    y = sum_p W_l,p T_p W_r,p^T v + d o v.  cols [*batch, P, M], indices int64 / values fp32 [*batch, P, N, J] (the base
    operator's own tensors: the summed dimension is its last batch dimension), d [*batch, N] or [*batch].  None when the
    shapes are outside what the kind takes.  `right_plan`: interp_plan(right_idx, (*batch, P), M), kept by the caller
    (else every matvec / solve builds the grid-major copy of W_r itself)."""
    _hip.require_hip(cols, left_vals, right_vals, d)
    batch = cols.shape[:-2]
    P, M = cols.shape[-2:]
    N, J = left_idx.shape[-2:]
    B = math.prod(batch)
    if (M > _hip.LO_TOEPLITZ_MAX_M or not 1 <= P <= _hip.LO_SKI_SUM_MAX_TERMS or B * P > 65535
            or right_idx.shape[-2:] != (N, J) or left_idx.dtype != torch.int64 or right_idx.dtype != torch.int64
            or not left_idx.is_cuda or not right_idx.is_cuda):
        return None
    col = cols.contiguous().reshape(B, P, M)

    def flat(t):
        return t.expand(*batch, P, N, J).contiguous().reshape(B, P, N, J)

    li, lv = flat(left_idx), flat(left_vals)
    shared = right_idx is left_idx and right_vals is left_vals  # (one copy: the kernels read the same arrays twice)
    ri, rv = (li, lv) if shared else (flat(right_idx), flat(right_vals))
    return _with_diag(OperatorDescriptor(_hip.LO_OP_SKI_SUM_DIAG, B, N, A0=col, R=M, n2=J, batch_shape=batch,
                                         interp=(li, lv, ri, rv), interp_plan=right_plan, kernel_terms=P), d, const_diag)


# Memo of the concatenated columns of a Kronecker-of-Toeplitz base, keyed on the factors' column tensors (address, version
# counter, layout) and the batch they were expanded to: every lowering of one operator then hands the kernels the SAME
# tensor (the preconditioner cache recognises its operator by that address), and the small copy is made once.  The entry
# keeps the columns alive, so no address is reused while it exists; an in-place update bumps the version counter.
SKI_GRID_COLS_MEMO_SIZE = 4
_ski_grid_cols_memo: "list[tuple]" = []


def _ski_grid_columns(cols, batch) -> torch.Tensor:
    """[B, M_1 + .. + M_D] fp32: the factors' first columns [*b_k, M_k] expanded to `batch` and concatenated per member."""
    keyed = not any(t.is_inference() for t in cols)
    key = None
    if keyed:
        key = (tuple((t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride())) for t in cols), tuple(batch))
    if keyed:
        for entry in _ski_grid_cols_memo:
            if entry[0] == key:
                return entry[2]
    with torch.no_grad():
        cat = torch.cat([t.detach().expand(*batch, t.shape[-1]).reshape(-1, t.shape[-1]) for t in cols], -1).contiguous()
    if keyed:
        _ski_grid_cols_memo.insert(0, (key, tuple(cols), cat))
        del _ski_grid_cols_memo[SKI_GRID_COLS_MEMO_SIZE:]
    return cat


def clear_ski_grid_memo():
    _ski_grid_cols_memo.clear()


def ski_grid_shape_ok(grid) -> bool:
    """Whether the native grid product takes a grid of this shape: 2 or 3 axes of at most LO_SKI_GRID_MAX_AXIS points,
    at most LO_SKI_GRID_MAX_M points in all."""
    return (len(grid) in (2, 3) and all(1 <= m <= _hip.LO_SKI_GRID_MAX_AXIS for m in grid)
            and math.prod(grid) <= _hip.LO_SKI_GRID_MAX_M)


def ski_grid_diag_descriptor(cols, left_idx: torch.Tensor, left_vals: torch.Tensor, right_idx: torch.Tensor,
                             right_vals: torch.Tensor, d: Optional[torch.Tensor], const_diag: bool = False,
                             right_plan: Optional[torch.Tensor] = None):
    """AddedDiag(Interpolated(Kron(Toeplitz(cols[0]), .., Toeplitz(cols[D-1])), W_l, W_r), Diag(d)), D = 2 or 3:
    y = W_l (T_1 (x) .. (x) T_D) W_r^T v + d o v.  cols[k] [*b_k, M_k] (batch shapes that broadcast to the indices'),
    indices int64 / values fp32 [*batch, N, J] into the grid of M = prod M_k points, g = (g_1 M_2 + g_2) M_3 + g_3.  The
    columns are concatenated once per (columns, batch) and memoised.  None when the shapes are outside what the kind
    takes."""
    cols = list(cols)
    _hip.require_hip(*cols, left_vals, right_vals, d)
    grid = tuple(int(t.shape[-1]) for t in cols)
    batch = left_idx.shape[:-2]
    N, J = left_idx.shape[-2:]
    if (not ski_grid_shape_ok(grid) or right_idx.shape[-2:] != (N, J) or right_idx.shape[:-2] != batch
            or left_idx.dtype != torch.int64 or right_idx.dtype != torch.int64 or not left_idx.is_cuda
            or not right_idx.is_cuda):
        return None
    col = _ski_grid_columns(cols, batch)
    B = col.shape[0]

    def flat(t):
        return t.expand(*batch, N, J).contiguous().reshape(B, N, J)

    li, lv = flat(left_idx), flat(left_vals)
    shared = right_idx is left_idx and right_vals is left_vals
    ri, rv = (li, lv) if shared else (flat(right_idx), flat(right_vals))
    return _with_diag(OperatorDescriptor(_hip.LO_OP_SKI_GRID_DIAG, B, N, A0=col, R=math.prod(grid), n2=J,
                                         batch_shape=batch, interp=(li, lv, ri, rv), interp_plan=right_plan, grid=grid),
                      d, const_diag)


def toeplitz_kron_diag_descriptor(cols, d: Optional[torch.Tensor], const_diag: bool = False):
    """AddedDiag(Kron(Toeplitz(cols[0]), .., Toeplitz(cols[D-1])), Diag(d)) (or the product alone), D = 2 or 3:
    y = (T_1 (x) .. (x) T_D) v + d o v.  cols[k] [*b_k, M_k] of batch shapes that broadcast; the columns are concatenated
    once per (columns, batch) and memoised (_ski_grid_columns).  None when the grid is outside what the kind takes."""
    cols = list(cols)
    _hip.require_hip(*cols, d)
    grid = tuple(int(t.shape[-1]) for t in cols)
    if not ski_grid_shape_ok(grid):
        return None
    batch = torch.broadcast_shapes(*(t.shape[:-1] for t in cols))
    col = _ski_grid_columns(cols, batch)
    M = math.prod(grid)
    return _with_diag(OperatorDescriptor(_hip.LO_OP_TOEPLITZ_KRON_DIAG, col.shape[0], M, A0=col, R=M,
                                         batch_shape=torch.Size(batch), grid=grid), d, const_diag)


def toeplitz_kron_bilinear(cols, u: torch.Tensor, v: torch.Tensor):
    """Per-factor column gradients of sum_s u_s^T (T_1 (x) .. (x) T_D) v_s (lo_toeplitz_kron_bilinear_f32): cols[k]
    [B, M_k], D = 2 or 3; u, v [B, M, S].  Returns the list of g_k [B, M_k].  A shape the kernels do not take raises."""
    lib = _hip.load()
    cols = [t.contiguous() for t in cols]
    _hip.require_hip(*cols, u, v)
    grid = [int(t.shape[-1]) for t in cols]
    B, M, S = u.shape
    if any(t.dim() != 2 or t.shape[0] != B for t in cols) or math.prod(grid) != M or v.shape != u.shape:
        raise RuntimeError(f"toeplitz_kron_bilinear: columns of sizes {[tuple(t.shape) for t in cols]} for u "
                           f"{tuple(u.shape)}, v {tuple(v.shape)}")
    t = torch.cat(cols, -1).contiguous()
    u, v = u.contiguous(), v.contiguous()
    g = torch.empty(B, sum(grid), dtype=torch.float32, device=u.device)
    m = (C.c_int64 * len(grid))(*grid)
    _launch("lo_toeplitz_kron_bilinear_f32", u.device, t, m, len(grid), B, u, v, S, g,
            ws_bytes=lib.lo_toeplitz_kron_bilinear_workspace_bytes(m, len(grid), B, S))
    return list(g.split(grid, -1))


def toeplitz_kron_mv(cols, u: torch.Tensor) -> torch.Tensor:
    """(T_1 (x) .. (x) T_D) u for the symmetric Toeplitz matrices of cols[k] [B, M_k], D = 2 or 3; u [B, M, c] with
    M = prod M_k and the grid index g = (g_1 M_2 + g_2) M_3 + g_3 (lo_toeplitz_kron_mv_f32).  A shape the kernel does
    not take raises."""
    lib = _hip.load()
    cols = [t.contiguous() for t in cols]
    _hip.require_hip(*cols, u)
    grid = [int(t.shape[-1]) for t in cols]
    B, M, c = u.shape
    if any(t.dim() != 2 or t.shape[0] != B for t in cols) or math.prod(grid) != M:
        raise RuntimeError(f"toeplitz_kron_mv: columns of sizes {[tuple(t.shape) for t in cols]} for u {tuple(u.shape)}")
    t = torch.cat(cols, -1).contiguous()
    u = u.contiguous()
    y = torch.empty_like(u)
    m = (C.c_int64 * len(grid))(*grid)
    _launch("lo_toeplitz_kron_mv_f32", u.device, t, m, len(grid), B, u, c, y,
            ws_bytes=lib.lo_toeplitz_kron_workspace_bytes(m, len(grid), B, c))
    return y


def hadamard_diag_descriptor(F: torch.Tensor, G: torch.Tensor, d: Optional[torch.Tensor], const_diag: bool = False):
    """AddedDiag(Mul(Root(F), Root(G)), Diag(d)) (or the product alone): y = (F F^T o G G^T) v + d o v
    (mul_linear_operator.py:54-80).  F [*batch, N, p], G [*batch, N, q] of one batch shape.  None when a rank exceeds
    LO_HADAMARD_MAX_RANK (the caller takes the torch composition)."""
    _hip.require_hip(F, G, d)
    if F.shape[-1] > _hip.LO_HADAMARD_MAX_RANK or G.shape[-1] > _hip.LO_HADAMARD_MAX_RANK:
        return None
    batch = F.shape[:-2]
    N, p = F.shape[-2:]
    F3, G3 = _flat(F, 2), _flat(G, 2)
    return _with_diag(OperatorDescriptor(_hip.LO_OP_HADAMARD_DIAG, F3.shape[0], N, A0=F3, A1=G3, R=p, n2=G.shape[-1],
                                         batch_shape=batch), d, const_diag)


def kernel_theta(lengthscale: torch.Tensor, outputscale: torch.Tensor, batch, D: int,
                 dtype=torch.float32) -> torch.Tensor:
    """theta [B, D + 1] of the kernel entry points, of element type `dtype`: the D inverse lengthscales (a shared one
    replicated), then outputscale^2.  lengthscale [*b, 1, D] or [*b, 1, 1], outputscale [*b], both broadcast to `batch`."""
    with torch.no_grad():
        inv = (1.0 / lengthscale.detach()).expand(*batch, 1, D).reshape(-1, D)
        os2 = torch.broadcast_to(outputscale.detach().square(), tuple(batch)).reshape(-1, 1)
        return torch.cat((inv, os2), -1).to(dtype).contiguous()


def _kernel_dtype(what: str, *tensors):
    """The one element type of a kernel entry point's operands (float32: the _f32 entry point, float64: its _f64 twin);
    mixed types raise."""
    dtype = tensors[0].dtype
    for t in tensors:
        if t is not None and t.dtype != dtype:
            dtype = None
    if dtype != torch.float32 and dtype != torch.float64:
        raise _hip.HipExtensionError(f"{what}: the operands must all be float32 or all be float64, got "
                                     f"{sorted({str(t.dtype) for t in tensors if t is not None})}")
    return dtype


def _kernel_args(what, x1, x2, theta, right, left=None, d=None, task=None, families=None, ids=0, block=1, twin=False,
                 width=None):
    """The checked operands of an entry point of the matrix-free kernel family: the points x1 [B, M, D] and x2 [B, N, D]
    (`ids` = 1: one more column, the task id), theta [B, `width`] (None: D + 1; with `families`, the T codes of a sum:
    [B, T, D + 1]), `task` = Bt [B, T, T] or None, the right operand [B, N block, cols] and, for the derivatives, the
    left one [B, M block, cols] (`block` rows per point: T of the Kronecker kind, D + 1 of the gradient kind).  They are
    made contiguous and, like the diagonal `d`, must be HIP tensors of one element type: float32, or all float64 where
    the kind has _f64 twins (`twin`).  Returns (x1, x2, theta, extra, left, right, (B, M, N, D, T, cols), dtype) with
    extra = Bt, or the families as the int32 array the sum's entry points take, or None.  `families` and `task` together
    are the LMC kind over one point tensor: Bt [B, Q, T, T], extra the packed family codes and Q in the place of T."""
    x1, x2, theta, right = x1.contiguous(), x2.contiguous(), theta.contiguous(), right.contiguous()
    if left is not None:
        left = left.contiguous()
    extra, T, tasks = None, 0, ()
    if task is not None:
        extra = task = task.contiguous()
        T = task.shape[-1]
        tasks = (T, T)
    dtype = _kernel_dtype(what, x1, x2, theta, right, left, task, d) if twin else torch.float32
    _hip.require_hip(x1, x2, theta, right, left, task, d, dtype=dtype)
    if families is not None:
        packed = kernel_sum_pack_families(families)
        T = len(families)
        tasks = (T, *tasks)
        extra = (C.c_int32 * T)(*[int(f) for f in families]) if task is None else packed
    B, M, D = x1.shape
    N = x2.shape[-2] if x2.dim() == 3 else -1
    cols = right.shape[-1]
    if (x2.shape != (B, N, D) or theta.shape != ((B, width or D + 1 - ids) if families is None else (B, T, D + 1))
            or right.shape != (B, N * block, cols) or (left is not None and left.shape != (B, M * block, cols))
            or (task is not None and task.shape != (B, *tasks))):
        points = (f"x1 {tuple(x1.shape)}, x2 {tuple(x2.shape)}" if task is None or families is None
                  else f"x {tuple(x1.shape)}")
        raise RuntimeError(f"{what}: {points}, theta {tuple(theta.shape)}"
                           + (f" for {T} terms" if families is not None else "")
                           + (f", task {tuple(task.shape)}" if task is not None else "")
                           + (f", left operand {tuple(left.shape)}" if left is not None else "")
                           + f", right operand {tuple(right.shape)}")
    return x1, x2, theta, extra, left, right, (B, M, N, D - ids, T, cols), dtype


def _kernel_diag(d: Optional[torch.Tensor], B: int, rows: int, const_diag: bool):
    """(d as a product's entry point takes it, its LO_DIAG_* mode); without d: (None, LO_DIAG_NONE)."""
    if d is None:
        return None, _hip.LO_DIAG_NONE
    return _diag_operand(d, B, rows, const_diag)[:2]


@functools.lru_cache(maxsize=None)
def _kernel_entry(stem: str, f64: bool):
    """(name of the entry point `stem`_f32 or, float64, `stem`_f64 of the kernel family, its workspace sizer)."""
    sizer = getattr(_hip.load(), f"{stem}_f64_workspace_bytes" if f64 else f"{stem}_workspace_bytes")
    return (f"{stem}_f64" if f64 else f"{stem}_f32"), sizer


def kernel_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, family: int, d: Optional[torch.Tensor] = None,
                           const_diag: bool = False, dtype=torch.float32):
    """AddedDiag(Kernel(X, X, family), Diag(d)) (or the kernel matrix alone): y = K(X, X) v + d o v with K formed on the
    fly (csrc/lo_kernel_op.hip; dtype=torch.float64: csrc/lo_kernel_op_f64.hip through lo_matvec_f64 and the float64
    solvers).  X [*batch, N, D], theta [B, D + 1] from kernel_theta.  None when D exceeds LO_KERNEL_MAX_DIM (the caller
    evaluates covar_func)."""
    _check_dtype(dtype, X, theta, d)
    _hip.require_hip(X, theta, d, dtype=dtype)
    N, D = X.shape[-2:]
    if D > _hip.LO_KERNEL_MAX_DIM or D < 1:
        return None
    X3 = _flat(X.detach(), 2)
    if theta.shape != (X3.shape[0], D + 1):
        raise RuntimeError(f"kernel_diag_descriptor: theta of shape {tuple(theta.shape)} for X {tuple(X.shape)}")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_DIAG, X3.shape[0], N, A0=X3, A1=theta, R=D, n2=int(family),
                                         batch_shape=X.shape[:-2], dtype=dtype), d, const_diag)


def kernel_mv(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, v: torch.Tensor,
              d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_mv_f32 (all operands float64: lo_kernel_mv_f64): y [B, M, c] = K(x1, x2) v (+ d o v when M == N and d is
    given), x1 [B, M, D], x2 [B, N, D], theta [B, D + 1], v [B, N, c].  A shape the kernel does not take raises."""
    x1, x2, theta, _, _, v, (B, M, N, D, _, c), dtype = _kernel_args("kernel_mv", x1, x2, theta, v, d=d, twin=True)
    d, mode = _kernel_diag(d, B, N, const_diag)
    y = torch.empty(B, M, c, dtype=dtype, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_mv", dtype == torch.float64)
    _launch(name, v.device, x1, x2, theta, int(family), B, M, N, D, v, c, d, mode, y, ws_bytes=sizer(B, M, N, D, c))
    return y


def kernel_bilinear(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, U: torch.Tensor,
                    V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_bilinear_f32 (all operands float64: lo_kernel_bilinear_f64): g_theta [B, D + 1], the derivative of
    sum_s u_s^T K(x1, x2) v_s with respect to theta (the inverse lengthscales, then outputscale^2).  x1 [B, M, D],
    x2 [B, N, D], U [B, M, t], V [B, N, t]."""
    x1, x2, theta, _, U, V, (B, M, N, D, _, t), dtype = _kernel_args("kernel_bilinear", x1, x2, theta, V, U, twin=True)
    g = torch.empty(B, D + 1, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_bilinear", dtype == torch.float64)
    _launch(name, U.device, x1, x2, theta, int(family), B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, t))
    return g


def kernel_points_grad(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, U: torch.Tensor,
                       V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_points_grad_f32 (all operands float64: lo_kernel_points_grad_f64): g_x1 [B, M, D], the derivative of
    sum_s u_s^T K(x1, x2) v_s with respect to x1, x2 held fixed.  x1 [B, M, D], x2 [B, N, D], theta [B, D + 1],
    U [B, M, t], V [B, N, t].  The derivative with respect to x2 is kernel_points_grad(x2, x1, theta, family, V, U)."""
    x1, x2, theta, _, U, V, (B, M, N, D, _, t), dtype = _kernel_args("kernel_points_grad", x1, x2, theta, V, U,
                                                                        twin=True)
    g = torch.empty(B, M, D, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_points_grad", dtype == torch.float64)
    _launch(name, U.device, x1, x2, theta, int(family), B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, t))
    return g


def kernel_param_theta(lengthscale: torch.Tensor, outputscale: torch.Tensor, batch, D: int,
                       alpha: Optional[torch.Tensor] = None, period_length: Optional[torch.Tensor] = None) -> torch.Tensor:
    """theta [B, 2 D + 2] of the lo_kernel_param_* entry points: the D inverse lengthscales (a shared one replicated),
    outputscale^2, alpha (rational quadratic; else 0), the D inverse periods (periodic, a shared one replicated; else 0).
    lengthscale, period_length [*b, 1, D] or [*b, 1, 1], outputscale, alpha [*b], all broadcast to `batch`."""
    with torch.no_grad():
        head = kernel_theta(lengthscale, outputscale, batch, D)
        B = head.shape[0]
        al = (torch.zeros(B, 1, dtype=head.dtype, device=head.device) if alpha is None
              else torch.broadcast_to(alpha.detach(), tuple(batch)).reshape(-1, 1).to(head.dtype))
        nu = (torch.zeros(B, D, dtype=head.dtype, device=head.device) if period_length is None
              else (1.0 / period_length.detach()).expand(*batch, 1, D).reshape(-1, D).to(head.dtype))
        return torch.cat((head, al, nu), -1).contiguous()


def _kernel_param_family(what: str, family) -> int:
    if int(family) not in (_hip.LO_KERNEL_RQ, _hip.LO_KERNEL_PERIODIC):
        raise ValueError(f"{what}: family {family} is neither LO_KERNEL_RQ nor LO_KERNEL_PERIODIC")
    return int(family)


def kernel_param_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, family: int, d: Optional[torch.Tensor] = None,
                                 const_diag: bool = False):
    """AddedDiag(ParamKernel(X, X, family), Diag(d)) (or the kernel matrix alone), family LO_KERNEL_RQ or
    LO_KERNEL_PERIODIC: y = K(X, X) v + d o v with K formed on the fly (csrc/lo_kernel_param.hip), the kind
    LO_OP_KERNEL_PARAM_DIAG.  X [*batch, N, D], theta [B, 2 D + 2] from kernel_param_theta.  None when D exceeds
    LO_KERNEL_PARAM_MAX_DIM or the batch the sweep's grid (the caller evaluates covar_func)."""
    _hip.require_hip(X, theta, d)
    N, D = X.shape[-2:]
    X3 = _flat(X.detach(), 2)
    if (D > _hip.LO_KERNEL_PARAM_MAX_DIM or D < 1 or X3.shape[0] > 65535
            or int(family) not in (_hip.LO_KERNEL_RQ, _hip.LO_KERNEL_PERIODIC)):
        return None
    if theta.shape != (X3.shape[0], 2 * D + 2):
        raise RuntimeError(f"kernel_param_diag_descriptor: theta of shape {tuple(theta.shape)} for X {tuple(X.shape)}")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_PARAM_DIAG, X3.shape[0], N, A0=X3, A1=theta.contiguous(), R=D,
                                         n2=int(family), batch_shape=X.shape[:-2]), d, const_diag)


def kernel_param_mv(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, v: torch.Tensor,
                    d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_param_mv_f32: y [B, M, c] = K(x1, x2) v (+ d o v; d only when M == N), x1 [B, M, D], x2 [B, N, D], theta
    [B, 2 D + 2], v [B, N, c].  A shape the kernel does not take raises."""
    family = _kernel_param_family("kernel_param_mv", family)
    x1, x2, theta, _, _, v, (B, M, N, D, _, c), dtype = _kernel_args("kernel_param_mv", x1, x2, theta, v, d=d,
                                                                      width=2 * x1.shape[-1] + 2)
    d, mode = _kernel_diag(d, B, N, const_diag)
    y = torch.empty(B, M, c, dtype=dtype, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_param_mv", False)
    _launch(name, v.device, x1, x2, theta, family, B, M, N, D, v, c, d, mode, y, ws_bytes=sizer(B, M, N, D, c))
    return y


def kernel_param_bilinear(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, U: torch.Tensor,
                          V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_param_bilinear_f32: g_theta [B, 2 D + 2], the derivative of sum_s u_s^T K(x1, x2) v_s with respect to every
    entry of theta (0 where the family does not read the entry).  x1 [B, M, D], x2 [B, N, D], U [B, M, t], V [B, N, t]."""
    family = _kernel_param_family("kernel_param_bilinear", family)
    x1, x2, theta, _, U, V, (B, M, N, D, _, t), dtype = _kernel_args("kernel_param_bilinear", x1, x2, theta, V, U,
                                                                      width=2 * x1.shape[-1] + 2)
    g = torch.empty(B, 2 * D + 2, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_param_bilinear", False)
    _launch(name, U.device, x1, x2, theta, family, B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, t))
    return g


def kernel_param_points_grad(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, U: torch.Tensor,
                             V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_param_points_grad_f32: g_x1 [B, M, D], the derivative of sum_s u_s^T K(x1, x2) v_s with respect to x1, x2
    held fixed.  The derivative with respect to x2 is kernel_param_points_grad(x2, x1, theta, family, V, U)."""
    family = _kernel_param_family("kernel_param_points_grad", family)
    x1, x2, theta, _, U, V, (B, M, N, D, _, t), dtype = _kernel_args("kernel_param_points_grad", x1, x2, theta, V, U,
                                                                      width=2 * x1.shape[-1] + 2)
    g = torch.empty(B, M, D, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_param_points_grad", False)
    _launch(name, U.device, x1, x2, theta, family, B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, t))
    return g


def kernel_sm_theta(weights: torch.Tensor, means: torch.Tensor, scales: torch.Tensor, batch, D: int) -> torch.Tensor:
    """theta [B, Q, 2 D + 1] of the lo_kernel_sm_* entry points: per mixture the weight, the D means, the D scales, raw
    values (no inverses).  weights [*b, Q], means and scales [*b, Q, D], all broadcast to `batch`."""
    with torch.no_grad():
        Q = weights.shape[-1]
        w = weights.detach().expand(*batch, Q).reshape(-1, Q, 1)
        mu = means.detach().expand(*batch, Q, D).reshape(-1, Q, D)
        sg = scales.detach().expand(*batch, Q, D).reshape(-1, Q, D)
        return torch.cat((w, mu, sg), -1).to(torch.float32).contiguous()


def _kernel_sm_args(what, x1, x2, theta, right, left=None, d=None):
    """_kernel_args for theta [B, Q, 2 D + 1]: the checked operands and (B, M, N, D, Q, cols)."""
    if theta.dim() != 3 or theta.shape[-1] != 2 * x1.shape[-1] + 1 or theta.shape[-2] < 1:
        raise RuntimeError(f"{what}: theta of shape {tuple(theta.shape)} for x1 {tuple(x1.shape)}")
    Q = theta.shape[-2]
    x1, x2, flat, _, left, right, (B, M, N, D, _, cols), _ = _kernel_args(what, x1, x2, theta.reshape(theta.shape[0], -1),
                                                                         right, left, d=d, width=Q * theta.shape[-1])
    return x1, x2, flat, left, right, (B, M, N, D, Q, cols)


def kernel_sm_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, d: Optional[torch.Tensor] = None,
                              const_diag: bool = False):
    """AddedDiag(SM(X, X), Diag(d)) (or the kernel matrix alone): y = K(X, X) v + d o v with the spectral mixture K formed
    on the fly (csrc/lo_kernel_sm.hip), the kind LO_OP_KERNEL_SM_DIAG.  X [*batch, N, D], theta [B, Q, 2 D + 1] from
    kernel_sm_theta.  None when D or Q exceeds LO_KERNEL_SM_MAX_DIM / LO_KERNEL_SM_MAX_MIX or the batch the sweep's grid
    (the caller evaluates covar_func)."""
    _hip.require_hip(X, theta, d)
    N, D = X.shape[-2:]
    X3 = _flat(X.detach(), 2)
    Q = theta.shape[-2] if theta.dim() == 3 else 0
    if (D > _hip.LO_KERNEL_SM_MAX_DIM or D < 1 or Q > _hip.LO_KERNEL_SM_MAX_MIX or X3.shape[0] > 65535):
        return None
    if theta.shape != (X3.shape[0], Q, 2 * D + 1) or Q < 1:
        raise RuntimeError(f"kernel_sm_diag_descriptor: theta of shape {tuple(theta.shape)} for X {tuple(X.shape)}")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_SM_DIAG, X3.shape[0], N, A0=X3, A1=theta.contiguous(), R=D,
                                         n2=Q, batch_shape=X.shape[:-2]), d, const_diag)


def kernel_sm_mv(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, v: torch.Tensor,
                 d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_sm_mv_f32: y [B, M, c] = K(x1, x2) v (+ d o v; d only when M == N), x1 [B, M, D], x2 [B, N, D], theta
    [B, Q, 2 D + 1], v [B, N, c].  A shape the kernel does not take raises."""
    x1, x2, theta, _, v, (B, M, N, D, Q, c) = _kernel_sm_args("kernel_sm_mv", x1, x2, theta, v, d=d)
    d, mode = _kernel_diag(d, B, N, const_diag)
    y = torch.empty(B, M, c, dtype=torch.float32, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_sm_mv", False)
    _launch(name, v.device, x1, x2, theta, Q, B, M, N, D, v, c, d, mode, y, ws_bytes=sizer(B, M, N, D, Q, c))
    return y


def kernel_sm_bilinear(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, U: torch.Tensor,
                       V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_sm_bilinear_f32: g_theta [B, Q, 2 D + 1], the derivative of sum_s u_s^T K(x1, x2) v_s with respect to every
    entry of theta, in theta's layout.  x1 [B, M, D], x2 [B, N, D], U [B, M, t], V [B, N, t]."""
    x1, x2, theta, U, V, (B, M, N, D, Q, t) = _kernel_sm_args("kernel_sm_bilinear", x1, x2, theta, V, U)
    g = torch.empty(B, Q, 2 * D + 1, dtype=torch.float32, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_sm_bilinear", False)
    _launch(name, U.device, x1, x2, theta, Q, B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, Q, t))
    return g


def kernel_sm_points_grad(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, U: torch.Tensor,
                          V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_sm_points_grad_f32: g_x1 [B, M, D], the derivative of sum_s u_s^T K(x1, x2) v_s with respect to x1, x2 held
    fixed.  The derivative with respect to x2 is kernel_sm_points_grad(x2, x1, theta, V, U)."""
    x1, x2, theta, U, V, (B, M, N, D, Q, t) = _kernel_sm_args("kernel_sm_points_grad", x1, x2, theta, V, U)
    g = torch.empty(B, M, D, dtype=torch.float32, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_sm_points_grad", False)
    _launch(name, U.device, x1, x2, theta, Q, B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, Q, t))
    return g


def kernel_sum_theta(lengthscales, outputscales, batch, D: int) -> torch.Tensor:
    """theta [B, T, D + 1] of the fused kernel-sum entry points: per term the D inverse lengthscales (a shared one
    replicated), then outputscale^2 -- kernel_theta of every term, stacked in term order."""
    return torch.stack([kernel_theta(ls, os_, batch, D) for ls, os_ in zip(lengthscales, outputscales)], 1).contiguous()


def kernel_sum_pack_families(families) -> int:
    """The family codes as the descriptor's n2: four bits per term, term 0 lowest."""
    families = [int(f) for f in families]
    if not 1 <= len(families) <= _hip.LO_KERNEL_MAX_TERMS:
        raise ValueError(f"a fused kernel sum holds 1 .. {_hip.LO_KERNEL_MAX_TERMS} terms, got {len(families)}")
    if any(not _hip.LO_KERNEL_RBF <= f <= _hip.LO_KERNEL_MATERN52 for f in families):
        raise ValueError(f"unknown kernel family among {families}")
    return sum(f << (4 * t) for t, f in enumerate(families))


# Which derivative calls of a sum of kernel operators over one pair of point tensors are fused, from tools/mb_kernel_sum.py
# on the MI355X (fused / per-term time, T = 2 and 3, t = 1 and 17):
#   theta   D 4: 0.86 - 0.97   D 16: 1.09 - 1.12      points   D 4, T 3: 0.96 - 0.98   D 4, T 2: 1.04 - 1.05   D 16: 1.13 - 1.21
# The fused sweep forms W_ij once for all terms; beyond D = 4 the distances outweigh that and the term loop costs more
# than it saves.  A cell that was not measured (4 < D < 16, T = 4) takes the side of its nearest measured neighbour.
def kernel_sum_fused_bilinear(D: int, T: int) -> bool:
    return T >= 2 and D <= 4


def kernel_sum_fused_points_grad(D: int, T: int) -> bool:
    return T >= 3 and D <= 4


def kernel_sum_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, families, d: Optional[torch.Tensor] = None,
                               const_diag: bool = False):
    """AddedDiag(Kernel_1(X, X) + .. + Kernel_T(X, X), Diag(d)) (or the sum alone) over ONE point tensor:
    y = (sum_t K_t) v + d o v, all terms formed in one pass (csrc/lo_kernel_sum.hip).  X [*batch, N, D],
    theta [B, T, D + 1] from kernel_sum_theta, `families` the T codes.  None when D exceeds LO_KERNEL_MAX_DIM."""
    _hip.require_hip(X, theta, d)
    N, D = X.shape[-2:]
    if D > _hip.LO_KERNEL_MAX_DIM or D < 1:
        return None
    packed = kernel_sum_pack_families(families)
    T = len(families)
    X3 = _flat(X.detach(), 2)
    if theta.shape != (X3.shape[0], T, D + 1):
        raise RuntimeError(f"kernel_sum_diag_descriptor: theta of shape {tuple(theta.shape)} for X {tuple(X.shape)}, "
                           f"{T} terms")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_SUM_DIAG, X3.shape[0], N, A0=X3, A1=theta.contiguous(), R=D,
                                         n2=packed, batch_shape=X.shape[:-2], kernel_terms=T), d, const_diag)


def kernel_sum_mv(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, families, v: torch.Tensor,
                  d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_sum_mv_f32: y [B, M, c] = (sum_t K_t(x1, x2)) v (+ d o v when M == N and d is given), x1 [B, M, D],
    x2 [B, N, D], theta [B, T, D + 1], `families` the T codes, v [B, N, c].  A shape the kernel does not take raises."""
    x1, x2, theta, fams, _, v, (B, M, N, D, T, c), dtype = _kernel_args("kernel_sum_mv", x1, x2, theta, v, d=d,
                                                                         families=families)
    d, mode = _kernel_diag(d, B, N, const_diag)
    y = torch.empty(B, M, c, dtype=dtype, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_sum_mv", dtype == torch.float64)
    _launch(name, v.device, x1, x2, theta, fams, T, B, M, N, D, v, c, d, mode, y, ws_bytes=sizer(B, M, N, D, T, c))
    return y


def kernel_sum_bilinear(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, families, U: torch.Tensor,
                        V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_sum_bilinear_f32: g_theta [B, T, D + 1], every term's derivative of sum_s u_s^T K(x1, x2) v_s with
    respect to its theta, W_ij = sum_s U[i, s] V[j, s] formed once per pair.  U [B, M, t], V [B, N, t]."""
    x1, x2, theta, fams, U, V, (B, M, N, D, T, t), dtype = _kernel_args("kernel_sum_bilinear", x1, x2, theta, V, U,
                                                                         families=families)
    g = torch.empty(B, T, D + 1, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_sum_bilinear", dtype == torch.float64)
    _launch(name, U.device, x1, x2, theta, fams, T, B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, T, t))
    return g


def kernel_sum_points_grad(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, families, U: torch.Tensor,
                           V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_sum_points_grad_f32: g_x1 [B, M, D], the derivative of sum_s u_s^T (sum_t K_t(x1, x2)) v_s with respect
    to x1, x2 held fixed, in one sweep.  The x2 side is kernel_sum_points_grad(x2, x1, theta, families, V, U)."""
    x1, x2, theta, fams, U, V, (B, M, N, D, T, t), dtype = _kernel_args("kernel_sum_points_grad", x1, x2, theta, V, U,
                                                                         families=families)
    g = torch.empty(B, M, D, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_sum_points_grad", dtype == torch.float64)
    _launch(name, U.device, x1, x2, theta, fams, T, B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, T, t))
    return g


def kernel_kron_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, family: int, task: torch.Tensor,
                                d: Optional[torch.Tensor] = None, const_diag: bool = False):
    """AddedDiag(Kron(Kernel(X, X, family), Bt), Diag(d)) (or the product alone), the multitask covariance with row index
    i T + t: y = (K (x) Bt) v + d o v, K formed on the fly and Bt applied while v is staged (csrc/lo_kernel_kron.hip).
    X [*batch, n, D], theta [B, D + 1] from kernel_theta, task = Bt [*batch, T, T].  None when D exceeds LO_KERNEL_MAX_DIM
    or T exceeds LO_KERNEL_KRON_MAX_TASKS (the caller composes the factors)."""
    _hip.require_hip(X, theta, task, d)
    n, D = X.shape[-2:]
    T = task.shape[-1]
    if D > _hip.LO_KERNEL_MAX_DIM or D < 1 or not 1 <= T <= _hip.LO_KERNEL_KRON_MAX_TASKS:
        return None
    X3, Bt = _flat(X.detach(), 2), _flat(task.detach(), 2)
    if theta.shape != (X3.shape[0], D + 1) or Bt.shape != (X3.shape[0], T, T):
        raise RuntimeError(f"kernel_kron_diag_descriptor: theta {tuple(theta.shape)}, task {tuple(task.shape)} for X "
                           f"{tuple(X.shape)}")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_KRON_DIAG, X3.shape[0], n * T, A0=X3, A1=theta, R=D,
                                         n2=int(family), batch_shape=X.shape[:-2], kernel_terms=T, task=Bt), d, const_diag)


def kernel_kron_mv(x: torch.Tensor, theta: torch.Tensor, task: torch.Tensor, family: int, v: torch.Tensor,
                   d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_kron_mv_f32: y [B, n T, c] = (K(x, x) (x) Bt) v (+ d o v), x [B, n, D], theta [B, D + 1], task = Bt
    [B, T, T] (used as given, symmetric or not), v [B, n T, c], row index i T + t.  A shape the kernel does not take
    raises."""
    x, _, theta, task, _, v, (B, n, _, D, T, c), dtype = _kernel_args("kernel_kron_mv", x, x, theta, v, d=d, task=task,
                                                                       block=task.shape[-1])
    d, mode = _kernel_diag(d, B, n * T, const_diag)
    y = torch.empty(B, n * T, c, dtype=dtype, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_kron_mv", dtype == torch.float64)
    _launch(name, v.device, x, theta, task, int(family), B, n, D, T, v, c, d, mode, y, ws_bytes=sizer(B, n, D, T, c))
    return y


def kernel_lmc_terms(desc: OperatorDescriptor) -> int:
    """Q of an LO_OP_KERNEL_LMC_DIAG descriptor: bits 16 .. 19 of its n2 (the family codes sit below)."""
    return (desc.n2 >> 16) & 15


def kernel_lmc_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, families, Bt: torch.Tensor,
                               d: Optional[torch.Tensor] = None, const_diag: bool = False):
    """AddedDiag(Kron(Kernel_0(X, X), B_0) + .. + Kron(Kernel_{Q-1}(X, X), B_{Q-1}), Diag(d)) (or the sum alone), the linear
    model of coregionalisation over ONE point tensor with row index i T + t: y = (sum_q K_q (x) B_q) v + d o v, every K_q
    formed on the fly in one pass (csrc/lo_kernel_lmc.hip).  X [*batch, n, D], theta [B, Q, D + 1] from kernel_sum_theta,
    `families` the Q codes, Bt [*batch, Q, T, T].  None when D exceeds LO_KERNEL_MAX_DIM, Q LO_KERNEL_MAX_TERMS or T
    LO_KERNEL_KRON_MAX_TASKS (the caller composes the terms)."""
    _hip.require_hip(X, theta, Bt, d)
    n, D = X.shape[-2:]
    families = [int(f) for f in families]
    Q, T = len(families), Bt.shape[-1]
    if (D > _hip.LO_KERNEL_MAX_DIM or D < 1 or not 1 <= Q <= _hip.LO_KERNEL_MAX_TERMS
            or not 1 <= T <= _hip.LO_KERNEL_KRON_MAX_TASKS):
        return None
    packed = kernel_sum_pack_families(families) | (Q << 16)
    X3, B4 = _flat(X.detach(), 2), _flat(Bt.detach(), 3)
    if theta.shape != (X3.shape[0], Q, D + 1) or B4.shape != (X3.shape[0], Q, T, T):
        raise RuntimeError(f"kernel_lmc_diag_descriptor: theta {tuple(theta.shape)}, task {tuple(Bt.shape)} for X "
                           f"{tuple(X.shape)}, {Q} terms")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_LMC_DIAG, X3.shape[0], n * T, A0=X3, A1=theta.contiguous(), R=D,
                                         n2=packed, batch_shape=X.shape[:-2], kernel_terms=T, task=B4), d, const_diag)


def kernel_lmc_mv(x: torch.Tensor, theta: torch.Tensor, task: torch.Tensor, families, v: torch.Tensor,
                  d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_lmc_mv_f32: y [B, n T, c] = (sum_q K_q(x, x) (x) B_q) v (+ d o v), x [B, n, D], theta [B, Q, D + 1],
    task = Bt [B, Q, T, T] (used as given, symmetric or not), `families` the Q codes, v [B, n T, c], row index i T + t.
    A shape the kernel does not take raises."""
    task = task.contiguous()
    T = task.shape[-1]
    x, _, theta, packed, _, v, (B, n, _, D, Q, c), dtype = _kernel_args("kernel_lmc_mv", x, x, theta, v, d=d, task=task,
                                                                         families=families, block=T)
    d, mode = _kernel_diag(d, B, n * T, const_diag)
    y = torch.empty(B, n * T, c, dtype=dtype, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_lmc_mv", False)
    _launch(name, v.device, x, theta, task, packed, B, n, D, Q, T, v, c, d, mode, y, ws_bytes=sizer(B, n, D, Q, T, c))
    return y


def kernel_grad_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, family: int, d: Optional[torch.Tensor] = None,
                                const_diag: bool = False):
    """AddedDiag(GradKernel(X, X), Diag(d)) (or the operator alone): the covariance of the values and the D partial
    derivatives at the n points, row index i (D + 1) + a, formed pair by pair (csrc/lo_kernel_grad.hip).  X [*batch, n, D],
    theta [B, D + 1] from kernel_theta, d over the n (D + 1) rows.  None when D exceeds LO_KERNEL_GRAD_MAX_DIM or the
    family is not RBF (the caller evaluates covar_func)."""
    _hip.require_hip(X, theta, d)
    n, D = X.shape[-2:]
    if D > _hip.LO_KERNEL_GRAD_MAX_DIM or D < 1 or int(family) != _hip.LO_KERNEL_RBF:
        return None
    X3 = _flat(X.detach(), 2)
    if theta.shape != (X3.shape[0], D + 1):
        raise RuntimeError(f"kernel_grad_diag_descriptor: theta of shape {tuple(theta.shape)} for X {tuple(X.shape)}")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_GRAD_DIAG, X3.shape[0], n * (D + 1), A0=X3, A1=theta, R=D,
                                         n2=int(family), batch_shape=X.shape[:-2]), d, const_diag)


def kernel_grad_mv(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, v: torch.Tensor,
                   d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_grad_mv_f32: y [B, M (D + 1), c] = K(x1, x2) v (+ d o v, only when M == N) for the gradient kernel's
    block matrix, x1 [B, M, D], x2 [B, N, D], theta [B, D + 1], v [B, N (D + 1), c].  A shape the kernel does not take
    raises."""
    x1, x2, theta, _, _, v, (B, M, N, D, _, c), dtype = _kernel_args("kernel_grad_mv", x1, x2, theta, v, d=d,
                                                                      block=x1.shape[-1] + 1)
    d, mode = _kernel_diag(d, B, M * (D + 1), const_diag)
    y = torch.empty(B, M * (D + 1), c, dtype=dtype, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_grad_mv", dtype == torch.float64)
    _launch(name, v.device, x1, x2, theta, int(family), B, M, N, D, v, c, d, mode, y, ws_bytes=sizer(B, M, N, D, c))
    return y


def kernel_grad_bilinear(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, family: int, U: torch.Tensor,
                         V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_grad_bilinear_f32: g_theta [B, D + 1], the derivative of sum_s u_s^T K(x1, x2) v_s with respect to theta
    (the inverse lengthscales, then outputscale^2) for the gradient kernel's block matrix.  x1 [B, M, D], x2 [B, N, D],
    U [B, M (D + 1), t], V [B, N (D + 1), t]."""
    x1, x2, theta, _, U, V, (B, M, N, D, _, t), dtype = _kernel_args("kernel_grad_bilinear", x1, x2, theta, V, U,
                                                                      block=x1.shape[-1] + 1)
    g = torch.empty(B, D + 1, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_grad_bilinear", dtype == torch.float64)
    _launch(name, U.device, x1, x2, theta, int(family), B, M, N, D, U, V, t, g, ws_bytes=sizer(B, M, N, D, t))
    return g


def kernel_task_diag_descriptor(X: torch.Tensor, theta: torch.Tensor, family: int, task: torch.Tensor,
                                d: Optional[torch.Tensor] = None, const_diag: bool = False):
    """AddedDiag(TaskKernel(X, X, family), Diag(d)) (or the operator alone), the task-indexed multitask covariance
    K_ij = os2 g(r_ij) Bt[t_i, t_j] formed on the fly (csrc/lo_kernel_task.hip).  X [*batch, N, D + 1]: D coordinates and
    then the task id of the observation; theta [B, D + 1] from kernel_theta over the D coordinates, task = Bt
    [*batch, T, T].  None when D + 1 exceeds LO_KERNEL_MAX_DIM or T exceeds LO_KERNEL_TASK_MAX_TASKS (the caller
    evaluates covar_func)."""
    _hip.require_hip(X, theta, task, d)
    N, D = X.shape[-2], X.shape[-1] - 1
    T = task.shape[-1]
    if D + 1 > _hip.LO_KERNEL_MAX_DIM or D < 1 or not 1 <= T <= _hip.LO_KERNEL_TASK_MAX_TASKS:
        return None
    X3, Bt = _flat(X.detach(), 2), _flat(task.detach(), 2)
    if theta.shape != (X3.shape[0], D + 1) or Bt.shape != (X3.shape[0], T, T):
        raise RuntimeError(f"kernel_task_diag_descriptor: theta {tuple(theta.shape)}, task {tuple(task.shape)} for X "
                           f"{tuple(X.shape)}")
    return _with_diag(OperatorDescriptor(_hip.LO_OP_KERNEL_TASK_DIAG, X3.shape[0], N, A0=X3, A1=theta.contiguous(), R=D,
                                         n2=int(family), batch_shape=X.shape[:-2], kernel_terms=T, task=Bt), d, const_diag)


def kernel_task_mv(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, task: torch.Tensor, family: int,
                   v: torch.Tensor, d: Optional[torch.Tensor] = None, const_diag: bool = False) -> torch.Tensor:
    """lo_kernel_task_mv_f32: y [B, M, c] = K(x1, x2) v (+ d o v when M == N and d is given), K_ij = os2 g(r_ij)
    Bt[t_i, t_j]; x1 [B, M, D + 1], x2 [B, N, D + 1] with the task id in the last column, theta [B, D + 1], task = Bt
    [B, T, T] (used as given, symmetric or not), v [B, N, c].  A shape the kernel does not take raises."""
    x1, x2, theta, task, _, v, (B, M, N, D, T, c), dtype = _kernel_args("kernel_task_mv", x1, x2, theta, v, d=d,
                                                                         task=task, ids=1)
    d, mode = _kernel_diag(d, B, N, const_diag)
    y = torch.empty(B, M, c, dtype=dtype, device=v.device)
    name, sizer = _kernel_entry("lo_kernel_task_mv", dtype == torch.float64)
    _launch(name, v.device, x1, x2, theta, task, int(family), B, M, N, D, T, v, c, d, mode, y,
            ws_bytes=sizer(B, M, N, D, T, c))
    return y


def kernel_task_bilinear(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, task: torch.Tensor, family: int,
                         U: torch.Tensor, V: torch.Tensor):
    """lo_kernel_task_bilinear_f32: (g_theta [B, D + 1], g_task [B, T, T]), the derivatives of sum_s u_s^T K(x1, x2) v_s
    with respect to theta (the inverse lengthscales, then outputscale^2) and to Bt (entry by entry, not symmetrised).
    U [B, M, t], V [B, N, t]."""
    x1, x2, theta, task, U, V, (B, M, N, D, T, t), dtype = _kernel_args("kernel_task_bilinear", x1, x2, theta, V, U,
                                                                         task=task, ids=1)
    g = torch.empty(B, D + 1, dtype=dtype, device=U.device)
    gB = torch.empty(B, T, T, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_task_bilinear", dtype == torch.float64)
    _launch(name, U.device, x1, x2, theta, task, int(family), B, M, N, D, T, U, V, t, g, gB,
            ws_bytes=sizer(B, M, N, D, T, t))
    return g, gB


def kernel_task_points_grad(x1: torch.Tensor, x2: torch.Tensor, theta: torch.Tensor, task: torch.Tensor, family: int,
                            U: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
    """lo_kernel_task_points_grad_f32: g_x1 [B, M, D + 1], the derivative of sum_s u_s^T K(x1, x2) v_s with respect to
    x1, x2 held fixed; the task column is 0.  The x2 side is kernel_task_points_grad(x2, x1, theta, task.mT, family, V, U)."""
    x1, x2, theta, task, U, V, (B, M, N, D, T, t), dtype = _kernel_args("kernel_task_points_grad", x1, x2, theta, V, U,
                                                                         task=task, ids=1)
    g = torch.empty(B, M, D + 1, dtype=dtype, device=U.device)
    name, sizer = _kernel_entry("lo_kernel_task_points_grad", dtype == torch.float64)
    _launch(name, U.device, x1, x2, theta, task, int(family), B, M, N, D, T, U, V, t, g,
            ws_bytes=sizer(B, M, N, D, T, t))
    return g


_MASK_BASE_KINDS = (_hip.LO_OP_LOWRANK_DIAG, _hip.LO_OP_DENSE_DIAG, _hip.LO_OP_KRON_DIAG, _hip.LO_OP_SUM)


def masked_descriptor(base_desc: OperatorDescriptor, idx: torch.Tensor, d: Optional[torch.Tensor] = None,
                      const_diag: bool = False):
    """AddedDiag(Masked(base, mask, mask), Diag(d)) (or the masked operator alone): y = S (base) S^T v + d o v with S
    selecting the rows `idx` (int64 [M] on the device, strictly increasing) of the base -- whose own diagonal, if any,
    sits inside the mask.  d [*batch, M] (or one value per member) is the diagonal outside it.  None for a base kind
    the C side does not take (the caller composes the product)."""
    if base_desc is None or base_desc.kind not in _MASK_BASE_KINDS or base_desc.dtype != torch.float32:
        return None  # (float64 bases: the masked kernels are fp32)
    if any(t.kind in (_hip.LO_OP_KERNEL_DIAG, _hip.LO_OP_KERNEL_SUM_DIAG, _hip.LO_OP_KERNEL_PARAM_DIAG,
                      _hip.LO_OP_KERNEL_SM_DIAG)
           for t in base_desc.terms):
        return None  # (a sum's matrix-free kernel terms are not taken under a mask)
    if idx.dtype != torch.int64 or not idx.is_cuda or idx.dim() != 1 or idx.numel() < 1:
        return None
    _hip.require_hip(d)
    return _with_diag(OperatorDescriptor(_hip.LO_OP_MASKED, base_desc.B, idx.numel(), batch_shape=base_desc.batch_shape,
                                         mask=(base_desc, idx.contiguous())), d, const_diag)


def mask_expand(idx: torch.Tensor, n0: int, v: torch.Tensor) -> torch.Tensor:
    """u = S^T v: v [*batch, M, c] -> [*batch, n0, c] with the rows idx (int64 [M], strictly increasing) filled and zeros
    elsewhere (lo_mask_expand_f32: one coalesced write of u, no clearing pass)."""
    lib = _hip.load()
    _hip.require_hip(v)
    M, c = v.shape[-2:]
    if idx.numel() != M or idx.dtype != torch.int64 or not idx.is_cuda:
        raise RuntimeError(f"mask_expand: {idx.numel()} indices for vectors of shape {tuple(v.shape)}")
    v3 = _flat(v, 2)
    u = torch.empty(v3.shape[0], n0, c, dtype=torch.float32, device=v.device)
    _launch("lo_mask_expand_f32", v.device, idx.contiguous(), M, n0, v3, u, v3.shape[0], c,
            ws_bytes=lib.lo_mask_expand_workspace_bytes(n0))
    return u.reshape(*v.shape[:-2], n0, c)


def bilinear_hadamard(F: torch.Tensor, G: torch.Tensor, left_vecs: torch.Tensor, right_vecs: torch.Tensor):
    """lo_hadamard_bilinear_f32: (dF, dG) of sum_s u_s^T (F F^T o G G^T) v_s, F [*b, N, p], G [*b, N, q]
    (mul_linear_operator.py:91-126 summed over both roots).  Returned at the broadcast batch of the operands."""
    lib = _hip.load()
    bs0 = torch.broadcast_shapes(F.shape[:-2], G.shape[:-2])
    U, V, bs = _uv(left_vecs, right_vecs, bs0)
    B, N, S = U.shape
    p, q = F.shape[-1], G.shape[-1]
    F3 = F.expand(*bs, N, p).contiguous().reshape(B, N, p)
    G3 = G.expand(*bs, N, q).contiguous().reshape(B, N, q)
    _hip.require_hip(F3, G3)
    dev = U.device
    dF = torch.empty(B, N, p, dtype=torch.float32, device=dev)
    dG = torch.empty(B, N, q, dtype=torch.float32, device=dev)
    ws_bytes = lib.lo_hadamard_bilinear_workspace_bytes(B, N, p, q, S)
    if ws_bytes == 0:
        raise _hip.HipExtensionError(f"lo_hadamard_bilinear_f32 does not take B={B} N={N} p={p} q={q} S={S}")
    _launch("lo_hadamard_bilinear_f32", dev, F3, G3, U, V, B, N, p, q, S, dF, dG, ws_bytes=ws_bytes)
    return dF.reshape(*bs, N, p), dG.reshape(*bs, N, q)


def interp_plan_build(idx: torch.Tensor, M: int) -> torch.Tensor:
    """The grid-major copy of W (idx int64 [B, N, J], grid of M points) as a device byte tensor (lo_interp_plan_build)."""
    lib = _hip.load()
    idx = idx.contiguous()
    B, N, J = idx.shape
    plan = _hip.workspace(lib.lo_interp_plan_bytes(B, N, J, M), idx.device)
    _launch("lo_interp_plan_build", idx.device, idx, B, N, J, M, plan, plan.numel())
    return plan


# Memo of the grid-major copies, keyed on the index tensor the operator holds (address, version counter, layout) and
# the batch / grid the copy was built for; the entry keeps the tensor alive, so its address cannot be reused by other
# data, and an in-place update bumps the version counter (writes through `.data` do not: clear_interp_plan_memo()).
INTERP_PLAN_MEMO_SIZE = 4
_interp_plan_memo: "list[tuple]" = []


def interp_plan(idx: torch.Tensor, batch_shape, M: int) -> Optional[torch.Tensor]:
    """interp_plan_build of `idx` [*b, N, J] expanded to batch_shape, memoised across calls; None for inference
    tensors (no version counter: the caller lets every plan build its own copy)."""
    if idx.is_inference():
        return None
    key = (idx.data_ptr(), idx._version, tuple(idx.shape), tuple(idx.stride()), tuple(batch_shape), int(M))
    for entry in _interp_plan_memo:
        if entry[0] == key:
            return entry[2]
    N, J = idx.shape[-2:]
    plan = interp_plan_build(idx.expand(*batch_shape, N, J).reshape(-1, N, J), M)
    _interp_plan_memo.insert(0, (key, idx, plan))
    del _interp_plan_memo[INTERP_PLAN_MEMO_SIZE:]
    return plan


def clear_interp_plan_memo():
    _interp_plan_memo.clear()


def interp_t_planned(plan: torch.Tensor, vals: torch.Tensor, v: torch.Tensor, M: int) -> torch.Tensor:
    """W^T v from a kept grid-major copy (interp_plan): vals [B, N, J], v [B, N, c] -> [B, M, c]."""
    _hip.require_hip(vals, v)
    B, N, J = vals.shape
    c = v.shape[-1]
    vals, v = vals.contiguous(), v.contiguous()
    out = torch.empty(B, M, c, dtype=torch.float32, device=v.device)
    _launch("lo_interp_t_planned_f32", v.device, plan, vals, B, N, J, M, v, c, out)
    return out


def interp(idx: torch.Tensor, vals: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """W u: idx int64 / vals fp32 [B, N, J], u [B, M, c] -> [B, N, c] (lo_interp_f32)."""
    _hip.require_hip(vals, u)
    B, N, J = idx.shape
    M, c = u.shape[-2:]
    idx, vals, u = idx.contiguous(), vals.contiguous(), u.contiguous()
    y = torch.empty(B, N, c, dtype=torch.float32, device=u.device)
    _launch("lo_interp_f32", u.device, idx, vals, B, N, J, M, u, c, y)
    return y


def interp_sum(idx: torch.Tensor, vals: torch.Tensor, u: torch.Tensor, d: Optional[torch.Tensor] = None,
               v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sum_p W_p u_p (+ d o v): idx int64 / vals fp32 [B, P, N, J], u [B, P, M, c] -> [B, N, c], with d [B, N] or [B]
    and v [B, N, c] (lo_interp_sum_f32; terms summed in ascending order, no [P, N, c] intermediate)."""
    _hip.require_hip(vals, u, d, v)
    B, P, N, J = idx.shape
    M, c = u.shape[-2:]
    idx, vals, u = idx.contiguous(), vals.contiguous(), u.contiguous()
    mode = _hip.LO_DIAG_NONE if d is None else (_hip.LO_DIAG_FULL if d.dim() == 2 else _hip.LO_DIAG_CONST)
    if d is not None:
        d, v = d.contiguous(), v.contiguous()
    y = torch.empty(B, N, c, dtype=torch.float32, device=u.device)
    _launch("lo_interp_sum_f32", u.device, idx, vals, B, P, N, J, M, u, c, d, mode, v, y)
    return y


def interp_t_bcast(plan: torch.Tensor, vals: torch.Tensor, v: torch.Tensor, M: int) -> torch.Tensor:
    """W_p^T v for every term p from one v: plan = interp_plan_build over the B P members, vals [B, P, N, J],
    v [B, N, c] -> [B, P, M, c] (lo_interp_t_bcast_planned_f32; v is not copied P times)."""
    _hip.require_hip(vals, v)
    B, P, N, J = vals.shape
    c = v.shape[-1]
    vals, v = vals.contiguous(), v.contiguous()
    out = torch.empty(B, P, M, c, dtype=torch.float32, device=v.device)
    _launch("lo_interp_t_bcast_planned_f32", v.device, plan, vals, B, P, N, J, M, v, c, out)
    return out


def interp_t(idx: torch.Tensor, vals: torch.Tensor, v: torch.Tensor, M: int) -> torch.Tensor:
    """W^T v: idx / vals [B, N, J], v [B, N, c] -> [B, M, c] (lo_interp_t_f32, deterministic)."""
    lib = _hip.load()
    _hip.require_hip(vals, v)
    B, N, J = idx.shape
    c = v.shape[-1]
    idx, vals, v = idx.contiguous(), vals.contiguous(), v.contiguous()
    out = torch.empty(B, M, c, dtype=torch.float32, device=v.device)
    _launch("lo_interp_t_f32", v.device, idx, vals, B, N, J, M, v, c, out,
            ws_bytes=lib.lo_interp_t_workspace_bytes(B, N, J, M))
    return out


def toeplitz_mv(column: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """T u for the symmetric Toeplitz matrix of column [B, M]; u [B, M, c] (lo_toeplitz_mv_f32)."""
    lib = _hip.load()
    _hip.require_hip(column, u)
    B, M = column.shape
    c = u.shape[-1]
    column, u = column.contiguous(), u.contiguous()
    y = torch.empty(B, M, c, dtype=torch.float32, device=u.device)
    _launch("lo_toeplitz_mv_f32", u.device, column, B, M, u, c, y, ws_bytes=lib.lo_toeplitz_workspace_bytes(B, M, c))
    return y


def toeplitz_bilinear(u: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """g [B, M]: g_k = sum_s u_s^T (dT/dt_k) v_s for u, v [B, M, S] (lo_toeplitz_bilinear_f32)."""
    lib = _hip.load()
    _hip.require_hip(u, v)
    B, M, S = u.shape
    u, v = u.contiguous(), v.contiguous()
    g = torch.empty(B, M, dtype=torch.float32, device=u.device)
    _launch("lo_toeplitz_bilinear_f32", u.device, u, v, B, M, S, g, ws_bytes=lib.lo_toeplitz_workspace_bytes(B, M, 1))
    return g


def interp_values_grad(idx: torch.Tensor, lv: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    """g [B, N, J]: g[n, j] = sum_s lv[n, s] R[idx[n, j], s]; idx [B, N, J], lv [B, N, S], R [B, M, S]."""
    _hip.require_hip(lv, R)
    B, N, J = idx.shape
    M, S = R.shape[-2:]
    idx, lv, R = idx.contiguous(), lv.contiguous(), R.contiguous()
    g = torch.empty(B, N, J, dtype=torch.float32, device=R.device)
    _launch("lo_interp_values_grad_f32", R.device, idx, B, N, J, M, lv, R, S, g)
    return g


def _with_diag(desc: OperatorDescriptor, d, const_diag):
    if d is not None:
        if d.dtype != desc.dtype:
            raise _hip.HipExtensionError(f"a {d.dtype} diagonal cannot be attached to a {desc.dtype} operator descriptor")
        desc.d, desc.diag_mode, _ = _diag_operand(d, desc.B, desc.N, const_diag)
    return desc


# ------------------------------------------------------------------------------------------------
def matvec(desc: OperatorDescriptor, v: torch.Tensor) -> torch.Tensor:
    """y = A v for v [*batch, N, c] (LinearOperator._matmul of the lowered operator)."""
    lib = _hip.load()
    _hip.require_hip(v, dtype=desc.dtype)
    c = v.shape[-1]
    v3 = _flat(v, 2)
    if v3.shape[0] != desc.B or v3.shape[1] != desc.N:
        raise RuntimeError(f"matvec: rhs of shape {tuple(v.shape)} does not match operator batch {desc.B} x N {desc.N}")
    y = torch.empty_like(v3)
    s = desc.c_struct(desc.dtype)
    f64 = desc.dtype == torch.float64
    ws_bytes = (lib.lo_matvec_f64_workspace_bytes if f64 else lib.lo_matvec_workspace_bytes)(C.byref(s), c)
    ws = _hip.workspace(ws_bytes, v.device)
    name = "lo_matvec_f64" if f64 else "lo_matvec_f32"
    _hip.check(getattr(lib, name)(C.byref(s), _hip.ptr(v3), _hip.ptr(y), c, _hip.ptr(ws), ws.numel(),
                                  _hip.stream_ptr(v.device)), name)
    return y.reshape(v.shape)


# Which float64 products the operators' `_matmul` hands to lo_matvec_f64, by (kind, one column / more columns): True only
# where tools/mb_f64.py measured the native product at least as fast as the ATen composition `_matmul` otherwise runs
# (DESIGN.md section 6g).  A combination that is absent keeps the composition; the descriptor still serves the float64
# CG, MINRES and Lanczos, where it replaces a Python call per product.  Measured (native / ATen, microseconds):
#   low-rank 64 x 8192 x 32        1 column  76 / 161     17 columns   392 / 428
#   Kronecker 16 x (128 (x) 128)   1 column  31 /  60     17 columns   172 / 117   (stays with ATen)
#   sum low-rank + dense, N 4096   1 column 155 / 212     17 columns  3489 / 402   (stays with ATen)
# A dense operator alone was not timed and keeps torch.matmul.
# The matrix-free kernel kind (csrc/lo_kernel_op_f64.hip) is in the table unconditionally: its purpose is memory (the
# composition stores the [B, N, N] matrix), not a timing (DESIGN.md sections 6l, 6p).
_NATIVE_MATMUL_F64: dict = {("lowrank", 1): True, ("lowrank", 2): True, ("kron", 1): True, ("sum", 1): True,
                            ("kernel", 1): True, ("kernel", 2): True}
_F64_KIND_NAMES = {_hip.LO_OP_LOWRANK_DIAG: "lowrank", _hip.LO_OP_DENSE_DIAG: "dense", _hip.LO_OP_KRON_DIAG: "kron",
                   _hip.LO_OP_SUM: "sum", _hip.LO_OP_KERNEL_DIAG: "kernel"}


def _f64_route_kind(op) -> Optional[str]:
    """The routing-table kind of an operator from its classes alone (nothing is lowered, no tensor is touched): the
    kind its descriptor would have, or None for an operator the float64 kernels do not take."""
    from . import operators as ops

    if isinstance(op, ops.ConstantMulLinearOperator):
        return _f64_route_kind(op.base_linear_op)
    if isinstance(op, ops.SumLinearOperator):  # (AddedDiag included: a sum of its operator and its diagonal)
        flat, stack = [], list(op.linear_ops)
        while stack:
            t = stack.pop()
            if isinstance(t, ops.SumLinearOperator):
                stack.extend(t.linear_ops)
            elif not isinstance(t, ops.DiagLinearOperator):
                flat.append(t)
        if len(flat) == 1:
            return _f64_route_kind(flat[0])
        return "sum" if flat else None
    if isinstance(op, ops.RootLinearOperator):
        return "lowrank"
    if isinstance(op, ops.KroneckerProductLinearOperator):
        return "kron"
    if isinstance(op, ops.DenseLinearOperator):
        return "dense"
    if isinstance(op, ops.KernelLinearOperator) and op._native_f64_refusal(check_device=False) is None:
        return "kernel"
    return None


def native_matmul_candidate(op, rhs: torch.Tensor) -> bool:
    """Whether an operator's `_matmul` should lower itself for this right-hand side at all: fp32 device blocks always;
    float64 ones only when the routing table sends the product of THIS operator's kind and column class to
    lo_matvec_f64 -- decided before anything is lowered, so a product that stays with ATen pays nothing for the table."""
    if rhs.dim() < 2 or not rhs.is_cuda:
        return False
    if rhs.dtype == torch.float32:
        return True
    if rhs.dtype != torch.float64 or op.dtype != torch.float64:
        return False
    return bool(_NATIVE_MATMUL_F64.get((_f64_route_kind(op), 1 if rhs.shape[-1] == 1 else 2), False))


# Which products of the additive SKI kind (LO_OP_SKI_SUM_DIAG) the operators' `_matmul` hands to lo_matvec_f32, by column
# class (one column / more columns): True only where tools/mb_ski_sum.py measured the kind faster than the composition
# beyond the run-to-run spread.  The descriptor lowers always: CG, Lanczos, MINRES and the pivoted
# Cholesky run on it whatever this table says.  Measured (kind / composition, microseconds, median of 5 rounds):
#   S1: 1 x 262144, P 8, M 8192, J 4    1 column  177 / 196     17 columns  1317 / 1461
#   S2: 16 x 16384, P 4, M 2048, J 4    1 column   96 / 107     17 columns   661 /  721
NATIVE_MATMUL_SKI_SUM: dict = {1: True, 2: True}


# Which products of the LMC kind (LO_OP_KERNEL_LMC_DIAG) the operators' `_matmul` hands to lo_matvec_f32, by (Q, T, one
# column / more columns): True only where tools/mb_kernel_lmc.py measured the fused product faster than the per-term
# composition (Q calls of lo_kernel_kron_mv_f32 and the adds) beyond the run-to-run spread at BOTH measured shapes.  An
# absent cell keeps the composition; the descriptor lowers always: CG, Lanczos, MINRES and the pivoted Cholesky run on it
# whatever this table says.  Measured on the MI355X (fused / composition, microseconds, median of 5 rounds, the ranges
# within 1 % of the medians but for a few rounds; 1 x 16384, D 4 and 8 x 4096, D 16):
#   Q 2  T 2   1 column  394 / 314,  454 / 427     17 columns  1920 / 1607,  1768 / 1396
#   Q 2  T 4   1 column  401 / 320,  457 / 431     17 columns  3552 / 2826,  3128 / 2309
#   Q 4  T 2   1 column  787 / 643,  895 / 869     17 columns  4669 / 3218,  4874 / 2823
#   Q 4  T 4   1 column  800 / 659,  902 / 878     17 columns  9026 / 5620,  9114 / 4663
# The fused product wins in no cell -- the single-term sweep carries up to 32 wide columns without a term loop, and the
# pairs' work is the same either way -- so the table is empty.  What the kind buys is the solvers: one preconditioned solve
# at 1 x 8192 (T 4, Q 2) takes 93 ms on the kind against 197 ms through the closure.
_NATIVE_MATMUL_KERNEL_LMC: dict = {}


def native_matmul(desc: Optional[OperatorDescriptor], rhs: torch.Tensor) -> bool:
    """Whether `_matmul` hands the product of the lowered operator `desc` with `rhs` to `matvec`."""
    if desc is None or desc.dtype != rhs.dtype:
        return False
    if desc.kind == _hip.LO_OP_SKI_SUM_DIAG:
        return bool(NATIVE_MATMUL_SKI_SUM.get(1 if rhs.shape[-1] == 1 else 2, False))
    if desc.kind == _hip.LO_OP_KERNEL_LMC_DIAG:
        return bool(_NATIVE_MATMUL_KERNEL_LMC.get((kernel_lmc_terms(desc), desc.kernel_terms,
                                                   1 if rhs.shape[-1] == 1 else 2), False))
    if desc.dtype == torch.float32:
        return True
    return bool(_NATIVE_MATMUL_F64.get((_F64_KIND_NAMES.get(desc.kind), 1 if rhs.shape[-1] == 1 else 2), False))


def block_matvec(desc: OperatorDescriptor, layout: int, T: int, v: torch.Tensor) -> Optional[torch.Tensor]:
    """y = Block(A) v for the block operator over the B = G T members of `desc`, the block index fastest
    (lo_block_mv_f32): `layout` LO_BLOCK_DIAG / LO_BLOCK_INTERLEAVED with v [*batch, T N, c] in that row order, or
    LO_BLOCK_SUM with v [*batch, N, c].  None for a descriptor the kernels leave to the caller's composition
    (LO_ERR_UNSUPPORTED)."""
    lib = _hip.load()
    if desc.dtype != torch.float32:
        return None  # (the block kernels are fp32)
    _hip.require_hip(v)
    c = v.shape[-1]
    v3 = _flat(v, 2)
    rows = desc.N if layout == _hip.LO_BLOCK_SUM else T * desc.N
    if T < 1 or desc.B % T or v3.shape[0] != desc.B // T or v3.shape[1] != rows:
        raise RuntimeError(f"block_matvec: rhs of shape {tuple(v.shape)} does not match {desc.B} members of size "
                           f"{desc.N} in groups of {T} blocks (layout {layout})")
    y = torch.empty_like(v3)
    s = desc.c_struct()
    ws = _hip.workspace(lib.lo_block_mv_workspace_bytes(C.byref(s), layout, T, c), v.device)
    rc = lib.lo_block_mv_f32(C.byref(s), layout, T, _hip.ptr(v3), _hip.ptr(y), c, _hip.ptr(ws), ws.numel(),
                             _hip.stream_ptr(v.device))
    if rc == _hip.LO_ERR_UNSUPPORTED:
        return None
    _hip.check(rc, "lo_block_mv_f32")
    return y.reshape(v.shape)


_CACHE_GENERATIONS = itertools.count(1)


@dataclass
class WoodburyPreconditioner:
    """Device form of the reference's cached (Q, noise) pair, added_diag_linear_operator.py:63-70."""

    Q: Optional[torch.Tensor]  # [B, N, ldq]; None for a root-form-only preconditioner (built on demand: ensure_q)
    dinv: torch.Tensor  # [B, N] or [B]
    k: int
    constant_diag: bool
    logdet: Optional[torch.Tensor] = None  # [B]
    # root form (lo_precond_desc.F / EF / E): P^-1 r = (r - C F C^T (r o dinv)) o dinv for a low-rank operator whose
    # pivoted-Cholesky factor this preconditioner was built from; [B, rf_ld, rf_ld] each
    F: Optional[torch.Tensor] = None
    EF: Optional[torch.Tensor] = None
    E: Optional[torch.Tensor] = None
    # R-space form (lo_precond_desc.RS): fp64 [B, 6, rf_ld, rf_ld] = E | F E | E F E | C^T C | F | E F -- single-column result-only solves
    # run their iterations on R + 1 coordinates (csrc/lo_rspace.hip)
    RS: Optional[torch.Tensor] = None
    # diagonal form of the R-space iteration (lo_precond_desc.RSD, csrc/lo_eigform.hip): fp64 [B, 6, rf_ld, rf_ld], built by
    # ensure_eigform() once the cache has served enough single-column solves to pay for it (_eigform_due)
    RSD: Optional[torch.Tensor] = None
    rsd_refused: Optional[str] = None  # why lo_precond_eigform_f32's form is not used for this cache (None: not built yet / in use)
    rs_rank: int = 0      # true rank of the root the RS form was built from
    rs_uses: int = 0      # single-column result-only solves this cache has served
    source: Optional[tuple] = None  # (L, d) the preconditioner was built from (to build Q later)
    # Kronecker root form (lo_precond_desc.kron_*): (kron_a [B, n1, 16], kron_b [B, n2, 16], kron_F [B, 16, 16]) of a
    # Kronecker operator with a constant diagonal -- the single-column CG of large N forms the rows of the tall matrix
    # on the fly instead of streaming Q
    kron: Optional[tuple] = None
    kron_kappa: Optional[float] = None  # worst rounding amplification of the Kronecker root form over the batch
    rebuild: Optional[Callable] = None  # root form from the fused solve (no L exists): () -> the full preconditioner
    # lo_precond_desc.generation: one number per cache OBJECT (never 0), part of the key of the library's "this solve missed
    # the stop rule in its result-only pass" memo -- a tensor address the allocator hands out again does not inherit it
    generation: int = field(default_factory=lambda: next(_CACHE_GENERATIONS))
    # native solve sessions (lo_cg_session) of the single-column solves this cache serves, by operator and parameters
    # (_session_solve): a small LRU, dropped by whatever changes the cache and destroyed with it
    _sessions: OrderedDict = field(default_factory=OrderedDict, repr=False, compare=False)
    # the session of the last solve with what it was found by, in front of the LRU (_session_solve); gone with the sessions
    _memo: Optional[tuple] = field(default=None, repr=False, compare=False)

    @property
    def rf_ld(self) -> int:
        return 0 if self.F is None else int(self.F.shape[-1])

    def drop_sessions(self) -> None:
        """Destroy the native solve sessions of this cache (their structs hold pointers into its tensors)."""
        self.__dict__["_memo"] = None
        sessions = self.__dict__.get("_sessions")
        while sessions:
            _, ent = sessions.popitem()
            ent.close()

    def __del__(self):
        try:
            self.drop_sessions()
        except Exception:  # noqa: BLE001 -- interpreter shutdown: the library may be gone already
            pass

    def ensure_q(self) -> "WoodburyPreconditioner":
        """Build the generic (Q, dinv) form if this preconditioner only carries the root form."""
        if self.Q is None:
            if self.source is not None:
                L, d = self.source
                full = precond_build(L, d, self.constant_diag)
            elif self.rebuild is not None:
                full = self.rebuild().ensure_q()
            else:
                raise _hip.HipExtensionError("root-form-only preconditioner without its factor: Q cannot be built")
            self.drop_sessions()
            self.Q, self.dinv, self.k = full.Q, full.dinv, full.k
        return self

    def ensure_eigform(self) -> "WoodburyPreconditioner":
        """Build the diagonal form (lo_precond_eigform_f32) next to the R-space form.  The cache keeps the dense form when a
        member refuses it (`rsd_refused`: an eigenvalue of the preconditioned member not positive, or a change of basis that
        would cost accuracy -- DESIGN 4.14); one attempt per cache."""
        if self.RSD is None and self.rsd_refused is None and self.RS is not None:
            if self.rs_rank < 2 or self.rs_rank % 2:
                self.rsd_refused = "root rank"
                return self
            B, ld = self.RS.shape[0], self.RS.shape[-1]
            RSD = torch.empty_like(self.RS)
            _launch("lo_precond_eigform_f32", self.RS.device, self.RS, B, self.rs_rank, ld, RSD)
            worst = float(RSD[:, 5, 1, 0].amin().item())
            if worst > 0:
                self.drop_sessions()
                self.RSD = RSD
            else:
                self.rsd_refused = "ill-conditioned basis" if worst == -2.0 else "eigenvalue not positive"
        return self

    def c_struct(self) -> _hip.PrecondDesc:
        s = _hip.PrecondDesc()
        s.k, s.constant_diag, s.reserved = self.k, int(self.constant_diag), 0
        s.generation = (self.generation & 0x7FFFFFFF) or 1
        s.ldq = padded_rank(self.k) if self.Q is None else self.Q.shape[-1]
        s.Q = None if self.Q is None else self.Q.data_ptr()
        s.dinv = self.dinv.data_ptr()
        if self.F is not None:
            s.F, s.EF, s.rf_ld = self.F.data_ptr(), self.EF.data_ptr(), self.rf_ld
            s.E = None if self.E is None else self.E.data_ptr()
            s.RS = None if self.RS is None else self.RS.data_ptr()
            s.RSD = self.RSD.data_ptr() if (self.RS is not None and self.RSD is not None) else None
        if self.kron is not None:
            s.kron_a, s.kron_b, s.kron_F = (t.data_ptr() for t in self.kron)
        return s


@dataclass
class CGResult:
    x: torch.Tensor
    t_mat: Optional[torch.Tensor]
    iterations: int
    matvecs: int
    tolerance_reached: bool
    nan_detected: bool
    skipped: bool
    mean_residual: float


@dataclass
class MinresResult:
    x: torch.Tensor  # [n_shifts, *batch, N, c]
    iterations: int
    matvecs: int
    converged: bool
    conv: float


def _minres_operands(rhs, shifts, value, max_iter, tolerance, eps, prm_cls):
    """What the two MINRES entry points share: (rhs [B, N, c], shifts [Q] | [Q, B], the parameter struct, x [Q, B, N, c])."""
    rhs3 = _flat(rhs, 2)
    B = rhs3.shape[0]
    Q = shifts.shape[0]
    per_member = shifts.dim() > 1
    sh = shifts.to(device=rhs.device, dtype=rhs.dtype)
    sh = (sh.expand(Q, *rhs.shape[:-2]).reshape(Q, B) if per_member else sh.reshape(Q)).contiguous()
    prm = prm_cls()
    prm.c, prm.n_shifts, prm.max_iter = rhs.shape[-1], Q, max_iter
    prm.has_value, prm.value = (0, 1.0) if value is None else (1, float(value))
    prm.shifts_per_member, prm.tolerance, prm.eps = int(per_member), tolerance, eps
    return rhs3, sh, prm, torch.empty(Q, *rhs3.shape, dtype=rhs.dtype, device=rhs.device)


def _minres_result(x, rhs, info) -> MinresResult:
    return MinresResult(x.reshape(x.shape[0], *rhs.shape), info.iterations, info.matvecs, bool(info.converged),
                        float(info.conv))


def minres_solve(desc: Optional[OperatorDescriptor], rhs: torch.Tensor, shifts: torch.Tensor, *,
                 value: Optional[float] = None, precond: Optional[WoodburyPreconditioner] = None,
                 matvec_closure: Optional[Callable] = None, precond_closure: Optional[Callable] = None,
                 closure_batch_shape=None, max_iter: int = 1000, tolerance: float = 1e-4,
                 eps: float = 1e-25) -> MinresResult:
    """lo_minres_f32: the reference's shifted MINRES (utils/minres.py:10-207) on the device.
    rhs [*batch, N, c]; shifts [Q] or [Q, *batch]; returns x [Q, *batch, N, c] (scaled back by the rhs norms)."""
    lib = _hip.load()
    _hip.require_hip(rhs, shifts)
    N = rhs.shape[-2]
    dev = rhs.device
    rhs3, sh, prm, x = _minres_operands(rhs, shifts, value, max_iter, tolerance, eps, _hip.MinresParams)
    B = rhs3.shape[0]
    if desc is not None and (desc.B != B or desc.N != N):
        raise RuntimeError(f"minres: rhs {tuple(rhs.shape)} does not match operator batch {desc.B}, N {desc.N}")
    bshape = tuple(closure_batch_shape) if closure_batch_shape is not None else tuple(rhs.shape[:-2])
    s, mv_cb, mv_err = _f32_operator(desc, matvec_closure, bshape, B, N, dev)
    pc_cb, pc_err = _wrap_closure(precond_closure, dev, bshape) if precond_closure is not None else _NO_CLOSURE
    pre_s = precond.ensure_q().c_struct() if precond is not None else None  # (MINRES applies the Q form)
    info = _hip.MinresInfo()
    _launch("lo_minres_f32", dev, C.byref(s), mv_cb, None, _byref(pre_s), pc_cb, None, C.byref(prm), rhs3, sh, x,
            ws_bytes=lib.lo_minres_workspace_bytes(C.byref(s), _byref(pre_s), C.byref(prm)), info=info,
            errors=(mv_err, pc_err))
    return _minres_result(x, rhs, info)


def minres_solve_f64(A: Optional[torch.Tensor], rhs: torch.Tensor, shifts: torch.Tensor, *,
                     value: Optional[float] = None, matvec_closure: Optional[Callable] = None,
                     precond_closure: Optional[Callable] = None, max_iter: int = 1000, tolerance: float = 1e-4,
                     eps: float = 1e-25, desc: Optional[OperatorDescriptor] = None,
                     precond: Optional[tuple] = None) -> MinresResult:
    """lo_minres_f64: the reference's shifted MINRES (utils/minres.py:10-207) with float64 operands -- what the
    reference's test/utils/test_minres.py runs.  `A` [*batch, N, N] is multiplied by the library's fp64 kernel, a
    float64 descriptor `desc` by lo_matvec_f64 inside the library, any other operator is called back once per product;
    `precond`: the cached pair (Q, noise, constant_diag) of the float64 Woodbury preconditioner, applied inside the
    library (in place of `precond_closure`: any callable or None)."""
    lib = _hip.load()
    _hip.require_hip(rhs, A, dtype=torch.float64)
    N = rhs.shape[-2]
    dev = rhs.device
    bshape = tuple(rhs.shape[:-2])
    rhs3, sh, prm, x = _minres_operands(rhs, shifts, value, max_iter, tolerance, eps, _hip.MinresParamsF64)
    B = rhs3.shape[0]
    A3, d2, mv_cb, mv_user, pc_cb, pc_user, errors, keep = _f64_operands(
        lib, A, None, desc, matvec_closure, precond, precond_closure, bshape, B, N, rhs.shape[-1], dev)
    info = _hip.MinresInfoF64()
    _launch("lo_minres_f64", dev, A3, d2, mv_cb, mv_user, pc_cb, pc_user, C.byref(prm), B, N, rhs3, sh, x,
            ws_bytes=lib.lo_minres_f64_workspace_bytes(B, N, C.byref(prm)), info=info, errors=errors)
    del keep  # (the solver is synchronous: the contexts and workspaces of the callbacks were needed until here)
    return _minres_result(x, rhs, info)


# The diagonal form of the R-space iteration (csrc/lo_eigform.hip) is a cache-lifetime investment: two R x R Jacobi
# eigendecompositions per member (measured 0.45 ms + 0.45 us per member on the MI355X) against ~3.5 us per solve and
# round of 64 resident members (k_cg_rspace 200 -> 171 us at 512 members).  A cache gets the form when the solves it
# has served would have paid for it (the ski-rental rule: never more than twice the optimal cost):
#   512 members: on the 25th single-column solve, 4096 members: on the 11th, 40 members: on the 134th.
# EIGFORM_AFTER_USES >= 0 (LO_EIGFORM_AFTER_USES) fixes the count instead (0: with the first solve), -1: never; None: the model.
_e = os.environ.get("LO_EIGFORM_AFTER_USES")
EIGFORM_AFTER_USES = None if _e is None else int(_e)
del _e


def _eigform_due(uses: int, B: int) -> bool:
    if EIGFORM_AFTER_USES is not None:
        return EIGFORM_AFTER_USES >= 0 and uses > EIGFORM_AFTER_USES
    build_us = 450.0 + 0.45 * B
    gain_us = 3.5 * ((B + 63) // 64)
    return uses * gain_us >= build_us


def _cg_params(c, n_tridiag, max_iter, max_tridiag_iter, tolerance, eps, stop_updating_after, floor_max_iter,
               cls=_hip.CgParams):
    """lo_cg_params (or, cls=_hip.CgParamsF64, lo_cg_params_f64) of one solve."""
    prm = cls()
    prm.c, prm.n_tridiag, prm.max_iter, prm.max_tridiag_iter = c, n_tridiag, max_iter, max_tridiag_iter
    prm.floor_max_iter = floor_max_iter  # the reference's stop-rule floors use the unclipped max_iter (:303-305)
    prm.tolerance, prm.eps, prm.stop_updating_after = tolerance, eps, stop_updating_after
    return prm


def _tridiag_buffer(n_tridiag: int, B: int, max_tridiag_iter: int, like: torch.Tensor):
    if not n_tridiag:
        return None
    return torch.empty(n_tridiag, B, max_tridiag_iter, max_tridiag_iter, dtype=like.dtype, device=like.device)


def _cg_result(x: torch.Tensor, t_mat: Optional[torch.Tensor], info) -> CGResult:
    """CGResult from lo_cg_info / lo_cg_info_f64 / lo_fused_info; t_mat cropped to the iterations that filled it."""
    if t_mat is not None:
        m = info.last_tridiag_iter + 1
        t_mat = t_mat[:, :, :m, :m].contiguous()
    return CGResult(x, t_mat, info.iterations, info.matvecs, bool(info.tolerance_reached), bool(info.nan_detected),
                    bool(info.skipped), float(info.mean_residual))


_SESSIONS_PER_CACHE = 4    # (a cache serves one operator; a second entry is another tolerance or max_iter)
_SESSION_RETRY_AFTER = 32  # solves after which a refused creation is tried again (a cool-down ends, a switch is removed)


class _CgSession:
    """One lo_cg_session with what it needs kept alive: its workspace, the tensors its structs point to, and the result
    structs every solve fills.  handle None: the library refused the plan (LO_ERR_UNSUPPORTED) -- the general path."""

    __slots__ = ("handle", "ws", "keep", "info", "plan", "info_ref", "plan_ref", "retry", "busy", "_destroy")

    def __init__(self, lib, desc: "OperatorDescriptor", pre: "WoodburyPreconditioner", prm, dev):
        s, ps = desc.c_struct(), pre.c_struct()
        self.ws = _hip.workspace(lib.lo_cg_session_workspace_bytes(C.byref(s), C.byref(prm)), dev)
        self.keep = (desc.A0, desc.d, pre.Q, pre.dinv, pre.F, pre.EF, pre.E, pre.RS, pre.RSD)
        self.info, self.plan = _hip.CgInfo(), _hip.CgPlan()
        self.info_ref, self.plan_ref = C.byref(self.info), C.byref(self.plan)
        self.retry = _SESSION_RETRY_AFTER
        self.busy = threading.Lock()  # one solve at a time per session: a second thread takes the general path
        self._destroy = lib.lo_cg_session_destroy
        out = C.c_void_p()
        rc = lib.lo_cg_session_create_f32(C.byref(s), C.byref(ps), C.byref(prm), _hip.ptr(self.ws), self.ws.numel(),
                                          C.byref(out))
        if rc != _hip.LO_ERR_UNSUPPORTED:
            _hip.check(rc, "lo_cg_session_create_f32")
        self.handle = out.value if rc == 0 else None

    def close(self):
        if getattr(self, "handle", None) is not None:  # (absent: the constructor refused the descriptor)
            self._destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


def cg_sessions_live() -> int:
    """lo_cg_session_debug_live: native solve sessions alive in this process (tests)."""
    return int(_hip.load().lo_cg_session_debug_live())


_UNSET = object()
_fast_mode: Optional[bool] = None  # cg_fast_entry: True forced, False forbidden, None automatic
_fast_module = _UNSET              # _hip.fast(), once asked for


def _fast_resolve():
    global _fast_module
    _fast_module = _hip.fast()
    return _fast_module


def cg_fast_entry(mode: Optional[bool] = None) -> str:
    """Which binding calls lo_cg_session_solve_f32 for the session solves of `cg_solve`: True forces the native entry
    (csrc/lo_pyfast.cpp; an error where it is not built), False forbids it, None leaves it automatic (the native entry
    where it is built and imports).  Returns what is in force from now on: "native" or "ctypes"."""
    global _fast_mode
    if mode is not None and not isinstance(mode, bool):
        raise TypeError(f"cg_fast_entry takes True, False or None, not {mode!r}")
    mod = _fast_resolve()
    usable = mod is not None and _hip.RAW_STREAM is not None
    if mode is True and not usable:
        raise _hip.HipExtensionError(
            f"the native session entry is not available ({_hip._FAST_PATH}: not built, or it does not import); "
            "build it with `make -C linear_operator_amd/csrc`")
    _fast_mode = mode
    return "native" if usable and mode is not False else "ctypes"


def _session_solve(lib, desc: "OperatorDescriptor", pre: "WoodburyPreconditioner", rhs: torch.Tensor, rhs3: torch.Tensor,
                   params: tuple) -> Optional["CGResult"]:
    """The solve through the native session of (operator, cache, parameters), created on first use; None: the general path
    takes it (no session for this plan, or lo_cg_session_solve_f32 handed the call over)."""
    # (the operator by its POINTERS: the operator classes lower themselves to a fresh descriptor, with fresh views of the
    #  same storage, on every solve; the entry keeps the tensors it was made from alive, so no address is handed out again
    #  while it exists.  The cache's own tensors by identity: they are attributes of `pre`, replaced only by assignment.)
    # In front of the LRU, the session of the cache's last solve (always the LRU's newest entry): the same descriptor
    # object over the same tensors, the same parameters, the cache's tensors unchanged -- no key, no pointer is formed.
    m = pre._memo
    if (m is not None and m[1] is desc and m[2] is desc.A0 and m[3] is desc.d and m[4] == params and m[5] is pre.Q
            and m[6] is pre.dinv and m[7] is pre.RSD and m[8] == pre.generation and m[0].handle is not None):
        ent = m[0]
    else:
        key = (desc.A0.data_ptr(), 0 if desc.d is None else desc.d.data_ptr(), desc.kind, desc.diag_mode, desc.B, desc.N,
               desc.R, params, pre.generation, id(pre.Q), id(pre.dinv), id(pre.RSD))
        sessions = pre._sessions
        ent = sessions.get(key)
        if ent is None:
            max_iter, max_tridiag_iter, tolerance, eps, stop_updating_after, floor_max_iter = params
            prm = _cg_params(1, 0, max_iter, max_tridiag_iter, tolerance, eps, stop_updating_after, floor_max_iter)
            ent = sessions[key] = _CgSession(lib, desc, pre, prm, rhs.device)
            while len(sessions) > _SESSIONS_PER_CACHE:
                sessions.popitem(last=False)[1].close()
        else:
            sessions.move_to_end(key)
        if ent.handle is None:
            pre._memo = None
            ent.retry -= 1
            if ent.retry <= 0:
                del sessions[key]
            return None
        # (a descriptor rebuilt over the same storage finds its session by the key above and is remembered in its turn)
        pre._memo = (ent, desc, desc.A0, desc.d, params, pre.Q, pre.dinv, pre.RSD, pre.generation)
    if not ent.busy.acquire(False):
        return None
    try:
        x = torch.empty_like(rhs3)
        fast = _fast_module if _fast_mode is not False else None
        if fast is _UNSET:
            fast = _fast_resolve()
        if fast is not None and _hip.RAW_STREAM is not None:
            # csrc/lo_pyfast.cpp: the result structs on its stack, integers in, a tuple out
            rc, iterations, matvecs, reached, nan, skipped, residual, rspace = fast.session_solve(
                ent.handle, rhs3.data_ptr(), x.data_ptr(), _hip.RAW_STREAM(rhs3.get_device()))
            if rc == _hip.LO_ERR_UNSUPPORTED:
                return None
            _hip.check(rc, "lo_cg_session_solve_f32")
            if rspace == 2:
                pre.rs_uses += 1
            return CGResult(x if rhs3 is rhs else x.reshape(rhs.shape), None, iterations, matvecs, reached, nan, skipped,
                            residual)
        rc = lib.lo_cg_session_solve_f32(ent.handle, rhs3.data_ptr(), x.data_ptr(), ent.info_ref, ent.plan_ref,
                                         _hip.stream_ptr(rhs.device))
        if rc == _hip.LO_ERR_UNSUPPORTED:
            return None
        _hip.check(rc, "lo_cg_session_solve_f32")
        if ent.plan.rspace == 2:
            pre.rs_uses += 1
        return _cg_result(x if rhs3 is rhs else x.reshape(rhs.shape), None, ent.info)
    finally:
        ent.busy.release()


def cg_solve(desc: Optional[OperatorDescriptor], rhs: torch.Tensor, *, x0: Optional[torch.Tensor] = None,
             precond: Optional[WoodburyPreconditioner] = None, matvec_closure: Optional[Callable] = None,
             precond_closure: Optional[Callable] = None, closure_batch_shape=None, n_tridiag: int = 0,
             max_iter: int = 1000, max_tridiag_iter: int = 20, tolerance: float = 1.0, eps: float = 1e-10,
             stop_updating_after: float = 1e-10, floor_max_iter: int = 0,
             stop_reduce: Optional[Callable] = None, _retry: bool = False) -> CGResult:
    """lo_cg_solve_f32: the reference's linear_cg (utils/linear_cg.py:98-359) on the device.

    rhs [*batch, N, c].  Either `desc` (structured operator, fully native loop) or `matvec_closure`
    (opaque callable on [B,N,c] tensors).  `closure_batch_shape` reshapes [B,...] back for closures.
    """
    lib = _hip.load()
    _hip.require_hip(rhs, x0)
    shape = rhs.shape
    N, c = shape[-2:]
    if len(shape) == 3 and rhs.is_contiguous():  # (no view of what is [B, N, c] already)
        rhs3, B = rhs, shape[0]
    else:
        rhs3 = _flat(rhs, 2)
        B = rhs3.shape[0]
    x03 = None if x0 is None else _flat(x0.expand_as(rhs), 2)
    dev = rhs.device
    if desc is None:
        if matvec_closure is None:
            raise ValueError("need an operator descriptor or a matvec closure")
        s = _callback_desc(B, N)
    else:
        if desc.B != B or desc.N != N:
            raise RuntimeError(f"cg_solve: rhs {tuple(rhs.shape)} does not match operator batch {desc.B}, N {desc.N}")
        # The headline solve -- one column on a cache that carries the diagonal form -- through its native session: nothing
        # below depends on the right-hand side, and the session did it once.  LO_CG_NO_SESSION: everything below, always.
        if (precond is not None and precond.RSD is not None and precond.RS is not None and c == 1 and not n_tridiag
                and desc.kind == _hip.LO_OP_LOWRANK_DIAG and desc.A0 is not None
                and x0 is None and stop_reduce is None and precond_closure is None and not _retry
                and "LO_CG_NO_SESSION" not in os.environ):
            res = _session_solve(lib, desc, precond, rhs, rhs3,
                                 (max_iter, max_tridiag_iter, tolerance, eps, stop_updating_after, floor_max_iter))
            if res is not None:
                return res
        s = desc.c_struct()
    bshape = tuple(closure_batch_shape) if closure_batch_shape is not None else tuple(rhs.shape[:-2])
    mv_cb, mv_err = _wrap_closure(matvec_closure, dev, bshape) if desc is None else _NO_CLOSURE
    pc_cb, pc_err = _wrap_closure(precond_closure, dev, bshape) if precond_closure is not None else _NO_CLOSURE
    # The diagonal form (0.5 - 0.7 ms of Jacobi work, 25 MB at 512 x 32, one blocking read-back) is built once the cache has
    # served enough solves ON THE RESIDENT R-SPACE KERNEL to pay for it: solves that kernel does not take (members beyond its
    # range, the batch-global stop rule, a cool-down of the resident kernels, LO_OC_NO_RSPACE) are not counted -- they are
    # counted AFTER the solve, from what lo_cg_last_executed says ran.
    rs_candidate = (precond is not None and precond.RS is not None and c == 1 and not n_tridiag and x0 is None
                    and stop_reduce is None and not _retry)
    if rs_candidate and precond.RSD is None and precond.rsd_refused is None and _eigform_due(precond.rs_uses + 1, B) \
            and (precond.rs_uses > 0 or EIGFORM_AFTER_USES is not None):
        precond.ensure_eigform()
    if stop_reduce is not None and precond is not None and precond.Q is None and precond_closure is None:
        # batch-global stop rule over ranks: a root-form-only cache could send THIS rank through the "unsupported -> build Q
        # -> start over" retry below while another rank continues -- the collective counts would diverge.  Q up front.
        precond.ensure_q()
    pre_s = precond.c_struct() if precond is not None else None
    pre_p = _byref(pre_s)
    prm = _cg_params(c, n_tridiag, max_iter, max_tridiag_iter, tolerance, eps, stop_updating_after, floor_max_iter)
    sr_err = []
    if stop_reduce is not None:  # batch-global stopping rule over the ranks of a process group (distributed.py)
        def _sr(user, vals):
            try:
                out = stop_reduce([vals[0], vals[1], vals[2]])
                vals[0], vals[1], vals[2] = float(out[0]), float(out[1]), float(out[2])
                return 0
            except BaseException as e:  # noqa: BLE001 -- must not unwind through C
                sr_err.append(e)
                return 1

        sr_cb = _hip.STOP_REDUCE_CB(_sr)  # (held here for the call: the struct stores its address)
        prm.stop_reduce = sr_cb
    ws = _hip.workspace(lib.lo_cg_workspace_bytes(C.byref(s), pre_p, C.byref(prm)), dev)
    x = torch.empty_like(rhs3)
    t_mat = _tridiag_buffer(n_tridiag, B, max_tridiag_iter, rhs3)
    info = _hip.CgInfo()
    # (called directly, not through _launch: LO_ERR_UNSUPPORTED is a decision, and this is the headline solve's path)
    rc = lib.lo_cg_solve_f32(C.byref(s), mv_cb, None, pre_p, pc_cb, None, C.byref(prm), _hip.ptr(rhs3), _hip.ptr(x03),
                             _hip.ptr(x), _hip.ptr(t_mat), _hip.ptr(ws), ws.numel(), C.byref(info),
                             _hip.stream_ptr(dev))
    _reraise(mv_err, pc_err, sr_err)
    if rc == _hip.LO_ERR_UNSUPPORTED and precond is not None and precond.Q is None:
        # root-form-only preconditioner and the operator-resident kernels could not take the solve (shape outside
        # their range, or a group hand-off timed out): build the generic Q form and run again
        precond.ensure_q()
        return cg_solve(desc, rhs, x0=x0, precond=precond, matvec_closure=matvec_closure,
                        precond_closure=precond_closure, closure_batch_shape=closure_batch_shape, n_tridiag=n_tridiag,
                        max_iter=max_iter, max_tridiag_iter=max_tridiag_iter, tolerance=tolerance, eps=eps,
                        stop_updating_after=stop_updating_after, floor_max_iter=floor_max_iter, stop_reduce=stop_reduce,
                        _retry=True)
    _hip.check(rc, "lo_cg_solve_f32")
    if rs_candidate:
        ex = _hip.CgPlan()
        if lib.lo_cg_last_executed(C.byref(ex)) == 0 and ex.rspace == 2:
            precond.rs_uses += 1
    return _cg_result(x.reshape(rhs.shape), t_mat, info)


def _plan_dict(pl) -> dict:
    return dict(resident=bool(pl.resident), resident_iterations=pl.resident_iterations, lockstep_cols=pl.lockstep_cols,
                lockstep_group=pl.lockstep_group, serial_engine=_hip.ENGINE_NAMES[pl.serial_engine],
                serial_group=pl.serial_group, lean=bool(pl.lean), needs_q=bool(pl.needs_q),
                streaming_precond=_hip.STREAM_PRE_NAMES[pl.streaming_precond], poll_chunk=pl.poll_chunk,
                first_stop_iteration=pl.first_stop_iteration, streaming_iterations=pl.streaming_iterations,
                rspace={0: "none", 1: "cols", 2: "resident"}[pl.rspace], rspace_diag=bool(pl.rspace_diag))


def cg_plan(desc: OperatorDescriptor, c: int, *, precond: Optional[WoodburyPreconditioner] = None, has_x0: bool = False,
            has_precond_closure: bool = False, n_tridiag: int = 0, max_iter: int = 1000, max_tridiag_iter: int = 20,
            floor_max_iter: int = 0, global_rule: bool = False, cus: int = 0) -> dict:
    """lo_cg_plan_f32: which engines `cg_solve` will run for these arguments (pure; nothing is launched).  cus = 0:
    this device."""
    s = desc.c_struct()
    pre_s = precond.c_struct() if precond is not None else None
    prm = _cg_params(c, n_tridiag, max_iter, max_tridiag_iter, 1.0, 1e-10, 1e-10, floor_max_iter)
    if global_rule:
        prm.stop_reduce = _hip.STOP_REDUCE_CB(lambda user, vals: 0)
    out = _hip.CgPlan()
    _hip.call("lo_cg_plan_f32", C.byref(s), _byref(pre_s), int(has_precond_closure), int(has_x0), C.byref(prm),
              int(cus), C.byref(out))
    return _plan_dict(out)


def cg_last_executed() -> dict:
    """lo_cg_last_executed: the plan the calling thread's last `cg_solve` actually ran (after run-time fall-backs)."""
    out = _hip.CgPlan()
    _hip.call("lo_cg_last_executed", C.byref(out))
    return _plan_dict(out)


@dataclass
class FusedSolveResult:
    """Outcome of the one-launch end-to-end solve: the linear_cg result, the root-form preconditioner it built on the
    way (for later solves with the same operator) and the recorded pivots."""

    cg: CGResult
    precond: WoodburyPreconditioner  # root form only (Q is None); `source` is None: L was never materialised
    swaps: torch.Tensor  # [B, rank] int32: position exchanged with position m at pivot m
    rank: int

    def permutation(self, N: int) -> torch.Tensor:
        """The reference's permutation [B, N] int64 (_pivoted_cholesky.py:47-48, :67-70) from the recorded exchanges."""
        B = self.swaps.shape[0]
        perm = torch.empty(B, N, dtype=torch.int64, device=self.swaps.device)
        _launch("lo_solve_fused_perm", perm.device, self.swaps, B, N, self.rank, perm)
        return perm


_fused_ws_bytes: dict = {}  # workspace size of lo_solve_fused_f32 per (B, rank, c, max_iter, floor): a pure function


def solve_fused_supported(desc: Optional[OperatorDescriptor], c: int, rank: int, max_iter: int = 1000,
                          floor_max_iter: int = 0) -> bool:
    """True if lo_solve_fused_f32 takes this operator / right-hand side shape (see include/lo_amd.h)."""
    if (desc is None or desc.kind != _hip.LO_OP_LOWRANK_DIAG or desc.A0 is None or not desc.A0.is_cuda
            or desc.dtype != torch.float32):
        return False
    prm = _cg_params(c, 0, max_iter, min(20, max_iter), 1.0, 1e-10, 1e-10, floor_max_iter)
    s = desc.c_struct()
    return bool(_hip.load().lo_solve_fused_supported(C.byref(s), int(rank), C.byref(prm)))


def solve_fused(desc: OperatorDescriptor, rhs: torch.Tensor, rank: int, error_tol: float = 1e-3, *,
                max_iter: int = 1000, tolerance: float = 1.0, eps: float = 1e-10, stop_updating_after: float = 1e-10,
                floor_max_iter: int = 0) -> Optional[FusedSolveResult]:
    """lo_solve_fused_f32: pivoted Cholesky (rank pivots) -> root-form preconditioner -> preconditioned CG of
    AddedDiag(LowRankRoot, Diag) in ONE resident launch, the operator read once.  Returns None when the result would
    not be the reference's (a member's own pivot error reached the tolerance before `rank` pivots, the CG tolerance was
    not met at the iteration floor, or a group exchange timed out): the caller then takes the three-launch path."""
    lib = _hip.load()
    _hip.require_hip(rhs)
    N, c = rhs.shape[-2:]
    rhs3 = _flat(rhs, 2)
    B = rhs3.shape[0]
    if desc.B != B or desc.N != N:
        raise RuntimeError(f"solve_fused: rhs {tuple(rhs.shape)} does not match operator batch {desc.B}, N {desc.N}")
    dev = rhs.device
    rank = min(int(rank), N)
    prm = _cg_params(c, 0, max_iter, min(20, max_iter), tolerance, eps, stop_updating_after, floor_max_iter)
    s = desc.c_struct()  # (shapes the kernel does not take come back as LO_ERR_UNSUPPORTED from the call itself)
    R = desc.R
    const = desc.diag_mode == _hip.LO_DIAG_CONST
    x = torch.empty_like(rhs3)
    small = torch.empty(B * (3 * R * R + 1 + rank), dtype=torch.float32, device=dev)  # one allocation: F | EF | E | logdet | swaps
    F, EF, E = (small[i * B * R * R:(i + 1) * B * R * R].view(B, R, R) for i in range(3))
    logdet = small[3 * B * R * R:3 * B * R * R + B]
    swaps = small[3 * B * R * R + B:].view(torch.int32).view(B, rank)
    dinv = torch.empty(B if const else (B, N), dtype=torch.float32, device=dev)
    wkey = (B, rank, c, max_iter, floor_max_iter)
    nbytes = _fused_ws_bytes.get(wkey)
    if nbytes is None:
        nbytes = _fused_ws_bytes[wkey] = lib.lo_solve_fused_workspace_bytes(C.byref(s), rank, C.byref(prm))
    ws = _hip.workspace(nbytes, dev)
    info = _hip.FusedInfo()
    rc = lib.lo_solve_fused_f32(C.byref(s), rank, float(error_tol), C.byref(prm), _hip.ptr(rhs3), _hip.ptr(x),
                                _hip.ptr(F), _hip.ptr(EF), _hip.ptr(E), _hip.ptr(dinv), _hip.ptr(logdet),
                                _hip.ptr(swaps), _hip.ptr(ws), ws.numel(), C.byref(info), _hip.stream_ptr(dev))
    if rc == _hip.LO_ERR_UNSUPPORTED:
        return None
    _hip.check(rc, "lo_solve_fused_f32")
    if info.status != _hip.LO_FUSED_OK:
        return None
    pre = WoodburyPreconditioner(None, dinv, rank, const, logdet.reshape(desc.batch_shape) if desc.batch_shape else logdet,
                                 F, EF, E)
    return FusedSolveResult(_cg_result(x.reshape(rhs.shape), None, info), pre, swaps, rank)


def cg_solve_f64(A: Optional[torch.Tensor], diag: Optional[torch.Tensor], rhs: torch.Tensor, *,
                 x0: Optional[torch.Tensor] = None, matvec_closure: Optional[Callable] = None,
                 precond_closure: Optional[Callable] = None, n_tridiag: int = 0, max_iter: int = 1000,
                 max_tridiag_iter: int = 20, tolerance: float = 1.0, eps: float = 1e-10,
                 stop_updating_after: float = 1e-10, floor_max_iter: int = 0,
                 desc: Optional[OperatorDescriptor] = None, precond: Optional[tuple] = None) -> CGResult:
    """lo_cg_solve_f64: the reference's linear_cg (utils/linear_cg.py:98-359) with float64 operands -- what every case
    of the reference's test/utils/test_linear_cg.py runs.  `A` [*batch, N, N] (+ `diag` [*batch, N]) is multiplied by
    the library's fp64 kernel, a float64 descriptor `desc` (in place of `A` / `matvec_closure`) by lo_matvec_f64 inside
    the library; otherwise `matvec_closure` is called back once per product.  `precond`: the cached pair (Q, noise,
    constant_diag) of the float64 Woodbury preconditioner, applied inside the library (in place of `precond_closure`:
    any callable or None)."""
    lib = _hip.load()
    _hip.require_hip(rhs, x0, A, diag, dtype=torch.float64)
    N, c = rhs.shape[-2:]
    rhs3 = _flat(rhs, 2)
    B = rhs3.shape[0]
    dev = rhs.device
    bshape = tuple(rhs.shape[:-2])
    x03 = None if x0 is None else _flat(x0.expand_as(rhs), 2)
    A3, d2, mv_cb, mv_user, pc_cb, pc_user, errors, keep = _f64_operands(
        lib, A, diag, desc, matvec_closure, precond, precond_closure, bshape, B, N, c, dev)
    prm = _cg_params(c, n_tridiag, max_iter, max_tridiag_iter, tolerance, eps, stop_updating_after, floor_max_iter,
                     _hip.CgParamsF64)
    x = torch.empty_like(rhs3)
    t_mat = _tridiag_buffer(n_tridiag, B, max_tridiag_iter, rhs3)
    info = _hip.CgInfoF64()
    _launch("lo_cg_solve_f64", dev, A3, d2, mv_cb, mv_user, pc_cb, pc_user, C.byref(prm), B, N, rhs3, x03, x, t_mat,
            ws_bytes=lib.lo_cg_f64_workspace_bytes(B, N, C.byref(prm)), info=info, errors=errors)
    del keep  # (the solver is synchronous: the contexts and workspaces of the callbacks were needed until here)
    return _cg_result(x.reshape(rhs.shape), t_mat, info)


def precond_apply(pre: WoodburyPreconditioner, r: torch.Tensor) -> torch.Tensor:
    lib = _hip.load()
    _hip.require_hip(r)
    N, c = r.shape[-2:]
    r3 = _flat(r, 2)
    B = r3.shape[0]
    z = torch.empty_like(r3)
    s = pre.ensure_q().c_struct()
    _launch("lo_precond_apply_f32", r.device, C.byref(s), r3, z, B, N, c,
            ws_bytes=lib.lo_precond_apply_workspace_bytes(B, N, pre.k, c))
    return z.reshape(r.shape)


def probe_vectors(L: torch.Tensor, d: torch.Tensor, e1: torch.Tensor, e2: torch.Tensor,
                  inv_quad_rhs: Optional[torch.Tensor], batch_shape) -> tuple:
    """lo_probe_vectors_f32: the probe vectors of InvQuadLogdet.forward (functions/_inv_quad_logdet.py:91-110, :131) for
    the preconditioner L L^T + Diag(d): z = L e1 + sqrt(d) o e2, normalised, with the inv_quad columns behind them.
    L [*b, N, k] (any strides, broadcast batch), d [*b, N] or [*b, 1] / [*b] (constant), e1 [*batch, k, P], e2 [*batch, N, P].
    Returns (rhs [*batch, N, P + q], norms [*batch, 1, P]); the probes are rhs[..., :P]."""
    lib = _hip.load()
    bs = tuple(batch_shape)
    N, P = e2.shape[-2:]
    k = L.shape[-1]
    e13, e23 = _flat(e1.expand(*bs, k, P), 2), _flat(e2.expand(*bs, N, P), 2)
    B = e23.shape[0]
    _hip.require_hip(L, d, e13, e23, inv_quad_rhs)
    Lx = L.expand(*bs, N, k)
    if len(bs) > 1:  # (one batch stride is all the kernel takes: several batch dimensions are flattened by a copy)
        Lx = Lx.reshape(B, N, k)
    elif len(bs) == 0:
        Lx = Lx.unsqueeze(0)
    const = d.shape[-1] == 1 and N != 1
    d2 = (d.expand(*bs, 1) if const else d.expand(*bs, N)).contiguous().reshape(B, -1)
    q = 0 if inv_quad_rhs is None else inv_quad_rhs.shape[-1]
    iq3 = None if inv_quad_rhs is None else _flat(inv_quad_rhs.expand(*bs, N, q), 2)
    dev = e2.device
    out = torch.empty(B, N, P + q, dtype=torch.float32, device=dev)
    norms = torch.empty(B, P, dtype=torch.float32, device=dev)
    _launch("lo_probe_vectors_f32", dev, Lx, Lx.stride(0), Lx.stride(1), Lx.stride(2), k, d2,
            _hip.LO_DIAG_CONST if const else _hip.LO_DIAG_FULL, e13, e23, iq3, q, B, N, P, out, norms,
            ws_bytes=lib.lo_probe_vectors_workspace_bytes(B, N, P))
    return out.reshape(*bs, N, P + q), norms.reshape(*bs, 1, P)


def iql_backward_factors(solves: torch.Tensor, pp: torch.Tensor, norms: torch.Tensor, g_ld: torch.Tensor,
                         g_iq: Optional[torch.Tensor], P: int):
    """lo_iql_backward_factors_f32: the element-wise part of InvQuadLogdet.backward (functions/_inv_quad_logdet.py:183-213)
    in one pass.  solves [*batch, N, P + q]; pp [*batch, N, >= P] the preconditioner applied to the NORMALISED probes;
    norms [*batch, 1, P]; g_ld [*batch]; g_iq [*batch, q] or None.  Returns (left, right [*batch, N, P + q], pre_left,
    pre_right [*batch, N, P])."""
    bs = solves.shape[:-2]
    N, c = solves.shape[-2:]
    q = c - P
    s3, p3 = _flat(solves, 2), _flat(pp, 2)
    B = s3.shape[0]
    n2 = norms.expand(*bs, 1, P).contiguous().reshape(B, P)
    gl = g_ld.expand(bs).contiguous().reshape(B).to(torch.float32)
    gq = None if (g_iq is None or q == 0) else g_iq.expand(*bs, q).contiguous().reshape(B, q).to(torch.float32)
    _hip.require_hip(s3, p3, n2, gl, gq)
    left, right = torch.empty_like(s3), torch.empty_like(s3)
    pre_left = torch.empty(B, N, P, dtype=torch.float32, device=s3.device)
    pre_right = torch.empty_like(pre_left)
    _launch("lo_iql_backward_factors_f32", s3.device, s3, p3, p3.shape[-1], n2, gl, gq, 1.0 / P, B, N, P, q, left, right,
            pre_left, pre_right)
    return (left.reshape(*bs, N, c), right.reshape(*bs, N, c), pre_left.reshape(*bs, N, P), pre_right.reshape(*bs, N, P))


# ------------------------------------------------------------------------------------------------
def _pivchol_out(L_rows: torch.Tensor, perm: torch.Tensor, m: int, batch_shape, contiguous: bool):
    """(L [*batch, N, m], permutation [*batch, N]) from the [B, max_rank, N] rows the kernels wrote and the m pivots taken."""
    N = L_rows.shape[-1]
    L = L_rows[:, :m, :].mT  # _pivoted_cholesky.py:105
    if contiguous:
        L = L.contiguous()
    return L.reshape(*batch_shape, N, m), perm.reshape(*batch_shape, N)


def pivoted_cholesky(desc: OperatorDescriptor, rank: int, error_tol: float = 1e-3, contiguous: bool = True):
    """lo_pivoted_cholesky_f32: PivotedCholesky.forward (functions/_pivoted_cholesky.py:14-105) of the
    NON-diagonal part of `desc`.  Returns (L [*batch, N, m], permutation [*batch, N] int64).
    contiguous=False skips the transposed copy of :105 and returns L as a strided view of the [B, m, N] rows the
    kernels write (what precond_build consumes directly)."""
    lib = _hip.load()
    dev = desc.device
    B, N = desc.B, desc.N
    max_rank = min(int(rank), N)
    L_rows = torch.empty(B, max_rank, N, dtype=torch.float32, device=dev)
    perm = torch.empty(B, N, dtype=torch.int64, device=dev)
    s = desc.without_diag().c_struct()
    m = C.c_int32(0)
    _launch("lo_pivoted_cholesky_f32", dev, C.byref(s), max_rank, float(error_tol), L_rows, perm, C.byref(m),
            ws_bytes=lib.lo_pivoted_cholesky_workspace_bytes(C.byref(s), max_rank))
    return _pivchol_out(L_rows, perm, m.value, tuple(desc.batch_shape), contiguous)


def pivoted_cholesky_generic(diag: torch.Tensor, row_fetch: Callable, rank: int, error_tol: float = 1e-3,
                             contiguous: bool = True):
    """lo_pivoted_cholesky_cb_f32: PivotedCholesky.forward for an operator that does not lower to a descriptor.
    diag [*batch, N] = matrix._diagonal(); row_fetch(piv [*batch] int64 device tensor) -> rows [*batch, N] is the
    reference's generic row access `matrix[..., pi_m, :]` (_pivoted_cholesky.py:81), called once per pivot without a
    host synchronisation; pivot search, Schur update and the stopping rule run in the same kernels as for lowered
    operators.  Returns (L [*batch, N, m], permutation [*batch, N])."""
    lib = _hip.load()
    f64 = diag.dtype == torch.float64  # (round 4: the reference is dtype-generic; same kernels instantiated for double)
    _hip.require_hip(diag, dtype=diag.dtype if f64 else torch.float32)
    dev = diag.device
    bs = tuple(diag.shape[:-1])
    N = diag.shape[-1]
    d2 = _flat(diag, 1)
    B = d2.shape[0]
    max_rank = min(int(rank), N)
    L_rows = torch.empty(B, max_rank, N, dtype=diag.dtype, device=dev)
    perm = torch.empty(B, N, dtype=torch.int64, device=dev)
    err = []

    def cb(user, piv_ptr, rows_ptr, B_, N_, stream):
        try:
            piv = _hip.as_tensor(piv_ptr, (B_,), dev, "<i8")
            rows = _hip.as_tensor(rows_ptr, (B_, N_), dev, "<f8" if f64 else "<f4")
            rows.copy_(row_fetch(piv.reshape(bs)).reshape(B_, N_))
            return 0
        except BaseException as e:  # noqa: BLE001 -- must not unwind through C
            err.append(e)
            return 1

    m = C.c_int32(0)
    ws_bytes = (lib.lo_pivoted_cholesky_cb_f64_workspace_bytes if f64 else lib.lo_pivoted_cholesky_cb_workspace_bytes)
    _launch("lo_pivoted_cholesky_cb_f64" if f64 else "lo_pivoted_cholesky_cb_f32", dev, B, N, d2, _hip.ROWFETCH_CB(cb),
            None, max_rank, float(error_tol), L_rows, perm, C.byref(m), ws_bytes=ws_bytes(B, N, max_rank), errors=(err,))
    return _pivchol_out(L_rows, perm, m.value, bs, contiguous)


def _root_form(lib, root, perm, L3, d, constant_diag, B, N, k, dev) -> WoodburyPreconditioner:
    R = root.shape[-1]
    C3 = _flat(root, 2)
    p2 = _flat(perm, 1)
    ld = padded_rank(R)
    F = torch.empty(B, ld, ld, dtype=torch.float32, device=dev)
    EF = torch.empty_like(F)
    E = torch.empty_like(F)
    d2, mode, dinv = _diag_operand(d, B, N, constant_diag, want_dinv=True)
    logdet = torch.empty(B, dtype=torch.float32, device=dev)
    if R % 4 == 0 and C3.data_ptr() % 16 == 0 and not os.environ.get("LO_NO_RSPACE_FORM"):
        # with the R-space form: E and C^T C on the fp64 matrix cores (the fp32 F / EF / E are roundings of the same)
        RS = torch.empty(B, 6, ld, ld, dtype=torch.float64, device=dev)
        _launch("lo_precond_root_form_rs_f32", dev, C3, R, d2, mode, L3, *_row_strides(L3), p2, B, N, k, ld, F, EF, E,
                dinv, logdet, RS, ws_bytes=lib.lo_precond_root_form_rs_workspace_bytes(B, N, R))
        return WoodburyPreconditioner(None, dinv, k, constant_diag, logdet, F, EF, E, RS, rs_rank=R)
    _launch("lo_precond_root_form_f32", dev, C3, R, d2, mode, L3, *_row_strides(L3), p2, B, N, k, ld, F, EF, E, dinv,
            logdet, ws_bytes=lib.lo_precond_root_form_workspace_bytes(B, N, R))
    return WoodburyPreconditioner(None, dinv, k, constant_diag, logdet, F, EF, E)


# the Kronecker root form multiplies the fp32 rounding of KP^T (r/d) by `kappa` (lo_amd.h); beyond this bound the
# pivot rows are too close to dependent for 1e-4 solves and the orthonormal Q form is kept
KRON_ROOT_MAX_KAPPA = 200.0


def _kron_root(lib, desc: "OperatorDescriptor", perm, L3, k, dev):
    """lo_precond_kron_root_f32 for a Kronecker operator with a constant diagonal (descriptor with the diagonal
    attached) -> ((kron_a, kron_b, kron_F) or None when some member's pivot rows are too ill conditioned, worst kappa);
    one read-back of B floats."""
    B, n1, n2 = desc.B, desc.R, desc.n2
    ka = torch.empty(B, n1, 16, dtype=torch.float32, device=dev)
    kb = torch.empty(B, n2, 16, dtype=torch.float32, device=dev)
    kF = torch.empty(B, 16, 16, dtype=torch.float32, device=dev)
    kappa = torch.empty(B, dtype=torch.float32, device=dev)
    p2 = _flat(perm, 1)
    s = desc.c_struct()
    _launch("lo_precond_kron_root_f32", dev, C.byref(s), L3, *_row_strides(L3), p2, k, ka, kb, kF, kappa,
            ws_bytes=lib.lo_precond_kron_root_workspace_bytes(B))
    worst = float(kappa.max())
    if not (worst < KRON_ROOT_MAX_KAPPA):  # (also NaN)
        return None, worst
    return (ka, kb, kF), worst


def padded_rank(k: int) -> int:
    rq, p = (k + 3) // 4, 1
    while p < rq:
        p <<= 1
    return 4 * p


def precond_build(L: torch.Tensor, d: torch.Tensor, constant_diag: bool, root: Optional[torch.Tensor] = None,
                  perm: Optional[torch.Tensor] = None, need_q: bool = True,
                  kron: Optional["OperatorDescriptor"] = None) -> WoodburyPreconditioner:
    """lo_precond_build_f32: AddedDiagLinearOperator._init_cache* (added_diag_linear_operator.py:144-184).
    L [*batch, N, k]; d [*batch, N] (or [*batch] when constant_diag).
    root, perm: the root C [*batch, N, R <= 32] of the low-rank operator L was factored from and the permutation
    pivoted_cholesky returned -- adds the ROOT FORM (lo_precond_root_form_f32) the operator-resident CG kernels
    prefer (one all-reduce per iteration, no second tall matrix); need_q=False then skips the generic Q.
    kron, perm: the descriptor (LO_OP_KRON_DIAG, constant diagonal) of the Kronecker operator L was factored from --
    adds the Kronecker root form (lo_precond_kron_root_f32) for the single-column CG of 8192 <= N <= 65536."""
    lib = _hip.load()
    _hip.require_hip(L, d)
    N, k = L.shape[-2:]
    L3 = L.reshape(-1, N, k)  # stays a view for the strided rows layout pivoted_cholesky(contiguous=False) returns
    if min(L3.stride()) < 0 or L3.dtype != torch.float32:
        L3 = L3.contiguous()
    B = L3.shape[0]
    dev = L.device
    if root is not None and perm is not None and root.shape[-1] <= 32 and 1 <= k <= 32:
        rf = _root_form(lib, root, perm, L3, d, constant_diag, B, N, k, dev)
        rf.source = (L, d)
        if not need_q:
            return rf
        full = precond_build(L, d, constant_diag)
        full.F, full.EF, full.E, full.RS, full.source = rf.F, rf.EF, rf.E, rf.RS, rf.source
        full.rs_rank = rf.rs_rank
        return full
    ldq = padded_rank(k)
    Q = torch.empty(B, N, ldq, dtype=torch.float32, device=dev)
    d2, mode, dinv = _diag_operand(d, B, N, constant_diag, want_dinv=True)
    logdet = torch.empty(B, dtype=torch.float32, device=dev)
    _launch("lo_precond_build_strided_f32", dev, L3, *_row_strides(L3), d2, mode, B, N, k, Q, dinv, logdet,
            ws_bytes=lib.lo_precond_build_workspace_bytes(B, N, k))
    out = WoodburyPreconditioner(Q, dinv, k, constant_diag, logdet.reshape(L.shape[:-2]))
    if (kron is not None and perm is not None and constant_diag and kron.kind == _hip.LO_OP_KRON_DIAG
            and kron.diag_mode == _hip.LO_DIAG_CONST and kron.B == B and kron.N == N and 1 <= k <= 16
            and 8192 <= N <= 65536):
        out.kron, out.kron_kappa = _kron_root(lib, kron, perm, L3, k, dev)
    return out


def tridiag_eigh_slq(t_mat: torch.Tensor, n: int, want_evecs: bool = False, want_logdet: bool = True):
    """lo_tridiag_eigh_slq_f32 on t_mat [P, *batch, T, T] -> (evals [P,*batch,T], evecs or None, logdet [*batch])."""
    lib = _hip.load()
    _hip.require_hip(t_mat)
    P = t_mat.shape[0]
    T = t_mat.shape[-1]
    batch = t_mat.shape[1:-2]
    t3 = t_mat.contiguous().reshape(-1, T, T)
    B = t3.shape[0] // P
    dev = t_mat.device
    evals = torch.empty(P * B, T, dtype=torch.float32, device=dev)
    evecs = torch.empty(P * B, T, T, dtype=torch.float32, device=dev) if want_evecs else None
    logdet = torch.empty(B, dtype=torch.float32, device=dev) if want_logdet else None
    _launch("lo_tridiag_eigh_slq_f32", dev, t3, P, B, T, int(n), evals, evecs, logdet,
            ws_bytes=lib.lo_tridiag_eigh_slq_workspace_bytes(P, B))
    return (evals.reshape(P, *batch, T), None if evecs is None else evecs.reshape(P, *batch, T, T),
            None if logdet is None else logdet.reshape(batch))


def lanczos_tridiag(desc: Optional[OperatorDescriptor], init_vecs: torch.Tensor, max_iter: int, tol: float = 1e-5,
                    matvec_closure: Optional[Callable] = None, contiguous: bool = False):
    """lo_lanczos_tridiag_f32: utils/lanczos.py:9-164.  init_vecs [*batch, N, P].
    Returns (q_mat [P,*batch,N,k'], t_mat [P,*batch,k',k']) with the reference's output shapes (:151-161); q_mat is a
    strided view of the basis as the kernels wrote it unless `contiguous=True` asks for the reference's memory layout
    (one more pass over the basis: lo_lanczos_permute_f32)."""
    lib = _hip.load()
    _hip.require_hip(init_vecs)
    N, P = init_vecs.shape[-2:]
    batch = tuple(init_vecs.shape[:-2])
    v3 = _flat(init_vecs, 2)
    B = v3.shape[0]
    dev = init_vecs.device
    s, cb, err = _f32_operator(desc, matvec_closure, batch, B, N, dev)
    max_iter = int(max_iter)
    q, t = _lanczos_buffers(max_iter, v3)
    iters = C.c_int32(0)
    _launch("lo_lanczos_tridiag_f32", dev, C.byref(s), cb, None, v3, P, max_iter, float(tol), q, t, C.byref(iters),
            ws_bytes=lib.lo_lanczos_workspace_bytes(C.byref(s), P, max_iter), errors=(err,))
    k = iters.value
    q_out = None
    if contiguous:
        q_out = torch.empty(P, *batch, N, k, dtype=torch.float32, device=dev)
        rc = lib.lo_lanczos_permute_f32(_hip.ptr(q), k, B, N, P, _hip.ptr(q_out), _hip.stream_ptr(dev))  # lanczos.py:154
        if rc == _hip.LO_ERR_UNSUPPORTED:
            q_out = q[:k].reshape(k, *batch, N, P).permute(-1, *range(1, 1 + len(batch)), -2, 0).contiguous()
        else:
            _hip.check(rc, "lo_lanczos_permute_f32")
    return _lanczos_out(q, t, k, batch, q_out)


def _lanczos_buffers(max_iter: int, v3: torch.Tensor):
    """The basis [max_iter, B, N, P] and the tridiagonals [max_iter, max_iter, B, P] as the step kernels write them."""
    B, N, P = v3.shape
    return (torch.empty(max_iter, B, N, P, dtype=v3.dtype, device=v3.device),
            torch.empty(max_iter, max_iter, B, P, dtype=v3.dtype, device=v3.device))


def _lanczos_out(q: torch.Tensor, t: torch.Tensor, k: int, batch, q_out: Optional[torch.Tensor] = None):
    """(q_mat [P, *batch, N, k], t_mat [P, *batch, k, k]) of the reference (lanczos.py:151-161) from the buffers after k
    steps; q_out: the basis already in the reference's memory layout."""
    nb = len(batch)
    N, P = q.shape[-2:]
    if q_out is None:
        # the reference's q_mat [P, *batch, N, k] (lanczos.py:154) as a VIEW of the basis in the layout the step kernels
        # write it ([k, B, N, P]): same shape, same values, no 5 GB copy at the cfg3 shape.  The consumers on the path
        # (root_from_lanczos below) read this layout directly; anything else sees an ordinary strided tensor.
        # (an early stop -- k well below the allocated steps -- must not keep the whole basis buffer alive behind the view:
        #  ADVICE r4)
        qk = q[:k] if k == q.shape[0] else q[:k].clone()
        q_out = qk.reshape(k, *batch, N, P).permute(-1, *range(1, 1 + nb), -2, 0)
    t_out = t[:k, :k].reshape(k, k, *batch, P).permute(-1, *range(2, 2 + nb), 0, 1).contiguous()  # :156
    if P == 1:  # squeeze_(0) (:159-161) only acts on a size-1 leading dim
        q_out, t_out = q_out[0], t_out[0]
    return q_out, t_out


def lanczos_tridiag_f64(A: Optional[torch.Tensor], diag: Optional[torch.Tensor], init_vecs: torch.Tensor,
                        max_iter: int, tol: float = 1e-5, matvec_closure: Optional[Callable] = None,
                        desc: Optional[OperatorDescriptor] = None):
    """lo_lanczos_tridiag_f64: utils/lanczos.py:9-164 with float64 operands (the reference is dtype-generic).  `A`
    [*batch, N, N] (+ `diag` [*batch, N]) is multiplied by the library's fp64 kernel, a float64 descriptor `desc` by
    lo_matvec_f64 inside the library, otherwise `matvec_closure` is called back once per step.  Same return shapes as
    `lanczos_tridiag`; q_mat is the permuted view of the basis."""
    lib = _hip.load()
    _hip.require_hip(init_vecs, A, diag, dtype=torch.float64)
    N, P = init_vecs.shape[-2:]
    batch = tuple(init_vecs.shape[:-2])
    v3 = _flat(init_vecs, 2)
    B = v3.shape[0]
    dev = init_vecs.device
    A3, d2, cb, user, _, _, errors, keep = _f64_operands(lib, A, diag, desc, matvec_closure, None, None, batch, B, N, P,
                                                         dev)
    max_iter = int(max_iter)
    q, t = _lanczos_buffers(max_iter, v3)
    iters = C.c_int32(0)
    _launch("lo_lanczos_tridiag_f64", dev, A3, d2, cb, user, v3, B, N, P, max_iter, float(tol), q, t, C.byref(iters),
            ws_bytes=lib.lo_lanczos_f64_workspace_bytes(B, N, P, max_iter), errors=errors)
    del keep
    return _lanczos_out(q, t, iters.value, batch)


def _native_lanczos_layout(q_mat: torch.Tensor):
    """(P, B) if q_mat [P, *batch, N, k] is the permuted view `lanczos_tridiag` returns of a basis stored [k, B, N, P]
    (element (p, b, n, a) at ((a B + b) N + n) P + p from its first element), else None.  Size-1 dimensions carry no
    information (the callers unsqueeze / squeeze them)."""
    if q_mat.dim() < 3:
        return None
    N, k = q_mat.shape[-2:]
    lead = list(q_mat.shape[:-2])
    P = lead[0]
    B = 1
    for s in lead[1:]:
        B *= s
    want = [1]  # stride of the probe dimension
    acc = N * P
    batch_strides = []
    for s in reversed(lead[1:]):
        batch_strides.append(acc)
        acc *= s
    want += list(reversed(batch_strides)) + [P, B * N * P]
    for size, have, exp in zip(q_mat.shape, q_mat.stride(), want):
        if size > 1 and have != exp:
            return None
    return P, B


def root_from_lanczos(q_mat: torch.Tensor, evecs: torch.Tensor, evals: torch.Tensor, want_root: bool = True,
                      want_inverse: bool = False):
    """lo_root_from_lanczos_f32: the epilogue of RootDecomposition.forward (functions/_root_decomposition.py:73-85).
    q_mat [*lead, N, k], evecs [*lead, k, k], evals [*lead, k] -> (q V, q V o sqrt(evals) or None, q V / sqrt(evals)
    or None).  k > 32: the same three expressions with torch (as the reference)."""
    lib = _hip.load()
    lead = q_mat.shape[:-2]
    N, k = q_mat.shape[-2:]
    if k > 32 or not (q_mat.is_cuda and q_mat.dtype == torch.float32):
        qv = q_mat.matmul(evecs)
        s = evals.sqrt().unsqueeze(-2)
        return qv, (qv * s if want_root else None), (qv / s if want_inverse else None)
    _hip.require_hip(q_mat, evecs, evals)
    native = _native_lanczos_layout(q_mat)
    if native is not None:
        P, B = native
        dev = q_mat.device
        v4 = evecs.contiguous().reshape(P * B, k, k)
        e4 = evals.contiguous().reshape(P * B, k)
        qv = torch.empty(P * B, N, k, dtype=torch.float32, device=dev)
        root = torch.empty_like(qv) if want_root else None
        inv = torch.empty_like(qv) if want_inverse else None
        rc = lib.lo_root_from_lanczos_native_f32(_hip.ptr(q_mat), _hip.ptr(v4), _hip.ptr(e4), B, N, P, k, _hip.ptr(qv),
                                                 _hip.ptr(root), _hip.ptr(inv), _hip.stream_ptr(dev))
        if rc == 0:
            shp = (*lead, N, k)
            return qv.reshape(shp), (None if root is None else root.reshape(shp)), (None if inv is None else inv.reshape(shp))
        if rc != _hip.LO_ERR_UNSUPPORTED:
            _hip.check(rc, "lo_root_from_lanczos_native_f32")
    q3 = q_mat.contiguous().reshape(-1, N, k)
    PB = q3.shape[0]
    v3 = evecs.contiguous().reshape(PB, k, k)
    e3 = evals.contiguous().reshape(PB, k)
    dev = q_mat.device
    qv = torch.empty_like(q3)
    root = torch.empty_like(q3) if want_root else None
    inv = torch.empty_like(q3) if want_inverse else None
    _launch("lo_root_from_lanczos_f32", dev, q3, v3, e3, PB, N, k, qv, root, inv)
    shp = (*lead, N, k)
    return qv.reshape(shp), (None if root is None else root.reshape(shp)), (None if inv is None else inv.reshape(shp))


def _uv(left_vecs: torch.Tensor, right_vecs: torch.Tensor, batch_shape):
    """Broadcast left / right vectors [*b, N, D] to the operator's batch and flatten it."""
    if left_vecs.dim() == 1:
        left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
    bs = torch.broadcast_shapes(tuple(batch_shape), left_vecs.shape[:-2], right_vecs.shape[:-2])
    N, D = left_vecs.shape[-2:]
    U = left_vecs.expand(*bs, N, D).contiguous().reshape(-1, N, D)
    V = right_vecs.expand(*bs, N, D).contiguous().reshape(-1, N, D)
    _hip.require_hip(U, V, dtype=U.dtype if U.dtype == torch.float64 else torch.float32)
    return U, V, bs


def _is_f64(*ts):
    """fp64 operands of the backward contractions (the pull-backs of an fp64 linear_cg solve): plain library GEMMs /
    reductions on the device -- the hand-written contraction kernels are fp32."""
    return all(t.is_cuda and t.dtype == torch.float64 for t in ts)


def bilinear_dense(left_vecs: torch.Tensor, right_vecs: torch.Tensor, batch_shape=()):
    """lo_bilinear_dense_f32: U V^T [*batch, N, N] (dense_linear_operator.py:69-71)."""
    U, V, bs = _uv(left_vecs, right_vecs, batch_shape)
    B, N, D = U.shape
    if _is_f64(U, V):
        return torch.matmul(U, V.mT).reshape(*bs, N, N)
    out = torch.empty(B, N, N, dtype=torch.float32, device=U.device)
    _launch("lo_bilinear_dense_f32", U.device, U, V, B, N, D, out)
    return out.reshape(*bs, N, N)


def bilinear_diag(left_vecs: torch.Tensor, right_vecs: torch.Tensor, batch_shape=(), constant: bool = False):
    """lo_bilinear_diag_f32: sum_d U o V [*batch, N], or its sum over N as [*batch, 1] for a constant diagonal
    (diag_linear_operator.py:37-45, :337-344)."""
    U, V, bs = _uv(left_vecs, right_vecs, batch_shape)
    B, N, D = U.shape
    dev = U.device
    if _is_f64(U, V):
        rd = (U * V).sum(-1)
        return rd.sum(-1).reshape(*bs, 1) if constant else rd.reshape(*bs, N)
    out = torch.empty(B if constant else B * N, dtype=torch.float32, device=dev)
    ws = _hip.workspace(4 * B * N + 256, dev) if constant else None
    _launch("lo_bilinear_diag_f32", dev, U, V, B, N, D, 1 if constant else 0, out, ws, 0 if ws is None else ws.numel())
    return out.reshape(*bs, 1) if constant else out.reshape(*bs, N)


def bilinear_root(root: torch.Tensor, left_vecs: torch.Tensor, right_vecs: torch.Tensor, with_rowdot: bool = False):
    """lo_bilinear_root_f32: U (V^T C) + V (U^T C) [*batch, N, R] for K = C C^T (autograd of the two-GEMM matvec).
    `with_rowdot`: also return sum_d U o V [*batch, N] (the Diag derivative for the same factors) from the same pass."""
    lib = _hip.load()
    U, V, bs = _uv(left_vecs, right_vecs, root.shape[:-2])
    B, N, D = U.shape
    R = root.shape[-1]
    Cm = root.expand(*bs, N, R).contiguous().reshape(B, N, R)
    if _is_f64(U, V, Cm):
        out = U @ (V.mT @ Cm) + V @ (U.mT @ Cm)
        if with_rowdot:
            return out.reshape(*bs, N, R), (U * V).sum(-1).reshape(*bs, N)
        return out.reshape(*bs, N, R)
    _hip.require_hip(Cm)
    dev = U.device
    # the kernel keeps a D x R tile on chip (D R <= 2048): wider problems go in column chunks, the derivative is a sum
    # over the columns
    # (phase A: D R <= 2048; phase B: T1 | T2 padded to 32-column blocks + 32 staged rows of U, V in 64 KB of LDS)
    rp = (R + 31) // 32 * 32
    dmax = max(1, min(2048 // R, (16000 // (2 * rp + 64)) & ~1))
    out, rowdot = None, None
    for d0 in range(0, D, dmax):
        Uc, Vc = (U, V) if D <= dmax else (U[..., d0:d0 + dmax].contiguous(), V[..., d0:d0 + dmax].contiguous())
        Dc = Uc.shape[-1]
        o = torch.empty(B, N, R, dtype=torch.float32, device=dev)
        rd = torch.empty(B, N, dtype=torch.float32, device=dev) if with_rowdot else None
        _launch("lo_bilinear_root_f32", dev, Cm, Uc, Vc, B, N, R, Dc, o, rd,
                ws_bytes=lib.lo_bilinear_root_workspace_bytes(B, N, R, Dc))
        out = o if out is None else out.add_(o)
        if with_rowdot:
            rowdot = rd if rowdot is None else rowdot.add_(rd)
    if with_rowdot:
        return out.reshape(*bs, N, R), rowdot.reshape(*bs, N)
    return out.reshape(*bs, N, R)


def root_apply_add(U: torch.Tensor, T: torch.Tensor, out: torch.Tensor) -> bool:
    """lo_root_apply_add_f32: out [*batch, N, R] += U [*batch, N, D] @ T [*batch, D, R] in place, one pass over `out`
    (the N-sized product of the pull-back through the pivoted Cholesky of a root, functions/_pivoted_cholesky.py).
    Returns False -- nothing touched -- when the kernel does not take the operands (the caller runs the library product):
    not fp32 CUDA, `out` not contiguous or not the whole of its storage (a slice of somebody else's tensor), R not 8 / 16 /
    32, D > 32, more than 65535 members."""
    if not (out.is_cuda and out.dtype == torch.float32 and U.dtype == torch.float32 and T.dtype == torch.float32
            and out.is_contiguous() and out.storage_offset() == 0
            and out.untyped_storage().nbytes() == out.numel() * 4 and not out.requires_grad) \
            or os.environ.get("LO_NO_ROOT_APPLY_ADD"):
        return False
    *bs, N, R = out.shape
    D = U.shape[-1]
    B = 1
    for x in bs:
        B *= int(x)
    if R not in (8, 16, 32) or not 1 <= D <= 32 or not 1 <= B <= 65535 or tuple(U.shape) != (*bs, N, D) \
            or tuple(T.shape[-2:]) != (D, R):
        return False
    lib = _hip.load()
    _hip.require_hip(out)
    Uc = U.contiguous()
    Tc = T.expand(*bs, D, R).contiguous()
    _hip.check(lib.lo_root_apply_add_f32(_hip.ptr(Uc), _hip.ptr(Tc), B, N, D, R, _hip.ptr(out),
                                         _hip.stream_ptr(out.device)), "lo_root_apply_add_f32")
    return True


def bilinear_kron(K1: torch.Tensor, K2: torch.Tensor, left_vecs: torch.Tensor, right_vecs: torch.Tensor):
    """lo_bilinear_kron_f32: (dK1, dK2) of sum_d u_d^T (K1 (x) K2) v_d (autograd of the Kronecker matvec)."""
    lib = _hip.load()
    bs0 = torch.broadcast_shapes(K1.shape[:-2], K2.shape[:-2])
    U, V, bs = _uv(left_vecs, right_vecs, bs0)
    B, N, D = U.shape
    n1, n2 = K1.shape[-1], K2.shape[-1]
    assert n1 * n2 == N
    A1 = K1.expand(*bs, n1, n1).contiguous().reshape(B, n1, n1)
    A2 = K2.expand(*bs, n2, n2).contiguous().reshape(B, n2, n2)
    _hip.require_hip(A1, A2)
    dev = U.device
    d1 = torch.empty(B, n1, n1, dtype=torch.float32, device=dev)
    d2 = torch.empty(B, n2, n2, dtype=torch.float32, device=dev)
    _launch("lo_bilinear_kron_f32", dev, A1, A2, U, V, B, n1, n2, D, d1, d2,
            ws_bytes=lib.lo_bilinear_kron_workspace_bytes(B, n1, n2, D))
    return d1.reshape(*bs, n1, n1), d2.reshape(*bs, n2, n2)


# Which shapes `kron_eig_apply` hands to the fused kernel of lo_kron_eig_apply_f32, by (n2 class, one column / more
# columns): True only where tools/mb_sum_kron.py measured the fused launch at least as fast as the composition (the
# Kronecker matvec kernels on (M1, S2^T) and one scale pass).  A cell that is absent keeps the
# composition.  The n2 classes are the measured task-factor sizes; a size between two of them takes the next one above.
# Measured (fused / composition, microseconds; 1 column, 17 columns):
#   n2  4   1 x (4096 (x) 4)      35 /  595      533 /  696
#   n2  8   64 x (512 (x) 8)      78 /  116     1442 /  215   (17 columns stay with the composition)
#   n2 16   16 x (1024 (x) 16)   237 /  189     5025 /  338   (both stay with the composition)
_KRON_EIG_SIZES = (4, 8, 16)
_NATIVE_KRON_EIG: dict = {(4, 1): True, (4, 2): True, (8, 1): True}


def kron_eig_routed(n2: int, c: int) -> bool:
    """Whether the routing table sends (n2, c) to the fused kernel."""
    if n2 > _hip.LO_KRON_EIG_MAX_SMALL or c > _hip.LO_KRON_EIG_MAX_COLS:
        return False
    cell = next(s for s in _KRON_EIG_SIZES if n2 <= s)
    return bool(_NATIVE_KRON_EIG.get((cell, 1 if c == 1 else 2), False))


def kron_eig_apply(M1: torch.Tensor, S2: torch.Tensor, scale: Optional[torch.Tensor], z: torch.Tensor,
                   fused: Optional[bool] = None) -> Optional[torch.Tensor]:
    """y = scale o ((M1 (x) S2^T) z), lo_kron_eig_apply_f32: M1 [*batch, n1, n1], S2 [*batch, n2, n2], scale
    [*batch, n1 n2] or None, z [*batch, n1 n2, c] of batch shapes that broadcast.  Per column, with Z its [n1, n2] view,
    Y = scale o (M1 (Z S2)).  n2 <= LO_KRON_EIG_MAX_SMALL: `fused` True is the one-launch kernel, False the composition
    of the Kronecker matvec kernels with one scale pass, None what `kron_eig_routed` measured to be the faster of the
    two; larger n2 compose inside the entry point.  None when the library does not take the shape (LO_ERR_UNSUPPORTED)."""
    lib = _hip.load()
    if M1.dim() < 2 or S2.dim() < 2 or z.dim() < 2 or M1.shape[-1] != M1.shape[-2] or S2.shape[-1] != S2.shape[-2]:
        raise ValueError(f"kron_eig_apply: square factors and a matrix of columns expected, got {tuple(M1.shape)}, "
                         f"{tuple(S2.shape)}, {tuple(z.shape)}")
    n1, n2, (N, c) = M1.shape[-1], S2.shape[-1], z.shape[-2:]
    if n1 * n2 != N or (scale is not None and scale.shape[-1] != N):
        raise RuntimeError(f"kron_eig_apply: factors of {n1} and {n2} rows, scale "
                           f"{None if scale is None else tuple(scale.shape)} against {N} rows of z")
    _hip.require_hip(M1, S2, scale, z)
    bs = torch.broadcast_shapes(M1.shape[:-2], S2.shape[:-2], z.shape[:-2], *([] if scale is None else [scale.shape[:-1]]))
    if n2 <= _hip.LO_KRON_EIG_MAX_SMALL and not (kron_eig_routed(n2, c) if fused is None else fused):
        # the composition on the Kronecker matvec kernels (what the entry point runs for larger n2)
        desc = kron_diag_descriptor(M1.expand(*bs, n1, n1), S2.mT.expand(*bs, n2, n2), None)
        y = matvec(desc, z.expand(*bs, N, c))
        return y if scale is None else y.mul_(scale.unsqueeze(-1))
    A1, A2, z3 = _flat(M1.expand(*bs, n1, n1), 2), _flat(S2.expand(*bs, n2, n2), 2), _flat(z.expand(*bs, N, c), 2)
    sc = None if scale is None else _flat(scale.expand(*bs, N), 1)
    B = z3.shape[0]
    y = torch.empty_like(z3)
    if y.numel() == 0:
        return y.reshape(*bs, N, c)
    ws = _hip.workspace(lib.lo_kron_eig_apply_workspace_bytes(B, n1, n2, c), z.device)
    rc = lib.lo_kron_eig_apply_f32(_hip.ptr(A1), _hip.ptr(A2), _hip.ptr(sc), _hip.ptr(z3), _hip.ptr(y), B, n1, n2, c,
                                   _hip.ptr(ws), ws.numel(), _hip.stream_ptr(z.device))
    if rc == _hip.LO_ERR_UNSUPPORTED:
        return None
    _hip.check(rc, "lo_kron_eig_apply_f32")
    return y.reshape(*bs, N, c)


def set_onchip_cg(enable: bool):
    """Allow (default) or forbid the operator-resident CG fast path (csrc/lo_cg_onchip.hip); test / A-B switch.
    Enabling also ends a cool-down of the resident kernels (`resident_status`)."""
    _hip.load().lo_cg_set_onchip(1 if enable else 0)


def resident_status() -> dict:
    """lo_resident_status_get: the gate of the resident kernels -- hand-off timeouts seen by this process, calls still
    to be served by the streaming engines (cool-down), length of the next cool-down, re-arms so far."""
    out = _hip.ResidentStatus()
    _hip.call("lo_resident_status_get", C.byref(out))
    return {n: int(getattr(out, n)) for n, _ in _hip.ResidentStatus._fields_}


def inject_resident_timeouts(n: int):
    """lo_resident_inject_timeouts: the next n resident CG launches are treated as timed out (the solve is redone on
    the streaming engine and a cool-down starts) -- tests and `bench.py --inject-timeouts`."""
    _hip.call("lo_resident_inject_timeouts", int(n))


def resident_handoff_debug(force_clear: bool = False, next_tag: int = -1, next_epoch: int = -1) -> dict:
    """lo_resident_handoff_debug: the hand-off buffer the library owns for the headline solve (`k_cg_rspace3`) on the
    current device -- optionally make the next launch clear it first, or replace the tag / epoch counters (tests of the
    wrap-around); returns the counters and how many launches / clears the buffer has seen."""
    out = (C.c_uint32 * 4)()
    _hip.call("lo_resident_handoff_debug", 1 if force_clear else 0, int(next_tag), int(next_epoch), out)
    return {"next_tag": int(out[0]), "next_epoch": int(out[1]), "clears": int(out[2]), "launches": int(out[3])}


def resident_order_debug(mode: int = -1) -> dict:
    """lo_resident_order_debug: the order in which the headline solve (`k_cg_rspace3`) walks its members on the current
    device -- mode 0 automatic (opposite to a clean predecessor on the same operator), 1 always forward, 2 always
    reverse, -1 leave; returns the direction of the last launch and how many launches ran in reverse."""
    out = (C.c_uint32 * 2)()
    _hip.call("lo_resident_order_debug", int(mode), out)
    return {"last": "reverse" if out[0] else "forward", "reversed": int(out[1])}


RESIDENT_START_CAP_TICKS = 800  # (csrc/lo_rs3_start.h: no workgroup waits longer, 8 us of the 100 MHz clock)


def resident_start_debug(mode: int = -1, delta_ticks: int = 0) -> dict:
    """lo_resident_start_debug: the ordered start of the headline solve (`k_cg_rspace3`) on the current device -- mode 0
    automatic (the committed delay in launches of six rounds or more, in the layouts it was measured in), 1 never, 2
    the committed delay always, 3 `delta_ticks`, -1 leave; returns the mode in force and what the last launch used:
    its delta (0: no wait), its groups, and how many launches waited."""
    out = (C.c_uint32 * 4)()
    _hip.call("lo_resident_start_debug", int(mode), int(delta_ticks), out)
    return {"mode": int(out[0]), "delta": int(out[1]), "ngroups": int(out[2]), "waited": int(out[3])}


def resident_start_delay(mode: int, delta_ticks: int, B: int, ngroups: int, grp: int) -> int:
    """lo_resident_start_delay: the ticks group `grp` of a launch of B members in `ngroups` groups waits under
    (mode, delta_ticks) -- the rule of the ordered start, evaluated on the host (no device needed)."""
    return int(_hip.load().lo_resident_start_delay(int(mode), int(delta_ticks), int(B), int(ngroups), int(grp)))


def peer_gather_set(bufs=(), member_offset: int = 0) -> None:
    """lo_peer_gather_set (prototype): up to seven [B_total, N] fp32 buffers the resident single-column solve writes its
    solutions into next to its own output -- the gather of SURVEY 8(e) as peer writes.  () removes them."""
    n = len(bufs)
    arr = (C.c_void_p * max(n, 1))(*[b.data_ptr() for b in bufs])
    _hip.call("lo_peer_gather_set", arr, n, int(member_offset))


# ------------------------------------------- exact small-N path (csrc/lo_chol.hip, float64: csrc/lo_chol_f64.hip)
CHOLESKY_MAX_N = 1024  # what lo_cholesky_* / lo_tri_solve_* / lo_cholesky_solve_* take, _f32 and _f64 alike
_CHOL_SUFFIX = {torch.float32: "f32", torch.float64: "f64"}


def _chol_suffix(*tensors: torch.Tensor) -> str:
    """The entry-point suffix of the operands' common dtype, float32 or float64; mixed dtypes are an error."""
    dtype = tensors[0].dtype
    if dtype not in _CHOL_SUFFIX:
        raise ValueError(f"the exact path takes float32 or float64 tensors, got {dtype}")
    if any(t.dtype != dtype for t in tensors):
        raise ValueError(f"factor and right-hand side must share one dtype, got {[t.dtype for t in tensors]}")
    _hip.require_hip(*tensors, dtype=dtype)
    return _CHOL_SUFFIX[dtype]


def _factor_and_rhs(L: torch.Tensor, rhs: torch.Tensor):
    """A factor [*b, N, N] and right-hand sides [*b', N, c] (or [N]) of one dtype, broadcast to one batch and flattened;
    last the suffix of the entry points for that dtype."""
    if L.dim() < 2 or L.shape[-1] != L.shape[-2]:
        raise ValueError(f"expected square factors [..., N, N], got {tuple(L.shape)}")
    is_vec = rhs.dim() == 1
    cols = rhs.unsqueeze(-1) if is_vec else rhs
    N, c = L.shape[-1], cols.shape[-1]
    if cols.shape[-2] != N:
        raise ValueError(f"right-hand side of {cols.shape[-2]} rows against a factor of {N}")
    sfx = _chol_suffix(L, cols)
    bs = torch.broadcast_shapes(L.shape[:-2], cols.shape[:-2])
    L3 = _flat(L.expand(*bs, N, N), 2)
    R3 = _flat(cols.expand(*bs, N, c), 2)
    return L3, R3, bs, is_vec, sfx


def cholesky(A: torch.Tensor, want_logdet: bool = False):
    """lo_cholesky_f32 / lo_cholesky_f64 by dtype: (L, info[, logdet]) of A [*batch, N, N] = L L^T, N <= 1024; only the
    lower triangle of A is read, the strict upper triangle of L is zero, info [*batch] int32 is 0 or the 1-based order of
    the first leading minor whose pivot is not > 0 (that member's L is unspecified), logdet [*batch] float64 =
    2 sum log L_ii."""
    if A.dim() < 2 or A.shape[-1] != A.shape[-2]:
        raise ValueError(f"expected square matrices [..., N, N], got {tuple(A.shape)}")
    sfx = _chol_suffix(A)
    bs, N = A.shape[:-2], A.shape[-1]
    A3 = _flat(A, 2)
    B, dev = A3.shape[0], A.device
    L = torch.empty_like(A3)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    logdet = torch.empty(B, dtype=torch.float64, device=dev) if want_logdet else None
    if B > 0 and N > 0:
        sizer = "lo_cholesky_workspace_bytes" if sfx == "f32" else "lo_cholesky_f64_workspace_bytes"
        _launch(f"lo_cholesky_{sfx}", dev, A3, L, info, logdet, B, N, ws_bytes=getattr(_hip.load(), sizer)(B, N))
    out = (L.reshape(*bs, N, N), info.reshape(bs))
    return out + (logdet.reshape(bs),) if want_logdet else out


def triangular_solve(L: torch.Tensor, rhs: torch.Tensor, transpose: bool = False, want_sumsq: bool = False,
                     upper: bool = False):
    """lo_tri_solve_f32 / lo_tri_solve_f64 by dtype: L^-1 rhs, or L^-T rhs (`transpose`), for a lower (or `upper`) factor
    [*b, N, N], N <= 1024; with `want_sumsq` also sum_i out_ic^2 [*batch, c], of the operands' dtype, from the same
    launch (the inv_quad of a Cholesky factor)."""
    L3, R3, bs, is_vec, sfx = _factor_and_rhs(L, rhs)
    B, N, c = R3.shape
    out = torch.empty_like(R3)
    sumsq = torch.empty(B, c, dtype=R3.dtype, device=R3.device) if want_sumsq else None
    if out.numel():
        _launch(f"lo_tri_solve_{sfx}", R3.device, L3, R3, out, sumsq, B, N, c, int(bool(upper)), int(bool(transpose)))
    out = out.reshape(*bs, N) if is_vec else out.reshape(*bs, N, c)
    if not want_sumsq:
        return out
    return out, (sumsq.reshape(bs) if is_vec else sumsq.reshape(*bs, c))


def cholesky_solve(L: torch.Tensor, rhs: torch.Tensor, upper: bool = False) -> torch.Tensor:
    """lo_cholesky_solve_f32 / lo_cholesky_solve_f64 by dtype: (L L^T)^-1 rhs for a lower factor, (U^T U)^-1 rhs for an
    `upper` one, in one launch."""
    L3, R3, bs, is_vec, sfx = _factor_and_rhs(L, rhs)
    B, N, c = R3.shape
    out = torch.empty_like(R3)
    if out.numel():
        _launch(f"lo_cholesky_solve_{sfx}", R3.device, L3, R3, out, B, N, c, int(bool(upper)))
    return out.reshape(*bs, N) if is_vec else out.reshape(*bs, N, c)


# ------------------------------------------- symmetric eigendecomposition, float64 (csrc/lo_eigh_f64.hip)
EIGH_MAX_N = _hip.LO_EIGH_MAX_N  # what lo_eigh_f64 takes


def eigh(A: torch.Tensor, want_vectors: bool = True):
    """lo_eigh_f64: (evals [*batch, N] ascending, evecs [*batch, N, N] or None, info [*batch] int32) of the symmetric
    float64 matrices A [*batch, N, N], 1 <= N <= 1024; only the lower triangle of A is read.  Column j of evecs is the
    unit eigenvector of evals[j].  info is 0, or > 0 for a member whose input holds a non-finite value or whose iteration
    did not converge: that member's outputs are NaN.  Without vectors the eigenvalues are the same bits."""
    if A.dim() < 2 or A.shape[-1] != A.shape[-2]:
        raise ValueError(f"expected square matrices [..., N, N], got {tuple(A.shape)}")
    _hip.require_hip(A, dtype=torch.float64)
    bs, N = A.shape[:-2], A.shape[-1]
    A3 = _flat(A, 2)
    B, dev = A3.shape[0], A.device
    evals = torch.empty(B, N, dtype=torch.float64, device=dev)
    evecs = torch.empty_like(A3) if want_vectors else None
    info = torch.empty(B, dtype=torch.int32, device=dev)
    if B > 0 and N > 0:
        wv = int(bool(want_vectors))
        _launch("lo_eigh_f64", dev, A3, evals, evecs, info, B, N, wv,
                ws_bytes=_hip.load().lo_eigh_f64_workspace_bytes(B, N, wv))
    return evals.reshape(*bs, N), (evecs.reshape(*bs, N, N) if want_vectors else None), info.reshape(bs)
