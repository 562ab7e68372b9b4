"""Autograd Functions of the exact small-N path: the native batched Cholesky, triangular solve and Cholesky solve
(csrc/lo_chol.hip, float64: csrc/lo_chol_f64.hip, through kernels.cholesky / triangular_solve / cholesky_solve) with
their pull-backs, which run on the kernels of the same dtype.  The ATen calls
they replace (torch.linalg.cholesky_ex, torch.linalg.solve_triangular, torch.cholesky_solve) are differentiable, so
these are too.

`impl` holds the three kernel wrappers the Functions call.  It is a seam for exactly one purpose: a test substitutes
float64 torch implementations to run `torch.autograd.gradcheck` on the backward formulas without a device."""
from __future__ import annotations

import types

import torch
from torch.autograd.function import once_differentiable

from .. import kernels as K

impl = types.SimpleNamespace(cholesky=K.cholesky, triangular_solve=K.triangular_solve, cholesky_solve=K.cholesky_solve)


def _sum_to(grad: torch.Tensor, shape) -> torch.Tensor:
    return grad if tuple(grad.shape) == tuple(shape) else grad.sum_to_size(*shape)


class NativeCholesky(torch.autograd.Function):
    """(L, info) = cholesky_ex(A).  Backward: A_bar = sym(L^-T Phi(L^T L_bar) L^-1), Phi = lower triangle with the
    diagonal halved; the two N-column substitutions are native."""

    @staticmethod
    def forward(ctx, A):
        L, info = impl.cholesky(A)
        ctx.save_for_backward(L)
        ctx.mark_non_differentiable(info)
        return L, info

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_L, _grad_info):
        (L,) = ctx.saved_tensors
        P = torch.tril(L.mT @ grad_L)
        P.diagonal(dim1=-2, dim2=-1).mul_(0.5)
        Y = impl.triangular_solve(L, P, transpose=True)  # L^-T P
        S = impl.triangular_solve(L, Y.mT, transpose=True).mT  # (L^-T Y^T)^T = Y L^-1
        return 0.5 * (S + S.mT)


class NativeCholeskySolve(torch.autograd.Function):
    """x = (L L^T)^-1 rhs (lower factor) or (U^T U)^-1 rhs (upper).  Backward: g = the same solve of x_bar, rhs_bar = g,
    L_bar = -tril((g x^T + x g^T) L) (U_bar = -triu(U (g x^T + x g^T)))."""

    @staticmethod
    def forward(ctx, factor, rhs, upper):
        x = impl.cholesky_solve(factor, rhs, upper=upper)
        ctx.save_for_backward(factor, x)
        ctx.upper = upper
        ctx.shapes = (factor.shape, rhs.shape)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_x):
        factor, x = ctx.saved_tensors
        g = impl.cholesky_solve(factor, grad_x, upper=ctx.upper)
        grad_factor = None
        if ctx.needs_input_grad[0]:
            sym = g @ x.mT
            sym = sym + sym.mT
            grad_factor = -torch.triu(factor @ sym) if ctx.upper else -torch.tril(sym @ factor)
            grad_factor = _sum_to(grad_factor, ctx.shapes[0])
        return grad_factor, _sum_to(g, ctx.shapes[1]), None


class NativeTriSolve(torch.autograd.Function):
    """x = M^-1 rhs, M = T or T^T of a lower / upper factor T.  Backward: the same kernel with the flag flipped,
    g = M^-T x_bar = rhs_bar, M_bar = -g x^T restricted to the triangle of T."""

    @staticmethod
    def forward(ctx, factor, rhs, upper, transpose):
        x = impl.triangular_solve(factor, rhs, transpose=transpose, upper=upper)
        ctx.save_for_backward(factor, x)
        ctx.flags = (upper, transpose)
        ctx.shapes = (factor.shape, rhs.shape)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_x):
        factor, x = ctx.saved_tensors
        upper, transpose = ctx.flags
        g = impl.triangular_solve(factor, grad_x, transpose=not transpose, upper=upper)
        grad_factor = None
        if ctx.needs_input_grad[0]:
            gm = -(x @ g.mT) if transpose else -(g @ x.mT)
            grad_factor = _sum_to(torch.triu(gm) if upper else torch.tril(gm), ctx.shapes[0])
        return grad_factor, _sum_to(g, ctx.shapes[1]), None, None


# 1 x 800^2: the two sweeps take about 1040 us against about 500 us for ATen, the only single-matrix solve measured
SINGLE_SOLVE_MAX_N = 0
# float64, 1 x 800^2 (tools/mb_chol.py --dtype float64): factor + one-column solve takes about
# 4140 us with the native substitution against about 3360 us with ATen's, so ATen keeps the unbatched float64 solve
SINGLE_SOLVE_MAX_N_F64 = 0
_NATIVE_DTYPES = (torch.float32, torch.float64)


def native_ok(factor: torch.Tensor, *others: torch.Tensor, solve: bool = False) -> bool:
    """The routing predicate of the exact path: float32 or float64 HIP tensors, all of one dtype, with 1 <= N <= 1024
    go to the native kernels (csrc/lo_chol.hip, csrc/lo_chol_f64.hip), everything else (CPU, other or mixed dtypes,
    larger N) keeps the ATen calls.  `solve`: the call is a substitution, not a factorisation -- one workgroup per member
    and column block leaves a single matrix on a few compute units, and above SINGLE_SOLVE_MAX_N (float64:
    SINGLE_SOLVE_MAX_N_F64) rows ATen's whole-device substitution is faster (measured, DESIGN sections 6d and 6d-64),
    so an unbatched solve of that size stays there.  Batched calls are always native: they win at every measured
    shape, and they include the shapes at which the ATen routines fault."""
    if not (factor.is_cuda and factor.dtype in _NATIVE_DTYPES and factor.dim() >= 2
            and 1 <= factor.shape[-1] <= K.CHOLESKY_MAX_N and factor.shape[-1] == factor.shape[-2]
            and all(o.is_cuda and o.dtype == factor.dtype for o in others)):
        return False
    single_max = SINGLE_SOLVE_MAX_N if factor.dtype == torch.float32 else SINGLE_SOLVE_MAX_N_F64
    if solve and factor.shape[-1] > single_max:
        batch = torch.broadcast_shapes(factor.shape[:-2], *(o.shape[:-2] for o in others if o.dim() >= 2))
        return batch.numel() > 1
    return True


def _cols(rhs):
    return (rhs.unsqueeze(-1), True) if rhs.dim() == 1 else (rhs, False)


def tri_solve(factor, rhs, upper=False, transpose=False):
    """NativeTriSolve on matrix or vector right-hand sides."""
    cols, is_vec = _cols(rhs)
    x = NativeTriSolve.apply(factor, cols, bool(upper), bool(transpose))
    return x.squeeze(-1) if is_vec else x


def chol_solve(factor, rhs, upper=False):
    """NativeCholeskySolve on matrix or vector right-hand sides."""
    cols, is_vec = _cols(rhs)
    x = NativeCholeskySolve.apply(factor, cols, bool(upper))
    return x.squeeze(-1) if is_vec else x


def substitute(factor, rhs, upper=False, transpose=False):
    """M^-1 rhs for M = factor or factor^T (`transpose`) of a lower / upper triangular tensor: the native kernel for
    float32 or float64 HIP factors of at most 1024 rows, torch.linalg.solve_triangular otherwise.  A transposed view of a
    contiguous factor is handed over as that factor with both flags flipped, never copied."""
    if native_ok(factor, rhs, solve=True):
        if not factor.is_contiguous() and factor.mT.is_contiguous():
            factor, upper, transpose = factor.mT, not upper, not transpose
        return tri_solve(factor, rhs, upper=upper, transpose=transpose)
    cols, is_vec = _cols(rhs)
    x = torch.linalg.solve_triangular(factor.mT if transpose else factor, cols, upper=bool(upper) != bool(transpose))
    return x.squeeze(-1) if is_vec else x


__all__ = ["substitute", "NativeCholesky", "NativeCholeskySolve", "NativeTriSolve", "native_ok", "tri_solve", "chol_solve", "impl"]
