"""CholLinearOperator: a positive definite matrix held as its Cholesky factor, L L^T for a lower factor and U^T U for
an upper one (reference: linear_operator/operators/chol_linear_operator.py:18-189; GPyTorch constructs it and tests
`isinstance` against it).  A RootLinearOperator whose root is a TriangularLinearOperator: solves are the two
substitutions of that root, the quadratic form is one substitution and a column sum of squares, the log-determinant
comes off the stored diagonal.  With a float32 or float64 HIP factor of at most 1024 rows all of these are the
native kernels of csrc/lo_chol.hip and csrc/lo_chol_f64.hip; CPU factors take ATen."""
from __future__ import annotations

import warnings

import torch
from torch import Tensor

from .. import kernels as K
from ._linear_operator import LinearOperator
from .root_linear_operator import RootLinearOperator
from .triangular_linear_operator import TriangularLinearOperator, _routed, _TriangularLinearOperatorBase


class CholLinearOperator(RootLinearOperator):
    def __init__(self, chol, upper: bool = False):
        if not isinstance(chol, _TriangularLinearOperatorBase):
            warnings.warn("chol argument to CholLinearOperator should be a TriangularLinearOperator. "
                          "Passing a dense tensor will cause errors in future versions.", DeprecationWarning)
            if bool(torch.all(torch.tril(chol) == chol)):
                chol = TriangularLinearOperator(chol, upper=False)
            elif bool(torch.all(torch.triu(chol) == chol)):
                chol = TriangularLinearOperator(chol, upper=True)
            else:
                raise ValueError("chol must be either lower or upper triangular")
        LinearOperator.__init__(self, chol, upper=upper)  # (`upper` travels with the representation tree)
        self.root = chol
        self.upper = bool(upper)

    @property
    def _chol_diag(self) -> Tensor:
        return self.root._diagonal()

    def _cholesky(self, upper: bool = False):
        return self.root if bool(upper) == self.upper else self.root._transpose_nonbatch()

    def cholesky(self, upper: bool = False):
        return self._cholesky(upper=upper)

    def _kernel_descriptor(self, batch_shape=None):
        return None  # the root is triangular, not a skinny dense factor: products go through the root

    def _matmul(self, rhs: Tensor) -> Tensor:
        if self.upper:
            return self.root._t_matmul(self.root._matmul(rhs))
        return self.root._matmul(self.root._t_matmul(rhs))

    def _diagonal(self) -> Tensor:
        return (self.root.to_dense() ** 2).sum(-2 if self.upper else -1)

    def _expand_batch(self, batch_shape):
        if len(batch_shape) == 0:
            return self
        return CholLinearOperator(self.root._expand_batch(batch_shape), upper=self.upper)

    def _solve(self, rhs: Tensor, preconditioner=None, num_tridiag: int = 0):
        if num_tridiag:
            return super()._solve(rhs, preconditioner, num_tridiag=num_tridiag)
        return self.root._cholesky_solve(rhs, upper=self.upper)

    def to_dense(self) -> Tensor:
        r = self.root.to_dense()
        return r.mT @ r if self.upper else r @ r.mT

    def inverse(self) -> "CholLinearOperator":
        """(L L^T)^-1 = (L^-1)^T L^-1: the inverse factor has the other orientation (reference :97-105)."""
        return CholLinearOperator(TriangularLinearOperator(self.root.inverse(), upper=not self.upper),
                                  upper=not self.upper)

    def inv_quad(self, inv_quad_rhs: Tensor, reduce_inv_quad: bool = True) -> Tensor:
        """sum_i (F^-1 r)_i^2 per column with F the lower-oriented factor: on the device one substitution launch that
        also returns the sums of squares."""
        t = self.root.to_dense()
        needs_grad = torch.is_grad_enabled() and (t.requires_grad or inv_quad_rhs.requires_grad)
        if not needs_grad and _routed().native_ok(t, inv_quad_rhs, solve=True):
            # lower L: L^-1 r; upper U (A = U^T U): U^-T r
            if not t.is_contiguous() and t.mT.is_contiguous():
                _, term = K.triangular_solve(t.mT, inv_quad_rhs, transpose=not self.upper, want_sumsq=True,
                                             upper=not self.root.upper)
            else:
                _, term = K.triangular_solve(t, inv_quad_rhs, transpose=self.upper, want_sumsq=True,
                                             upper=self.root.upper)
        else:
            half = (self.root._transpose_nonbatch() if self.upper else self.root).solve(inv_quad_rhs)
            term = (half ** 2).sum(-2) if inv_quad_rhs.dim() > 1 else (half ** 2).sum(-1)
        if inv_quad_rhs.dim() > 1 and term.numel() and reduce_inv_quad:
            term = term.sum(-1)
        return term

    def inv_quad_logdet(self, inv_quad_rhs=None, logdet=False, reduce_inv_quad=True):
        if not self.is_square:
            raise RuntimeError(
                "inv_quad_logdet only operates on (batches of) square (positive semi-definite) LinearOperators. "
                "Got a {} of size {}.".format(self.__class__.__name__, self.size()))
        if inv_quad_rhs is not None:
            if self.dim() == 2 and inv_quad_rhs.dim() == 1:
                if self.shape[-1] != inv_quad_rhs.numel():
                    raise RuntimeError("LinearOperator (size={}) cannot be multiplied with right-hand-side Tensor "
                                       "(size={}).".format(self.shape, inv_quad_rhs.shape))
            elif self.dim() != inv_quad_rhs.dim():
                raise RuntimeError("LinearOperator (size={}) and right-hand-side Tensor (size={}) should have the same "
                                   "number of dimensions.".format(self.shape, inv_quad_rhs.shape))
            elif self.shape[-1] != inv_quad_rhs.shape[-2]:
                raise RuntimeError("LinearOperator (size={}) cannot be multiplied with right-hand-side Tensor "
                                   "(size={}).".format(self.shape, inv_quad_rhs.shape))
        inv_quad_term = None if inv_quad_rhs is None else self.inv_quad(inv_quad_rhs, reduce_inv_quad=reduce_inv_quad)
        logdet_term = self._chol_diag.pow(2).log().sum(-1) if logdet else None
        return inv_quad_term, logdet_term

    def logdet(self) -> Tensor:
        return self._chol_diag.pow(2).log().sum(-1)

    def root_decomposition(self, method=None):
        return RootLinearOperator(self.root._transpose_nonbatch() if self.upper else self.root)

    def root_inv_decomposition(self, initial_vectors=None, test_vectors=None, method=None):
        """R with R R^T = A^-1: L^-T for a lower factor, U^-1 for an upper one."""
        inv = self.root.inverse()
        return RootLinearOperator(inv if self.upper else inv._transpose_nonbatch())

    def solve(self, right_tensor: Tensor, left_tensor=None) -> Tensor:
        is_vec = right_tensor.dim() == 1
        cols = right_tensor.unsqueeze(-1) if is_vec else right_tensor
        res = self.root._cholesky_solve(cols, upper=self.upper)
        if is_vec:
            res = res.squeeze(-1)
        return res if left_tensor is None else left_tensor @ res


__all__ = ["CholLinearOperator"]
