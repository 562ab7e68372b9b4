"""ToeplitzLinearOperator: a (batch of) symmetric Toeplitz matrices stored as their first column
(reference: linear_operator/operators/toeplitz_linear_operator.py).

fp32 HIP columns lower to LO_OP_TOEPLITZ_DIAG (csrc/lo_ski.hip): `_matmul`, CG, Lanczos, MINRES and the pivoted
Cholesky run on a direct Toeplitz product from LDS that never forms the M x M matrix; the backward pass is the lag
correlation kernel.  Grids beyond LO_TOEPLITZ_MAX_M points, CPU and fp64 columns take the reference's torch.fft
composition (utils/toeplitz.py).
"""
from __future__ import annotations

import torch
from torch import Tensor

from ..utils.toeplitz import sym_toeplitz, sym_toeplitz_derivative_quadratic_form, sym_toeplitz_matmul
from ._linear_operator import LinearOperator


class ToeplitzLinearOperator(LinearOperator):
    def __init__(self, column):
        super().__init__(column)
        self.column = column

    def _kernel_descriptor(self, batch_shape=None):
        col = self.column
        if not (col.is_cuda and col.dtype == torch.float32):
            return None
        from .. import kernels as K

        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        return K.toeplitz_diag_descriptor(col.expand(*bs, col.size(-1)), None)

    def _diagonal(self) -> Tensor:  # reference :25-31
        diag_term = self.column[..., 0]
        if self.column.ndimension() > 1:
            diag_term = diag_term.unsqueeze(-1)
        return diag_term.expand(*self.column.size())

    def _expand_batch(self, batch_shape):  # :33-36
        return self.__class__(self.column.expand(*batch_shape, self.column.size(-1)))

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:  # :38-40
        toeplitz_indices = (row_index - col_index).fmod(self.size(-1)).abs().long()
        return self.column[(*batch_indices, toeplitz_indices)]

    def _matmul(self, rhs: Tensor) -> Tensor:  # :42-47
        return sym_toeplitz_matmul(self.column, rhs)

    def _t_matmul(self, rhs: Tensor) -> Tensor:  # :49-53 (the matrix is symmetric)
        return self._matmul(rhs)

    def _mul_constant(self, other):
        """c T for a scalar or a per-member constant [*batch] (what InterpolatedLinearOperator._mul_constant hands its
        base): the constant scales the whole column of its member."""
        if torch.is_tensor(other) and other.dim() > 0:
            other = other.unsqueeze(-1)
        return self.__class__(self.column * other)

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):  # :55-66
        if left_vecs.ndimension() == 1:
            left_vecs = left_vecs.unsqueeze(1)
            right_vecs = right_vecs.unsqueeze(1)
        res = sym_toeplitz_derivative_quadratic_form(left_vecs, right_vecs)
        # collapse any expanded broadcast dimensions back to the column's shape
        if tuple(res.shape) != tuple(self.column.shape):
            res = res.sum_to_size(*self.column.shape)
        return (res,)

    def _size(self) -> torch.Size:  # :68-69
        return torch.Size((*self.column.shape, self.column.size(-1)))

    def _transpose_nonbatch(self):  # :71-74
        return ToeplitzLinearOperator(self.column)

    def add_jitter(self, jitter_val: float = 1e-3):  # :76-81
        jitter = torch.zeros_like(self.column)
        jitter.narrow(-1, 0, 1).fill_(jitter_val)
        return ToeplitzLinearOperator(self.column.add(jitter))

    def to_dense(self) -> Tensor:
        if self.column.dim() == 1:
            return sym_toeplitz(self.column)
        M = self.column.size(-1)
        lag = torch.arange(M, device=self.column.device)
        lag = (lag.unsqueeze(-1) - lag.unsqueeze(0)).abs()
        return self.column[..., lag]


__all__ = ["ToeplitzLinearOperator"]
