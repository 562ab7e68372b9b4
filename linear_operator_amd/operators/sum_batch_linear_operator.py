"""SumBatchLinearOperator: the sum of the blocks of the base operator (reference:
operators/sum_batch_linear_operator.py:14-69); what `LinearOperator.sum(dim)` returns for a batch dimension.  The
product is the composition: one batched product of the base operator and a reduction of the [T, n, c] result.  The
in-place kernel (LO_BLOCK_SUM of csrc/lo_block.hip, kernels.block_matvec) measured slower at every shape tried
(DESIGN.md section 6e), so `_native_worthwhile` keeps its default and no product of this class is routed to it."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _hip
from .block_linear_operator import BlockLinearOperator


class SumBatchLinearOperator(BlockLinearOperator):
    _layout = _hip.LO_BLOCK_SUM

    def _add_batch_dim(self, other: Tensor) -> Tensor:
        return other.unsqueeze(-3).expand(*other.shape[:-2], self.num_blocks, *other.shape[-2:])

    def _remove_batch_dim(self, other: Tensor) -> Tensor:
        return other.sum(-3)

    def _diagonal(self) -> Tensor:
        return self.base_linear_op._diagonal().sum(-2)

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:
        sum_index = torch.arange(self.num_blocks, device=self.device).view(*([1] * row_index.dim()), -1)
        res = self.base_linear_op._get_indices(row_index.unsqueeze(-1), col_index.unsqueeze(-1),
                                               *(i.unsqueeze(-1) for i in batch_indices), sum_index)
        return res.sum(-1)

    def _getitem(self, row_index, col_index, *batch_indices):
        return self.__class__(self.base_linear_op._getitem(row_index, col_index, *batch_indices, slice(None, None, None)))

    def _size(self) -> torch.Size:
        shape = list(self.base_linear_op.shape)
        del shape[-3]
        return torch.Size(shape)

    def to_dense(self) -> Tensor:
        return self.base_linear_op.to_dense().sum(dim=-3)


__all__ = ["SumBatchLinearOperator"]
