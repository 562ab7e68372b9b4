"""BlockInterleavedLinearOperator: the blocks of the base operator on the diagonal with the rows interleaved, row
i * T + t for row i of block t (reference: operators/block_interleaved_linear_operator.py:15-153): the covariance of
independent multi-output models in the (point, task) order.  The native product (csrc/lo_block.hip) reads the vectors
in that order and is taken for dense blocks and one column; the composition transposes the vectors into the base's
batch and back."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _hip
from .block_linear_operator import _BlockDiagonalBase


class BlockInterleavedLinearOperator(_BlockDiagonalBase):
    _layout = _hip.LO_BLOCK_INTERLEAVED

    def _add_batch_dim(self, other: Tensor) -> Tensor:
        *batch, rows, cols = other.shape
        return other.reshape(*batch, rows // self.num_blocks, self.num_blocks, cols).transpose(-2, -3).contiguous()

    def _remove_batch_dim(self, other: Tensor) -> Tensor:
        other = other.transpose(-2, -3).contiguous()
        *batch, rows, t, cols = other.shape
        return other.reshape(*batch, rows * t, cols)

    def _block_root(self, root):
        return BlockInterleavedLinearOperator(root)

    def _native_worthwhile(self, desc, cols: int) -> bool:
        # measured: dense blocks with one column, the product of every CG iteration of
        # AddedDiag(BlockInterleaved, Diag), are faster in place; more columns and low-rank blocks are not
        return desc.kind == _hip.LO_OP_DENSE_DIAG and cols == 1

    def _diagonal(self) -> Tensor:
        block_diag = self.base_linear_op._diagonal()
        return block_diag.mT.reshape(*block_diag.shape[:-2], -1)

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:
        t = self.num_blocks
        row_block, col_block = row_index.fmod(t), col_index.fmod(t)
        res = self.base_linear_op._get_indices(torch.div(row_index, t, rounding_mode="floor"),
                                               torch.div(col_index, t, rounding_mode="floor"), *batch_indices, row_block)
        return res * torch.eq(row_block, col_block).type_as(res)

    def to_dense(self) -> Tensor:
        dense = self.base_linear_op.to_dense()  # [*, T, n, m] -> [*, n, T, m, T]
        *batch, t, n, m = dense.shape
        return torch.diag_embed(dense.movedim(-3, -1)).permute(*range(len(batch)), -4, -2, -3, -1).reshape(
            *batch, n * t, m * t)


__all__ = ["BlockInterleavedLinearOperator"]
