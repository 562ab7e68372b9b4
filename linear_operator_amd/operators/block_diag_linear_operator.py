"""BlockDiagLinearOperator: the blocks of the base operator on the diagonal, row t * n + i for row i of block t
(reference: operators/block_diag_linear_operator.py:37-230).  In memory the vectors of this order ARE the base's batch,
so every method is the base operator's batched method on a reshaped view."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _hip
from .block_linear_operator import _BlockDiagonalBase
from .dense_linear_operator import DenseLinearOperator
from .diag_linear_operator import DiagLinearOperator


class BlockDiagLinearOperator(_BlockDiagonalBase):
    _layout = _hip.LO_BLOCK_DIAG
    _square_blocks = True

    def __new__(cls, base_linear_op=None, block_dim: int = -3):
        # a block diagonal of diagonal blocks is a diagonal matrix (reference :20-34)
        if cls is BlockDiagLinearOperator and isinstance(base_linear_op, DiagLinearOperator):
            if block_dim != -3:
                raise NotImplementedError(
                    "Passing a base_linear_op of type DiagLinearOperator to the constructor of "
                    f"BlockDiagLinearOperator with block_dim = {block_dim} != -3 is not supported."
                )
            return DiagLinearOperator(base_linear_op._diag.flatten(-2, -1))
        return super().__new__(cls)

    def __init__(self, base_linear_op, block_dim: int = -3):
        if isinstance(base_linear_op, Tensor):
            base_linear_op = DenseLinearOperator(base_linear_op)
        super().__init__(base_linear_op, block_dim)
        if self._square_blocks and self.base_linear_op.shape[-1] != self.base_linear_op.shape[-2]:
            raise RuntimeError(
                "base_linear_op must be a batch of square matrices, but non-batch dimensions are "
                f"{base_linear_op.shape[-2:]}"
            )

    def _add_batch_dim(self, other: Tensor) -> Tensor:
        *batch, rows, cols = other.shape
        return other.reshape(*batch, self.num_blocks, rows // self.num_blocks, cols)

    def _remove_batch_dim(self, other: Tensor) -> Tensor:
        *batch, t, rows, cols = other.shape
        return other.reshape(*batch, t * rows, cols)

    def _block_root(self, root):
        return _BlockDiagOfRoots(root)

    def _native_worthwhile(self, desc, cols: int) -> bool:
        return True  # (in this row order the call IS the base's batched product on a view: nothing is copied either way)

    def _diagonal(self) -> Tensor:
        return self.base_linear_op._diagonal().reshape(*self.batch_shape, self.size(-1))

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:
        n, m = self.base_linear_op.shape[-2:]
        row_block = torch.div(row_index, n, rounding_mode="floor")
        col_block = torch.div(col_index, m, rounding_mode="floor")
        res = self.base_linear_op._get_indices(row_index.fmod(n), col_index.fmod(m), *batch_indices, row_block)
        return res * torch.eq(row_block, col_block).type_as(res)  # (entries off the diagonal blocks are zero)

    def to_dense(self) -> Tensor:
        dense = self.base_linear_op.to_dense()  # [*, T, n, m] -> [*, T, n, T, m]
        *batch, t, n, m = dense.shape
        return torch.diag_embed(dense.movedim(-3, -1)).permute(*range(len(batch)), -2, -4, -1, -3).reshape(
            *batch, t * n, t * m)

    def matmul(self, other):
        if isinstance(other, BlockDiagLinearOperator) and self.base_linear_op.shape == other.base_linear_op.shape:
            return BlockDiagLinearOperator(self.base_linear_op.to_dense() @ other.base_linear_op.to_dense())
        if isinstance(other, DiagLinearOperator):
            diag = other._diag.reshape(*self.base_linear_op.shape[:-2], 1, self.base_linear_op.shape[-1])
            return BlockDiagLinearOperator(self.base_linear_op.to_dense() * diag)
        return super().matmul(other)


class _BlockDiagOfRoots(BlockDiagLinearOperator):
    """The block diagonal of the (n x k) roots of the blocks: R with R R^T the block diagonal operator."""
    _square_blocks = False


__all__ = ["BlockDiagLinearOperator"]
