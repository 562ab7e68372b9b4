"""SumBatchLinearOperator: the sum of the blocks of the base operator (reference:
operators/sum_batch_linear_operator.py:14-69); what `LinearOperator.sum(dim)` returns for a batch dimension.  The
product is the composition: one batched product of the base operator and a reduction of the [T, n, c] result.  The
in-place kernel (LO_BLOCK_SUM of csrc/lo_block.hip, kernels.block_matvec) measured slower at every shape tried
(DESIGN.md section 6e), so `_native_worthwhile` keeps its default and no product of this class is routed to it.

The additive SKI model -- a square InterpolatedLinearOperator over a ToeplitzLinearOperator as the base, one 1-D grid
per summed member -- lowers to LO_OP_SKI_SUM_DIAG (csrc/lo_ski_sum.hip): CG, Lanczos, MINRES and
the pivoted Cholesky then run on the descriptor, with no Python call per product or per pivot.  `_matmul` itself takes
the kind only in the cells of `kernels.NATIVE_MATMUL_SKI_SUM` (the routing table measured in section 6s)."""
from __future__ import annotations

import torch
from torch import Tensor

from .. import _hip
from .block_linear_operator import BlockLinearOperator
from .interpolated_linear_operator import InterpolatedLinearOperator
from .toeplitz_linear_operator import ToeplitzLinearOperator


class SumBatchLinearOperator(BlockLinearOperator):
    _layout = _hip.LO_BLOCK_SUM

    def _kernel_descriptor(self, batch_shape=None):
        """LO_OP_SKI_SUM_DIAG for a square InterpolatedLinearOperator over a ToeplitzLinearOperator (fp32 device
        tensors, equal left / right index shapes, M and the number of summed members within the kind's limits);
        else None.  The base's tensors over (*batch, P) are the kind's arrays as they are."""
        base = self.base_linear_op
        if not (isinstance(base, InterpolatedLinearOperator) and isinstance(base.base_linear_op, ToeplitzLinearOperator)):
            return None
        col = base.base_linear_op.column
        li, lv, ri, rv = (base.left_interp_indices, base.left_interp_values, base.right_interp_indices,
                          base.right_interp_values)
        if not all(t.is_cuda and t.dtype == torch.float32 for t in (col, lv, rv)) or not (li.is_cuda and ri.is_cuda):
            return None
        if li.shape[-2:] != ri.shape[-2:] or base.size(-1) != base.size(-2):
            return None
        from .. import kernels as K

        P, M = self.num_blocks, col.size(-1)
        if M > _hip.LO_TOEPLITZ_MAX_M or P > _hip.LO_SKI_SUM_MAX_TERMS:
            return None
        bs = torch.Size((*(self.batch_shape if batch_shape is None else batch_shape), P))
        N, J = li.shape[-2:]
        shared = li is ri and lv is rv
        ex = lambda t: t.expand(*bs, N, J)  # noqa: E731
        li_e, lv_e = ex(li), ex(lv)
        ri_e, rv_e = (li_e, lv_e) if shared else (ex(ri), ex(rv))
        desc = K.ski_sum_diag_descriptor(col.expand(*bs, M), li_e, lv_e, ri_e, rv_e, None)
        if desc is not None:  # the grid-major copy of W_r over the B P members, kept across calls (memo on the indices)
            desc.interp_plan = K.interp_plan(ri, bs, M)
        return desc

    def _matmul(self, rhs: Tensor) -> Tensor:
        from .. import kernels as K

        if (rhs.dim() >= 2 and rhs.is_cuda and rhs.dtype == torch.float32
                and K.NATIVE_MATMUL_SKI_SUM.get(1 if rhs.shape[-1] == 1 else 2, False)):
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
            if desc is not None:
                return K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
        return super()._matmul(rhs)

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
