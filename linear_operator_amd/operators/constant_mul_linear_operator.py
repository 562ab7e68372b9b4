"""ConstantMulLinearOperator c A (reference: operators/constant_mul_linear_operator.py:14-185), what `A.mul(c)`
returns for an operator without a `_mul_constant` of its own (GPyTorch's ScaleKernel: `orig_output.mul(outputscale)`).

`_kernel_descriptor` folds the constant into the smallest tensor of the base's descriptor, so the device engines see a
kind they already run: Kronecker c K1, Root / LowRank sqrt(c) C (N R floats), Hadamard sqrt(c) F, Dense c K.  The dense
fold is one extra pass over the N^2 matrix per descriptor build (every `_matmul` / solve lowers afresh).  Any other
base lowers to None (closure path).  The fold is made of ordinary torch ops on the representation tensors, so a graph
built through it still reaches `c`.
"""
from __future__ import annotations

import dataclasses

import torch
from torch import Tensor

from ._linear_operator import LinearOperator
from .root_linear_operator import RootLinearOperator


class ConstantMulLinearOperator(LinearOperator):
    """c A for a scalar constant or one constant per batch member (`constant` of shape [] or [*batch])."""

    def __init__(self, base_linear_op, constant):
        if not torch.is_tensor(constant):
            constant = torch.tensor(constant, device=base_linear_op.device, dtype=base_linear_op.dtype)
        super().__init__(base_linear_op, constant)
        self.base_linear_op = base_linear_op
        self._constant = constant

    @property
    def expanded_constant(self) -> Tensor:
        """The constant as [*c, 1, 1], ready to scale [*batch, N, k] blocks."""
        c = self._constant
        if c.dim() > len(self.base_linear_op.batch_shape):
            raise RuntimeError(
                "ConstantMulLinearOperator of size {} received an invalid constant of size {}.".format(
                    self.base_linear_op.shape, c.shape
                )
            )
        return c[..., None, None]

    def _kernel_descriptor(self, batch_shape=None):
        from .. import kernels as K

        c = self._constant
        if not (c.is_cuda and c.dtype in (torch.float32, torch.float64)) or self.size(-1) != self.size(-2):
            return None
        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        desc = self.base_linear_op._kernel_descriptor(bs)
        if desc is None or desc.diag_mode != K._hip.LO_DIAG_NONE or desc.dtype != c.dtype:
            return None
        scale = c.expand(bs).reshape(-1, 1, 1) if c.dim() else c  # one factor per flattened member
        if desc.kind in (K._hip.LO_OP_LOWRANK_DIAG, K._hip.LO_OP_HADAMARD_DIAG):
            if not bool((c >= 0).all()):  # (a root cannot carry a negative scale)
                return None
            scale = scale.sqrt()
        elif desc.kind not in (K._hip.LO_OP_KRON_DIAG, K._hip.LO_OP_DENSE_DIAG):
            return None
        return dataclasses.replace(desc, A0=(desc.A0 * scale).contiguous())

    def _approx_diagonal(self) -> Tensor:
        return self.base_linear_op._approx_diagonal() * self._constant[..., None]

    def _diagonal(self) -> Tensor:
        return self.base_linear_op._diagonal() * self._constant[..., None]

    def _expand_batch(self, batch_shape):
        c = self._constant.expand(*batch_shape) if len(batch_shape) else self._constant
        return type(self)(self.base_linear_op._expand_batch(batch_shape), c)

    def _permute_batch(self, *dims: int):  # (the constant holds batch dimensions only, and perhaps not all of them)
        c = self._constant.expand(self.batch_shape).permute(*dims) if self._constant.dim() else self._constant
        return type(self)(self.base_linear_op._permute_batch(*dims), c)

    def _unsqueeze_batch(self, dim: int):
        c = self._constant.expand(self.batch_shape).unsqueeze(dim) if self._constant.dim() else self._constant
        return type(self)(self.base_linear_op._unsqueeze_batch(dim), c)

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:
        per_member = self._constant.expand(self.batch_shape)[batch_indices]
        return self.base_linear_op._get_indices(row_index, col_index, *batch_indices) * per_member

    def _matmul(self, rhs: Tensor) -> Tensor:
        from .. import kernels as K

        if K.native_matmul_candidate(self, rhs):
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
            if K.native_matmul(desc, rhs):
                return K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
        return self.expanded_constant * self.base_linear_op._matmul(rhs)

    def _t_matmul(self, rhs: Tensor) -> Tensor:
        return self.expanded_constant * self.base_linear_op._t_matmul(rhs)

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """d/dc of sum_s u_s^T (c A) v_s is sum_s u_s^T A v_s, per member, summed down to the constant's shape; the base
        tensors get the base's derivatives for the left vectors scaled by c."""
        quad = (left_vecs * self.base_linear_op._matmul(right_vecs)).sum((-2, -1))
        c = self._constant
        grad_c = quad.sum() if c.dim() == 0 else quad.sum_to_size(c.shape)
        base_grads = self.base_linear_op._bilinear_derivative(left_vecs * self.expanded_constant, right_vecs)
        return (*base_grads, grad_c)

    def _size(self) -> torch.Size:
        return self.base_linear_op.size()

    def _transpose_nonbatch(self):
        return type(self)(self.base_linear_op._transpose_nonbatch(), self._constant)

    def to_dense(self) -> Tensor:
        return self.expanded_constant * self.base_linear_op.to_dense()

    def root_decomposition(self, method=None):
        """Root(sqrt(c) R) for a non-negative constant (R the base's root); otherwise the generic decomposition."""
        if not bool((self._constant >= 0).all()):
            return super().root_decomposition(method=method)
        base_root = self.base_linear_op.root_decomposition(method=method).root
        return RootLinearOperator(ConstantMulLinearOperator(base_root, self._constant.sqrt()))


__all__ = ["ConstantMulLinearOperator"]
