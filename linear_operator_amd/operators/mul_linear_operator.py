"""MulLinearOperator: the elementwise (Hadamard) product of two symmetric operators, kept as the product of their root
decompositions, K = (F F^T) o (G G^T).  `A.mul(B)` of two structured operators and SKIP's `prod` over a batch of
KISS-GP operators build it (the reference's operators/mul_linear_operator.py, same constructor and results).

With two dense fp32 device roots of rank <= LO_HADAMARD_MAX_RANK the operator lowers to LO_OP_HADAMARD_DIAG
(csrc/lo_hadamard.hip): the matvec is y_t = rowdot(F, G M_t^T) with M_t = F^T diag(v_t) G on the matrix cores, and the
derivative with respect to both roots is one native call.  CPU, fp64, larger ranks and roots that are not dense use
the torch composition below:  K v = sum_r f_r o (G G^T (f_r o v)), with f_r the columns of F.
"""
from __future__ import annotations

import torch
from torch import Tensor

from ._linear_operator import LinearOperator
from .dense_linear_operator import DenseLinearOperator
from .root_linear_operator import RootLinearOperator, _root_pullback


def _rowwise_outer(a: Tensor, b: Tensor) -> Tensor:
    """[*, n, s] x [*, n, r] -> [*, n, s r]: row n holds a[n, i] b[n, j] at i r + j."""
    return (a.unsqueeze(-1) * b.unsqueeze(-2)).flatten(-2)


def _dense_root_tensor(root_op: RootLinearOperator):
    """The root of `root_op` as one tensor when it is dense or a constant times a dense one, else None."""
    from .constant_mul_linear_operator import ConstantMulLinearOperator

    r = root_op.root
    if isinstance(r, DenseLinearOperator):
        return r.tensor
    if isinstance(r, ConstantMulLinearOperator) and isinstance(r.base_linear_op, DenseLinearOperator):
        return r.to_dense()
    return None


class MulLinearOperator(LinearOperator):
    def _check_args(self, left_linear_op, right_linear_op):
        if not (isinstance(left_linear_op, LinearOperator) and isinstance(right_linear_op, LinearOperator)):
            return "MulLinearOperator expects two LinearOperators."
        if left_linear_op.shape != right_linear_op.shape:
            return "MulLinearOperator expects two LinearOperators of the same size: got {} and {}.".format(
                left_linear_op, right_linear_op
            )

    def __init__(self, left_linear_op, right_linear_op):
        # the side with the larger root decomposition goes left; both sides are held as roots
        if right_linear_op._root_decomposition_size() > left_linear_op._root_decomposition_size():
            left_linear_op, right_linear_op = right_linear_op, left_linear_op
        left, right = (op if isinstance(op, RootLinearOperator) else op.root_decomposition()
                       for op in (left_linear_op, right_linear_op))
        super().__init__(left, right)
        self.left_linear_op = left
        self.right_linear_op = right

    # ------------------------------------------------------------------ native lowering
    def _roots(self):
        """(F, G) when both are fp32 device tensors the native kernels take, else None."""
        from .. import kernels as K

        F = _dense_root_tensor(self.left_linear_op)
        G = _dense_root_tensor(self.right_linear_op)
        if F is None or G is None or not (F.is_cuda and G.is_cuda):
            return None
        if F.dtype != torch.float32 or G.dtype != torch.float32:
            return None
        if max(F.shape[-1], G.shape[-1]) > K._hip.LO_HADAMARD_MAX_RANK:
            return None
        return F, G

    def _kernel_descriptor(self, batch_shape=None):
        from .. import kernels as K

        roots = self._roots()
        if roots is None:
            return None
        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        F, G = (r.expand(*bs, *r.shape[-2:]) for r in roots)
        return K.hadamard_diag_descriptor(F, G, None)

    # ------------------------------------------------------------------ operator protocol
    def _diagonal(self) -> Tensor:  # rowsum(F^2) o rowsum(G^2)
        return self.left_linear_op._diagonal() * self.right_linear_op._diagonal()

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:
        return (self.left_linear_op._get_indices(row_index, col_index, *batch_indices)
                * self.right_linear_op._get_indices(row_index, col_index, *batch_indices))

    def _matmul(self, rhs: Tensor) -> Tensor:
        if rhs.dim() >= 2 and rhs.is_cuda and rhs.dtype == torch.float32:
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
            if desc is not None:
                from .. import kernels as K

                return K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
        return self._matmul_composition(rhs)

    def _matmul_composition(self, rhs: Tensor) -> Tensor:
        """K v = sum_r f_r o (G G^T (f_r o v)): one product of the right operator with p t columns."""
        vec = rhs.dim() == 1
        v = rhs.unsqueeze(-1) if vec else rhs
        F = self.left_linear_op.root.to_dense()
        bs = torch.broadcast_shapes(F.shape[:-2], v.shape[:-2])
        F = F.expand(*bs, *F.shape[-2:])
        v = v.expand(*bs, *v.shape[-2:])
        p, t = F.shape[-1], v.shape[-1]
        z = self.right_linear_op._matmul(_rowwise_outer(F, v))  # column r t + s: G G^T (f_r o v_s)
        res = torch.einsum("...nr,...nrs->...ns", F, z.unflatten(-1, (p, t)))
        return res.squeeze(-1) if vec else res

    def _mul_constant(self, other):
        """c (A o B) = (c A) o B for c > 0 (the left root absorbs sqrt(c)); other constants keep the product as it is
        inside a ConstantMulLinearOperator."""
        if other > 0:
            return type(self)(self.left_linear_op._mul_constant(other), self.right_linear_op)
        return super()._mul_constant(other)

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """Derivatives with respect to both roots' tensors.  Native: dF and dG of the two dense roots in one call
        (lo_hadamard_bilinear_f32), pulled back to the roots' representations."""
        roots = self._roots()
        if roots is not None and left_vecs.is_cuda and left_vecs.dtype == torch.float32:
            from .. import kernels as K

            F, G = roots
            dF, dG = K.bilinear_hadamard(F.detach(), G.detach(), left_vecs, right_vecs)
            dF = dF if dF.shape == F.shape else dF.sum_to_size(*F.shape)
            dG = dG if dG.shape == G.shape else dG.sum_to_size(*G.shape)
            return _root_pullback(self.left_linear_op, dF) + _root_pullback(self.right_linear_op, dG)
        return self._bilinear_derivative_composition(left_vecs, right_vecs)

    def _bilinear_derivative_composition(self, left_vecs: Tensor, right_vecs: Tensor):
        """u^T (A o G G^T) v = sum_j (u o g_j)^T A (v o g_j): each side's derivative is its own bilinear derivative on
        the vectors multiplied row-wise by the other side's root columns."""
        if left_vecs.dim() == 1:
            left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
        F = self.left_linear_op.root.to_dense()
        G = self.right_linear_op.root.to_dense()
        grads_left = self.left_linear_op._bilinear_derivative(_rowwise_outer(left_vecs, G), _rowwise_outer(right_vecs, G))
        grads_right = self.right_linear_op._bilinear_derivative(_rowwise_outer(left_vecs, F),
                                                                _rowwise_outer(right_vecs, F))
        return tuple(grads_left) + tuple(grads_right)

    def _expand_batch(self, batch_shape):
        return type(self)(self.left_linear_op._expand_batch(batch_shape), self.right_linear_op._expand_batch(batch_shape))

    def to_dense(self) -> Tensor:
        return self.left_linear_op.to_dense() * self.right_linear_op.to_dense()

    def _size(self) -> torch.Size:
        return self.left_linear_op.size()

    def _transpose_nonbatch(self):
        return self  # (a product of symmetric matrices taken elementwise is symmetric)


__all__ = ["MulLinearOperator"]
