"""BlockLinearOperator: a batch of blocks read as one matrix (reference: operators/block_linear_operator.py:15-176).
The blocks are the members of the base operator along `block_dim`, which is moved to -3 at construction; the subclasses
say how the blocks are laid out (block diagonal, interleaved block diagonal, sum).

With fp32 device vectors and a base that lowers to a dense or low-rank descriptor the product can be one call of
lo_block_mv_f32 (csrc/lo_block.hip), which reads and writes the vectors in the layout of the block operator; each
subclass takes it for the shape classes in which it measured faster (`_native_worthwhile`).
Everything else (CPU, fp64, 1-D vectors, Kronecker / Toeplitz / SKI bases, the other shape classes) takes the torch
composition: reshape to the base's batch, one batched product of the base operator, reshape back."""
from __future__ import annotations

import torch
from torch import Tensor

from ._linear_operator import LinearOperator
from .dense_linear_operator import DenseLinearOperator, _sum_to, to_linear_operator


def _is_noop_index(index) -> bool:
    return isinstance(index, slice) and index == slice(None, None, None)


class BlockLinearOperator(LinearOperator):
    _layout = None  # LO_BLOCK_* of the subclass

    def __init__(self, base_linear_op, block_dim: int = -3):
        if base_linear_op.dim() < 3:
            raise RuntimeError(
                "base_linear_op must be a batch matrix (i.e. at least 3 dimensions - got "
                "{}".format(base_linear_op.dim())
            )
        base_linear_op = to_linear_operator(base_linear_op)
        block_dim = block_dim if block_dim < 0 else (block_dim - base_linear_op.dim())
        if block_dim != -3:  # the block dimension becomes the last batch dimension
            pos = base_linear_op.dim() + block_dim
            base_linear_op = base_linear_op._permute_batch(*range(pos), *range(pos + 1, base_linear_op.dim() - 2), pos)
        super().__init__(base_linear_op)
        self.base_linear_op = base_linear_op

    @property
    def num_blocks(self) -> int:
        return self.base_linear_op.size(-3)

    def _add_batch_dim(self, other: Tensor) -> Tensor:
        raise NotImplementedError

    def _remove_batch_dim(self, other: Tensor) -> Tensor:
        raise NotImplementedError

    # ------------------------------------------------------------------ products
    def _native_descriptor(self, batch_shape):
        """The base's descriptor over (*batch_shape, T) when lo_block_mv_f32 takes it, else None."""
        from .. import kernels as K

        desc = self.base_linear_op._kernel_descriptor(torch.Size((*batch_shape, self.num_blocks)))
        if (desc is None or desc.kind not in (K._hip.LO_OP_DENSE_DIAG, K._hip.LO_OP_LOWRANK_DIAG)
                or desc.dtype != torch.float32):  # (lo_block_mv_f32: float64 bases take the composition)
            return None
        return desc

    def _matmul(self, rhs: Tensor) -> Tensor:
        if rhs.dim() >= 2 and rhs.is_cuda and rhs.dtype == torch.float32:
            batch = torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2])
            desc = self._native_descriptor(batch)
            if desc is not None and self._native_worthwhile(desc, rhs.shape[-1]):
                from .. import kernels as K

                res = K.block_matvec(desc, self._layout, self.num_blocks, rhs.expand(*batch, *rhs.shape[-2:]))
                if res is not None:  # (None: a shape the kernels leave to the composition)
                    return res
        return self._matmul_composition(rhs)

    def _native_worthwhile(self, desc, cols: int) -> bool:
        """Whether the product of this layout, base kind and column count goes to lo_block_mv_f32: only the shape
        classes in which it was measured faster than the composition beyond run-to-run spread."""
        return False

    def _matmul_composition(self, rhs: Tensor) -> Tensor:
        """Reshape to the base's batch, one batched product of the base operator, reshape back (reference :104-118)."""
        vec = rhs.dim() == 1
        if vec:
            rhs = rhs.unsqueeze(-1)
        res = self._remove_batch_dim(self.base_linear_op._matmul(self._add_batch_dim(rhs)))
        return res.squeeze(-1) if vec else res

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        if left_vecs.dim() == 1:
            left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
        left, right = self._add_batch_dim(left_vecs), self._add_batch_dim(right_vecs)
        base = self.base_linear_op
        if isinstance(base, DenseLinearOperator) and not left.is_cuda:  # (the contraction kernels are device-only)
            return (_sum_to(left @ right.mT, base.tensor.shape),)
        return base._bilinear_derivative(left.contiguous(), right.contiguous())

    # ------------------------------------------------------------------ structure-preserving transformations
    def _expand_batch(self, batch_shape):
        return self.__class__(self.base_linear_op._expand_batch(torch.Size((*batch_shape, self.num_blocks))))

    def _permute_batch(self, *dims: int):
        return self.__class__(self.base_linear_op._permute_batch(*dims, self.base_linear_op.dim() - 3))

    def _unsqueeze_batch(self, dim: int):
        return self.__class__(self.base_linear_op._unsqueeze_batch(dim))

    def _mul_constant(self, other):
        """The constant goes onto the blocks, the block structure stays (reference :152-159)."""
        from .constant_mul_linear_operator import ConstantMulLinearOperator

        if torch.is_tensor(other) and other.dim() > 0:
            other = other.unsqueeze(-1)  # one constant per member of this operator: the same for each of its blocks
        return self.__class__(ConstantMulLinearOperator(self.base_linear_op, other))

    def _transpose_nonbatch(self):
        return self.__class__(self.base_linear_op._transpose_nonbatch())

    def _getitem(self, row_index, col_index, *batch_indices):
        if _is_noop_index(row_index) and _is_noop_index(col_index):  # batch-only: the blocks stay blocks
            noop = slice(None, None, None)
            return self.__class__(self.base_linear_op._getitem(noop, noop, *batch_indices, noop))
        return super()._getitem(row_index, col_index, *batch_indices)

    def zero_mean_mvn_samples(self, num_samples: int) -> Tensor:
        res = self.base_linear_op.zero_mean_mvn_samples(num_samples)
        return self._remove_batch_dim(res.unsqueeze(-1)).squeeze(-1)


class _BlockFactor:
    """Cholesky factor of a block-diagonal operator: the factors of the blocks, in the block operator's row order
    (the block counterpart of `_TriangularFactor`, the return convention of `LinearOperator.cholesky()`)."""

    def __init__(self, block_op, base_factor):
        self.block_op, self.base_factor = block_op, base_factor

    def to_dense(self) -> Tensor:
        return self.block_op.__class__(self.base_factor.to_dense()).to_dense()

    def _cholesky_solve(self, rhs: Tensor, upper: bool = False) -> Tensor:
        vec = rhs.dim() == 1
        cols = rhs.unsqueeze(-1) if vec else rhs
        res = self.block_op._remove_batch_dim(self.base_factor._cholesky_solve(self.block_op._add_batch_dim(cols)))
        return res.squeeze(-1) if vec else res

    def inv_quad_logdet(self, inv_quad_rhs=None, logdet=False, reduce_inv_quad=True):
        return self.block_op._sum_block_terms(self.base_factor.inv_quad_logdet, inv_quad_rhs, logdet, reduce_inv_quad)


class _BlockDiagonalBase(BlockLinearOperator):
    """What BlockDiag and BlockInterleaved share: every method defers to the base operator's batched one, with the
    vectors moved between the two row orders by the subclass (reference: block_diag_linear_operator.py:78-230,
    block_interleaved_linear_operator.py:43-153)."""

    def _size(self) -> torch.Size:
        *batch, t, n, m = self.base_linear_op.shape
        return torch.Size((*batch, t * n, t * m))

    def cholesky(self, upper: bool = False):
        return _BlockFactor(self, self.base_linear_op.cholesky(upper=upper))

    _cholesky = cholesky

    def _cholesky_solve(self, rhs: Tensor, upper: bool = False) -> Tensor:
        return self._remove_batch_dim(self.base_linear_op._cholesky_solve(self._add_batch_dim(rhs), upper=upper))

    def _solve(self, rhs: Tensor, preconditioner=None, num_tridiag: int = 0):
        if num_tridiag:
            return super()._solve(rhs, preconditioner, num_tridiag=num_tridiag)
        cols = self._add_batch_dim(rhs).contiguous()
        if preconditioner is None:
            # one batched solve of the base operator, with the base's own preconditioner and engine choice (the exact
            # branch for blocks of at most max_cholesky_size rows, the fused / resident CG beyond)
            from ..functions._solve import _solve as solve_batched

            res = solve_batched(self.base_linear_op, cols)
        else:
            res = self.base_linear_op._solve(cols, preconditioner, num_tridiag=0)
        return self._remove_batch_dim(res)

    def _sum_block_terms(self, base_fn, inv_quad_rhs, logdet, reduce_inv_quad):
        if inv_quad_rhs is not None:
            vec = inv_quad_rhs.dim() == 1
            cols = inv_quad_rhs.unsqueeze(-1) if vec else inv_quad_rhs
            inv_quad_rhs = self._add_batch_dim(cols).contiguous()
        inv_quad_res, logdet_res = base_fn(inv_quad_rhs, logdet, reduce_inv_quad=reduce_inv_quad)
        if inv_quad_rhs is not None and inv_quad_res is not None and inv_quad_res.numel():
            if reduce_inv_quad:
                inv_quad_res = inv_quad_res.reshape(*self.base_linear_op.batch_shape).sum(-1)
            else:
                inv_quad_res = inv_quad_res.reshape(*self.base_linear_op.batch_shape, inv_quad_res.size(-1)).sum(-2)
        if logdet and logdet_res is not None and logdet_res.numel():
            logdet_res = logdet_res.sum(-1)
        return inv_quad_res, logdet_res

    def inv_quad_logdet(self, inv_quad_rhs=None, logdet: bool = False, reduce_inv_quad: bool = True):
        """The base's batched inv_quad_logdet, summed over the block dimension."""
        return self._sum_block_terms(self.base_linear_op.inv_quad_logdet, inv_quad_rhs, logdet, reduce_inv_quad)

    def _block_root(self, root):
        """Block operator over a batch of (not necessarily square) roots."""
        raise NotImplementedError

    def root_decomposition(self, method=None):
        from .root_linear_operator import RootLinearOperator

        return RootLinearOperator(self._block_root(self.base_linear_op.root_decomposition(method=method).root))

    def root_inv_decomposition(self, initial_vectors=None, test_vectors=None, method=None):
        from .root_linear_operator import RootLinearOperator

        if initial_vectors is not None:
            initial_vectors = self._add_batch_dim(initial_vectors).contiguous()
        base_root = self.base_linear_op.root_inv_decomposition(initial_vectors=initial_vectors, method=method).root
        return RootLinearOperator(self._block_root(base_root))

    def _root_decomposition(self):
        return self._block_root(self.base_linear_op._root_decomposition())

    def _root_inv_decomposition(self, initial_vectors=None, test_vectors=None):
        if initial_vectors is not None:
            initial_vectors = self._add_batch_dim(initial_vectors).contiguous()
        return self._block_root(self.base_linear_op._root_inv_decomposition(initial_vectors))

    def _symeig(self, eigenvectors: bool = False, return_evals_as_lazy: bool = False):
        """Eigenvalues block by block, not sorted across blocks: that keeps the eigenvectors block structured."""
        evals, evecs = self.base_linear_op._symeig(eigenvectors=eigenvectors)
        evals = self._remove_batch_dim(evals.unsqueeze(-1)).squeeze(-1)
        return evals, (self.__class__(evecs) if eigenvectors else None)


__all__ = ["BlockLinearOperator"]
