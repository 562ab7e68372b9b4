"""InterpolatedLinearOperator  W_l K W_r^T  (reference: linear_operator/operators/interpolated_linear_operator.py).

The structured kernel interpolation of KISS-GP / SKI: K is a (batch of) base operator(s) on M grid points, W_l / W_r
sparse interpolation matrices with J nonzeros per row, stored as int64 indices and values [*batch, rows, J].

With a symmetric Toeplitz base and fp32 HIP tensors, a square operator lowers to LO_OP_SKI_DIAG (csrc/lo_ski.hip):
`_matmul`, CG, Lanczos, MINRES and the pivoted Cholesky run on the device, W_r^T v from a grid-major copy of W_r built
once per plan.  A Kronecker product of 2 or 3 Toeplitz factors (SKI on a 2-D / 3-D grid) lowers to LO_OP_SKI_GRID_DIAG
(csrc/lo_ski_grid.hip) the same way.  Other bases (dense bases, more factors) and rectangular operators compose the
interpolation kernels (utils/interpolation.py) with the base's own `_matmul`.
"""
from __future__ import annotations

import torch
from torch import Tensor

from ..utils.interpolation import left_interp, left_t_interp
from ._linear_operator import LinearOperator
from .dense_linear_operator import DenseLinearOperator, to_linear_operator
from .diag_linear_operator import DiagLinearOperator
from .root_linear_operator import RootLinearOperator
from .toeplitz_linear_operator import ToeplitzLinearOperator


def _to_helper(*args, **kwargs):
    """(device, dtype) of a `.to(...)` call (reference utils/generic.py)."""
    device = kwargs.get("device")
    dtype = kwargs.get("dtype")
    for arg in args:
        if isinstance(arg, torch.dtype):
            dtype = arg
        elif isinstance(arg, (torch.device, str)):
            device = torch.device(arg)
        elif torch.is_tensor(arg):
            device, dtype = arg.device, arg.dtype
    return device, dtype


# Which products of the grid kind `_matmul` hands to the kernels, by (grid axes, one column / more columns): True only
# where tools/mb_ski_grid.py measured the native product at least as fast as the composition `_matmul` otherwise runs
# (DESIGN.md section 6h holds both times of every cell).  A cell that is absent keeps the composition; the descriptor
# still serves CG, Lanczos, MINRES and the pivoted Cholesky, where it replaces a Python call per product.  Measured
# (native / composition, microseconds; 1 column, 17 columns):
#   2-D  1 x 65536 on 128 (x) 128, J 16            40 /   382     112 /  4288
#   2-D  16 x 16384 on 64 (x) 64, J 16            153 /   533     275 /  2397
#   3-D  1 x 65536 on 32 (x) 32 (x) 32, J 64      121 /  2939     308 / 41478
_NATIVE_MATMUL: dict = {(2, 1): True, (2, 2): True, (3, 1): True, (3, 2): True}


def _toeplitz_kron_columns(base):
    """The factors' first columns when `base` is a Kronecker product of 2 or 3 symmetric Toeplitz operators, else None."""
    from .kronecker_product_linear_operator import KroneckerProductLinearOperator

    if not isinstance(base, KroneckerProductLinearOperator) or len(base.linear_ops) not in (2, 3):
        return None
    if not all(isinstance(op, ToeplitzLinearOperator) for op in base.linear_ops):
        return None
    return [op.column for op in base.linear_ops]


class InterpolatedLinearOperator(LinearOperator):
    def _check_args(self, base_linear_op, left_interp_indices, left_interp_values, right_interp_indices,
                    right_interp_values):  # reference :20-41
        if left_interp_indices.size() != left_interp_values.size():
            return "Expected left_interp_indices ({}) to have the same size as left_interp_values ({})".format(
                left_interp_indices.size(), left_interp_values.size())
        if right_interp_indices.size() != right_interp_values.size():
            return "Expected right_interp_indices ({}) to have the same size as right_interp_values ({})".format(
                right_interp_indices.size(), right_interp_values.size())
        if left_interp_indices.shape[:-2] != right_interp_indices.shape[:-2]:
            return ("left interp size ({}) is incompatible with right interp size ({}). Make sure the two have the "
                    "same number of batch dimensions".format(left_interp_indices.size(), right_interp_indices.size()))
        if left_interp_indices.shape[:-2] != base_linear_op.shape[:-2]:
            return ("left interp size ({}) is incompatible with base lazy tensor size ({}). Make sure the two have the "
                    "same number of batch dimensions".format(left_interp_indices.size(), base_linear_op.size()))

    def __init__(self, base_linear_op, left_interp_indices=None, left_interp_values=None, right_interp_indices=None,
                 right_interp_values=None):  # reference :43-92
        base_linear_op = to_linear_operator(base_linear_op)
        if left_interp_indices is None:
            num_rows = base_linear_op.size(-2)
            left_interp_indices = torch.arange(0, num_rows, dtype=torch.long, device=base_linear_op.device)
            left_interp_indices.unsqueeze_(-1)
            left_interp_indices = left_interp_indices.expand(*base_linear_op.batch_shape, num_rows, 1)
        if left_interp_values is None:
            left_interp_values = torch.ones(left_interp_indices.size(), dtype=base_linear_op.dtype,
                                            device=base_linear_op.device)
        if right_interp_indices is None:
            num_cols = base_linear_op.size(-1)
            right_interp_indices = torch.arange(0, num_cols, dtype=torch.long, device=base_linear_op.device)
            right_interp_indices.unsqueeze_(-1)
            right_interp_indices = right_interp_indices.expand(*base_linear_op.batch_shape, num_cols, 1)
        if right_interp_values is None:
            right_interp_values = torch.ones(right_interp_indices.size(), dtype=base_linear_op.dtype,
                                             device=base_linear_op.device)
        if left_interp_indices.shape[:-2] != base_linear_op.batch_shape:
            try:
                base_linear_op = base_linear_op._expand_batch(left_interp_indices.shape[:-2])
            except RuntimeError:
                raise RuntimeError("interp size ({}) is incompatible with base_linear_op size ({}). ".format(
                    right_interp_indices.size(), base_linear_op.size()))
        super().__init__(base_linear_op, left_interp_indices, left_interp_values, right_interp_indices,
                         right_interp_values)
        self.base_linear_op = base_linear_op
        self.left_interp_indices = left_interp_indices
        self.left_interp_values = left_interp_values
        self.right_interp_indices = right_interp_indices
        self.right_interp_values = right_interp_values

    # ------------------------------------------------------------------ lowering
    def _kernel_descriptor(self, batch_shape=None):
        """LO_OP_SKI_DIAG for a square operator over a symmetric Toeplitz base, LO_OP_SKI_GRID_DIAG over a Kronecker
        product of 2 or 3 of them (axes and grid within the kernel's limits), fp32 HIP tensors; else None."""
        base = self.base_linear_op
        if not isinstance(base, ToeplitzLinearOperator):
            return self._grid_descriptor(batch_shape)
        col = base.column
        li, lv, ri, rv = (self.left_interp_indices, self.left_interp_values, self.right_interp_indices,
                          self.right_interp_values)
        if not (col.is_cuda and col.dtype == torch.float32 and lv.dtype == torch.float32
                and rv.dtype == torch.float32 and li.is_cuda and ri.is_cuda and lv.is_cuda and rv.is_cuda):
            return None
        if li.shape[-2:] != ri.shape[-2:]:
            return None
        from .. import kernels as K

        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        M = col.size(-1)
        N, J = li.shape[-2:]
        shared = li is ri and lv is rv
        ex = lambda t: t.expand(*bs, N, J)  # noqa: E731
        li_e, lv_e = ex(li), ex(lv)
        ri_e, rv_e = (li_e, lv_e) if shared else (ex(ri), ex(rv))
        # the grid-major copy of W_r is kept across calls (memo keyed on the index tensor): a matvec or a solve on the
        # same indices does not rebuild it
        desc = K.ski_diag_descriptor(col.expand(*bs, M), li_e, lv_e, ri_e, rv_e, None)
        if desc is not None:
            desc.interp_plan = K.interp_plan(ri, bs, M)
        return desc

    def _grid_descriptor(self, batch_shape=None):
        cols = _toeplitz_kron_columns(self.base_linear_op)
        if cols is None:
            return None
        li, lv, ri, rv = (self.left_interp_indices, self.left_interp_values, self.right_interp_indices,
                          self.right_interp_values)
        if not all(t.is_cuda and t.dtype == torch.float32 for t in (*cols, lv, rv)) or not (li.is_cuda and ri.is_cuda):
            return None
        if li.shape[-2:] != ri.shape[-2:]:
            return None
        from .. import kernels as K

        grid = tuple(int(t.shape[-1]) for t in cols)
        if not K.ski_grid_shape_ok(grid):
            return None
        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        M = self.base_linear_op.size(-1)
        N, J = li.shape[-2:]
        shared = li is ri and lv is rv
        ex = lambda t: t.expand(*bs, N, J)  # noqa: E731
        li_e, lv_e = ex(li), ex(lv)
        ri_e, rv_e = (li_e, lv_e) if shared else (ex(ri), ex(rv))
        desc = K.ski_grid_diag_descriptor(cols, li_e, lv_e, ri_e, rv_e, None)
        if desc is not None:
            desc.interp_plan = K.interp_plan(ri, bs, M)
        return desc

    # ------------------------------------------------------------------ reference methods
    def _approx_diagonal(self) -> Tensor:  # :94-101
        base_diag_root = self.base_linear_op._diagonal().sqrt()
        left_res = left_interp(self.left_interp_indices, self.left_interp_values, base_diag_root.unsqueeze(-1))
        right_res = left_interp(self.right_interp_indices, self.right_interp_values, base_diag_root.unsqueeze(-1))
        res = left_res * right_res
        return res.squeeze(-1)

    def _diagonal(self) -> Tensor:  # :103-117
        if isinstance(self.base_linear_op, RootLinearOperator) and isinstance(self.base_linear_op.root,
                                                                               DenseLinearOperator):
            left_interp_vals = left_interp(self.left_interp_indices, self.left_interp_values,
                                           self.base_linear_op.root.to_dense())
            right_interp_vals = left_interp(self.right_interp_indices, self.right_interp_values,
                                            self.base_linear_op.root.to_dense())
            return (left_interp_vals * right_interp_vals).sum(-1)
        # the generic diagonal: K[i, i] through _get_indices
        n = self.size(-1)
        idx = torch.arange(n, device=self.device)
        batch_idx = []
        for i, size in enumerate(self.batch_shape):
            shape = [1] * (len(self.batch_shape) + 1)
            shape[i] = size
            batch_idx.append(torch.arange(size, device=self.device).view(*shape))
        return self._get_indices(idx, idx, *batch_idx)

    def _expand_batch(self, batch_shape):  # :119-128
        return self.__class__(
            self.base_linear_op._expand_batch(batch_shape),
            self.left_interp_indices.expand(*batch_shape, *self.left_interp_indices.shape[-2:]),
            self.left_interp_values.expand(*batch_shape, *self.left_interp_values.shape[-2:]),
            self.right_interp_indices.expand(*batch_shape, *self.right_interp_indices.shape[-2:]),
            self.right_interp_values.expand(*batch_shape, *self.right_interp_values.shape[-2:]),
        )

    def _get_indices(self, row_index, col_index, *batch_indices) -> Tensor:  # :130-144
        left_interp_indices = self.left_interp_indices.__getitem__((*batch_indices, row_index)).unsqueeze(-2)
        right_interp_indices = self.right_interp_indices.__getitem__((*batch_indices, col_index)).unsqueeze(-1)
        base_vals = self.base_linear_op._get_indices(
            left_interp_indices,
            right_interp_indices,
            *[batch_index.view(*batch_index.shape, 1, 1) for batch_index in batch_indices],
        )
        left_interp_values = self.left_interp_values.__getitem__((*batch_indices, row_index)).unsqueeze(-2)
        right_interp_values = self.right_interp_values.__getitem__((*batch_indices, col_index)).unsqueeze(-1)
        interp_values = left_interp_values * right_interp_values
        return (base_vals * interp_values).sum([-2, -1])

    def _matmul(self, rhs: Tensor) -> Tensor:  # :192-219
        is_vector = rhs.ndimension() == 1
        if is_vector:
            rhs = rhs.unsqueeze(-1)
        if rhs.is_cuda and rhs.dtype == torch.float32 and self.size(-1) == self.size(-2):
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
            if desc is not None and desc.grid and not _NATIVE_MATMUL.get(
                    (len(desc.grid), 1 if rhs.shape[-1] == 1 else 2), False):
                desc = None  # (a cell of the routing table where the composition measured faster)
            if desc is not None:
                from .. import kernels as K

                res = K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
                return res.squeeze(-1) if is_vector else res
        right_interp_res = left_t_interp(self.right_interp_indices, self.right_interp_values, rhs,
                                         self.base_linear_op.size(-1))
        base_res = self.base_linear_op._matmul(right_interp_res)
        res = left_interp(self.left_interp_indices, self.left_interp_values, base_res)
        return res.squeeze(-1) if is_vector else res

    def _mul_constant(self, other):  # :221-232 (applied to the base: the interpolated structure is kept)
        base = self.base_linear_op
        new_base = base._mul_constant(other) if hasattr(base, "_mul_constant") else to_linear_operator(
            base.to_dense() * other)
        return self.__class__(new_base, self.left_interp_indices, self.left_interp_values, self.right_interp_indices,
                              self.right_interp_values)

    def _t_matmul(self, rhs: Tensor) -> Tensor:  # :234-261
        is_vector = rhs.ndimension() == 1
        if is_vector:
            rhs = rhs.unsqueeze(-1)
        left_interp_res = left_t_interp(self.left_interp_indices, self.left_interp_values, rhs,
                                        self.base_linear_op.size(-2))
        base_res = self.base_linear_op._t_matmul(left_interp_res)
        res = left_interp(self.right_interp_indices, self.right_interp_values, base_res)
        return res.squeeze(-1) if is_vector else res

    def _base_grads(self, left_res, right_res):
        base = self.base_linear_op
        from .kronecker_product_linear_operator import KroneckerProductLinearOperator

        if isinstance(base, KroneckerProductLinearOperator) and any(
                isinstance(op, ToeplitzLinearOperator) for op in base.linear_ops):
            reps = base.representation()
            if not any(t.requires_grad for t in reps):
                return [torch.zeros_like(t) for t in reps]
            raise NotImplementedError(
                "InterpolatedLinearOperator: gradients with respect to the Toeplitz factors of a Kronecker-product "
                "base (2-D SKI grid) are not implemented; detach the factors' columns (the interpolation values "
                "still receive gradients)")
        return list(base._bilinear_derivative(left_res, right_res))

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):  # :263-328
        if left_vecs.ndimension() == 1:
            left_vecs = left_vecs.unsqueeze(1)
            right_vecs = right_vecs.unsqueeze(1)
        base = self.base_linear_op
        batch = torch.broadcast_shapes(self.batch_shape, left_vecs.shape[:-2], right_vecs.shape[:-2])
        op = self if batch == self.batch_shape else self._expand_batch(batch)
        left_vecs = left_vecs.expand(*batch, *left_vecs.shape[-2:])
        right_vecs = right_vecs.expand(*batch, *right_vecs.shape[-2:])
        li, lv, ri, rv = (op.left_interp_indices, op.left_interp_values, op.right_interp_indices,
                          op.right_interp_values)
        # base gradient from the vectors taken to the grid
        left_res = left_t_interp(li, lv, left_vecs, base.size(-2))
        right_res = left_t_interp(ri, rv, right_vecs, base.size(-1))
        base_grads = op._base_grads(left_res, right_res)
        # interpolation-value gradients: gather-dot of the vectors with the base's products on the grid
        cols = _toeplitz_kron_columns(op.base_linear_op)
        grid_native = False
        if cols is not None and right_res.is_cuda and right_res.dtype == torch.float32 and all(
                t.is_cuda and t.dtype == torch.float32 for t in cols):
            from .. import kernels as K

            grid_native = K.ski_grid_shape_ok(tuple(int(t.shape[-1]) for t in cols))
        if grid_native:  # the two grid products through the native Kronecker-of-Toeplitz kernel (symmetric: T^T = T)
            flat_cols = [t.detach().expand(*batch, t.shape[-1]).reshape(-1, t.shape[-1]) for t in cols]
            gp = lambda g: K.toeplitz_kron_mv(flat_cols, g.reshape(-1, *g.shape[-2:])).reshape(g.shape)  # noqa: E731
            rr, ll = gp(right_res), gp(left_res)
        else:
            rr = op.base_linear_op._matmul(right_res).contiguous()
            ll = op.base_linear_op._t_matmul(left_res).contiguous()
        native = (rr.is_cuda and rr.dtype == torch.float32 and li.is_cuda and li.dtype == torch.int64
                  and left_vecs.dtype == torch.float32)
        if native:
            from .. import kernels as K

            def vgrad(idx, vecs, R):
                n, j = idx.shape[-2:]
                flat = lambda t, *s: t.expand(*batch, *t.shape[-2:]).reshape(-1, *t.shape[-2:])  # noqa: E731
                return K.interp_values_grad(flat(idx), flat(vecs), flat(R)).reshape(*batch, n, j)

            left_values_grad = vgrad(li, left_vecs, rr)
            right_values_grad = vgrad(ri, right_vecs, ll)
        else:
            def vgrad(idx, vecs, R):
                n, j = idx.shape[-2:]
                sel = R.gather(-2, idx.reshape(*batch, n * j, 1).expand(*batch, n * j, R.size(-1)))
                return (sel.view(*batch, n, j, R.size(-1)) * vecs.unsqueeze(-2)).sum(-1)

            left_values_grad = vgrad(li, left_vecs, rr)
            right_values_grad = vgrad(ri, right_vecs, ll)
        left_values_grad = left_values_grad.sum_to_size(*self.left_interp_values.shape)
        right_values_grad = right_values_grad.sum_to_size(*self.right_interp_values.shape)
        base_reps = base.representation()
        base_grads = [g if g is None or tuple(g.shape) == tuple(t.shape) else g.sum_to_size(*t.shape)
                      for g, t in zip(base_grads, base_reps)]
        return tuple(base_grads + [torch.zeros_like(self.left_interp_indices), left_values_grad,
                                   torch.zeros_like(self.right_interp_indices), right_values_grad])

    def _size(self) -> torch.Size:  # :330-333
        return torch.Size(self.base_linear_op.batch_shape + (self.left_interp_indices.size(-2),
                                                             self.right_interp_indices.size(-2)))

    def _transpose_nonbatch(self):  # :335-345
        return self.__class__(self.base_linear_op.mT, self.right_interp_indices, self.right_interp_values,
                              self.left_interp_indices, self.left_interp_values)

    def matmul(self, other):  # :413-451
        if isinstance(other, DiagLinearOperator):
            new_right_interp_values = self.right_interp_values * other._diag.unsqueeze(-1)
            return InterpolatedLinearOperator(
                base_linear_op=self.base_linear_op,
                left_interp_indices=self.left_interp_indices,
                left_interp_values=self.left_interp_values,
                right_interp_indices=self.right_interp_indices,
                right_interp_values=new_right_interp_values,
            )
        if torch.is_grad_enabled() and (self.requires_grad or (torch.is_tensor(other) and other.requires_grad)):
            return super().matmul(other)  # the Matmul Function: backward through _bilinear_derivative / _t_matmul
        is_vector = other.ndimension() == 1
        if is_vector:
            other = other.unsqueeze(-1)
        base_size = self.base_linear_op.size(-1)
        right_interp_res = left_t_interp(self.right_interp_indices, self.right_interp_values, other, base_size)
        base_res = self.base_linear_op._matmul(right_interp_res)
        res = left_interp(self.left_interp_indices, self.left_interp_values, base_res)
        return res.squeeze(-1) if is_vector else res

    def zero_mean_mvn_samples(self, num_samples: int) -> Tensor:  # :453-461
        base_samples = self.base_linear_op.zero_mean_mvn_samples(num_samples)
        batch_iter = tuple(range(1, base_samples.dim()))
        base_samples = base_samples.permute(*batch_iter, 0)
        res = left_interp(self.left_interp_indices, self.left_interp_values, base_samples).contiguous()
        batch_iter = tuple(range(res.dim() - 1))
        return res.permute(-1, *batch_iter).contiguous()

    def to(self, *args, **kwargs):  # :463-490: the index tensors keep their integer dtype
        device, dtype = _to_helper(*args, **kwargs)
        new_args = []
        for arg in self._args:
            if hasattr(arg, "to"):
                if dtype is not None and hasattr(arg, "dtype") and arg.dtype.is_floating_point == dtype.is_floating_point:
                    new_args.append(arg.to(dtype=dtype, device=device))
                else:
                    new_args.append(arg.to(device=device))
            else:
                new_args.append(arg)
        return self.__class__(*new_args)


__all__ = ["InterpolatedLinearOperator"]
