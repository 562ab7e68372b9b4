"""MaskedLinearOperator: the rows and columns of a base operator struck out by two boolean masks (the reference's
operators/masked_linear_operator.py, same constructor and results).  GPyTorch wraps the training covariance in it for
missing observations (`observation_nan_policy("mask")`, multitask GPs with unobserved tasks).

Beyond the reference: `nonzero(mask)` is taken ONCE, in the constructor; every product indexes through the kept lists
(`index_copy` into a zero buffer, `index_select` of the result), so a CG iteration no longer synchronises twice on a
boolean indexing.  With one mask for rows and columns, fp32 on the device and a base that lowers to a dense, Kronecker,
low-rank or sum descriptor, the operator lowers to LO_OP_MASKED (csrc/lo_masked.hip) and CG, Lanczos and MINRES run
without per-iteration Python.  A low-rank base is lowered algebraically instead, S (C C^T + D) S^T =
C[idx] C[idx]^T + D[idx]: an ordinary low-rank descriptor that reaches the resident engines.
"""
from __future__ import annotations

import torch
from torch import Tensor

from ._linear_operator import LinearOperator
from .block_linear_operator import _is_noop_index
from .interpolated_linear_operator import _to_helper

# Which products `_matmul` hands to lo_matvec_f32, by (base kind, one column / more columns): the combinations in which
# the native product was at least as fast as the index_copy / index_select composition on the MI355X (tools/mb_masked.py,
# DESIGN.md section 6f).  Only the dense route with one column won (1.09x - 1.49x); a dense base with more columns and
# a Kronecker base came out level or behind (0.95x - 1.08x), a sum base goes the same generic way and was not timed.
# Those keep the composition in `_matmul`; their descriptor still serves CG, Lanczos and MINRES.
_NATIVE_MATMUL = {("dense", 1): True}


def _route_key(desc, cols: int):
    from .. import kernels as K

    H = K._hip
    kind = {H.LO_OP_DENSE_DIAG: "dense", H.LO_OP_KRON_DIAG: "kron", H.LO_OP_SUM: "sum"}.get(desc.mask[0].kind)
    return kind, (1 if cols == 1 else 2)


# The operator classes are rebuilt from their tensors all the time (representation trees, detach, batch reshapes), and a
# nonzero or a comparison of the masks is a device-to-host synchronisation: the index lists of a pair of masks are taken
# once per (storage, version) and kept here, with the masks themselves so that no address is handed out again meanwhile.
MASK_MEMO_SIZE = 8
_mask_memo: "list[tuple]" = []


def _mask_key(mask: Tensor):
    return mask.data_ptr(), mask._version, tuple(mask.shape), mask.device


def _mask_lists(row_mask: Tensor, col_mask: Tensor):
    """(row_idx, col_idx, row_eq_col_mask): int64 index lists on the masks' device."""
    key = (_mask_key(row_mask), _mask_key(col_mask))
    for entry in _mask_memo:
        if entry[0] == key:
            return entry[2]
    same = key[0] == key[1] or torch.equal(row_mask, col_mask)
    row_idx = torch.nonzero(row_mask).squeeze(-1)
    col_idx = row_idx if same else torch.nonzero(col_mask).squeeze(-1)
    _mask_memo.insert(0, (key, (row_mask, col_mask), (row_idx, col_idx, same)))
    del _mask_memo[MASK_MEMO_SIZE:]
    return row_idx, col_idx, same


class MaskedLinearOperator(LinearOperator):
    def _check_args(self, base, row_mask, col_mask):
        if not isinstance(base, LinearOperator):
            return "MaskedLinearOperator expects a LinearOperator as its base."
        if row_mask.dtype != torch.bool or col_mask.dtype != torch.bool:
            return "MaskedLinearOperator expects boolean masks."
        if row_mask.shape != base.shape[-2:-1] or col_mask.shape != base.shape[-1:]:
            return "MaskedLinearOperator expects masks of sizes {} and {}: got {} and {}.".format(
                base.size(-2), base.size(-1), tuple(row_mask.shape), tuple(col_mask.shape))

    def __init__(self, base: LinearOperator, row_mask: Tensor, col_mask: Tensor):
        super().__init__(base, row_mask, col_mask)
        self.base = base
        self.row_mask = row_mask
        self.col_mask = col_mask
        # the index lists every product goes through: one nonzero per mask, none afterwards
        self.row_idx, self.col_idx, self.row_eq_col_mask = _mask_lists(row_mask, col_mask)
        self._gathered_root = None  # (key, C[idx]) of the low-rank lowering

    # ------------------------------------------------------------------ native lowering
    def _kernel_descriptor(self, batch_shape=None):
        if not self.row_eq_col_mask or self.row_idx.numel() == 0 or not self.row_idx.is_cuda:
            return None
        if self.dtype != torch.float32 or self.device.type != "cuda":
            return None
        from .. import kernels as K

        bs = torch.Size(self.batch_shape if batch_shape is None else batch_shape)
        desc = self.base._kernel_descriptor(bs)
        if desc is None or desc.dtype != torch.float32:
            return None
        if desc.kind == K._hip.LO_OP_LOWRANK_DIAG:
            return self._gathered_lowrank(desc)
        return K.masked_descriptor(desc, self.row_idx)

    def _gathered_lowrank(self, desc):
        """S (C C^T + D) S^T = C[idx] C[idx]^T + D[idx] as an LO_OP_LOWRANK_DIAG descriptor of size M; the gathered
        copy of C is kept while the base's root stays the same storage and version."""
        from .. import kernels as K

        C3 = desc.A0
        key = (C3.data_ptr(), C3._version, tuple(C3.shape))
        if self._gathered_root is None or self._gathered_root[0] != key:
            self._gathered_root = (key, C3.detach().index_select(1, self.row_idx))
        d = desc.d
        if d is not None and desc.diag_mode == K._hip.LO_DIAG_FULL:
            d = d.detach().index_select(1, self.row_idx)
        return K.OperatorDescriptor(K._hip.LO_OP_LOWRANK_DIAG, desc.B, self.row_idx.numel(), A0=self._gathered_root[1],
                                    d=d, diag_mode=desc.diag_mode, R=desc.R, batch_shape=desc.batch_shape)

    # ------------------------------------------------------------------ operator protocol
    @staticmethod
    def _expand(tensor: Tensor, idx: Tensor, size: int) -> Tensor:
        """[*batch, M, c] -> [*batch, size, c]: the rows idx filled, zeros where the mask is false."""
        if tensor.is_cuda and tensor.dtype == torch.float32 and idx.numel() > 0:
            from .. import kernels as K

            return K.mask_expand(idx, size, tensor)
        res = torch.zeros(*tensor.shape[:-2], size, tensor.size(-1), device=tensor.device, dtype=tensor.dtype)
        return res.index_copy_(-2, idx, tensor)

    def _matmul(self, rhs: Tensor) -> Tensor:
        if rhs.dim() >= 2 and rhs.is_cuda and rhs.dtype == torch.float32:
            desc = self._kernel_descriptor(torch.broadcast_shapes(self.batch_shape, rhs.shape[:-2]))
            if desc is not None and (not desc.mask or _NATIVE_MATMUL.get(_route_key(desc, rhs.shape[-1]), False)):
                from .. import kernels as K

                return K.matvec(desc, rhs.expand(*desc.batch_shape, *rhs.shape[-2:]))
        return self._matmul_composition(rhs)

    def _matmul_composition(self, rhs: Tensor) -> Tensor:
        """The reference's product through the kept index lists: no boolean indexing, no synchronisation."""
        vec = rhs.dim() == 1
        v = rhs.unsqueeze(-1) if vec else rhs
        res = torch.zeros(*v.shape[:-2], self.base.size(-1), v.size(-1), device=v.device, dtype=v.dtype)
        res = self.base._matmul(res.index_copy_(-2, self.col_idx, v)).index_select(-2, self.row_idx)
        return res.squeeze(-1) if vec else res

    def _t_matmul(self, rhs: Tensor) -> Tensor:
        vec = rhs.dim() == 1
        v = rhs.unsqueeze(-1) if vec else rhs
        res = torch.zeros(*v.shape[:-2], self.base.size(-2), v.size(-1), device=v.device, dtype=v.dtype)
        res = self.base._t_matmul(res.index_copy_(-2, self.row_idx, v)).index_select(-2, self.col_idx)
        return res.squeeze(-1) if vec else res

    def _size(self) -> torch.Size:
        return torch.Size((*self.base.shape[:-2], self.row_idx.numel(), self.col_idx.numel()))

    def _transpose_nonbatch(self):
        return self.__class__(self.base.mT, self.col_mask, self.row_mask)

    def _diagonal(self) -> Tensor:
        if not self.row_eq_col_mask:
            raise NotImplementedError()
        return self.base.diagonal().index_select(-1, self.row_idx)

    def to_dense(self) -> Tensor:
        return self.base.to_dense().index_select(-2, self.row_idx).index_select(-1, self.col_idx)

    def _bilinear_derivative(self, left_vecs: Tensor, right_vecs: Tensor):
        """The base's own contraction on the expanded vector blocks; the masks have no derivative."""
        if left_vecs.dim() == 1:
            left_vecs, right_vecs = left_vecs.unsqueeze(-1), right_vecs.unsqueeze(-1)
        left = self._expand(left_vecs, self.row_idx, self.base.size(-2))
        right = self._expand(right_vecs, self.col_idx, self.base.size(-1))
        return tuple(self.base._bilinear_derivative(left, right)) + (None, None)

    def _expand_batch(self, batch_shape):
        return self.__class__(self.base._expand_batch(batch_shape), self.row_mask, self.col_mask)

    def _unsqueeze_batch(self, dim: int):
        return self.__class__(self.base._unsqueeze_batch(dim), self.row_mask, self.col_mask)

    def _permute_batch(self, *dims: int):
        return self.__class__(self.base._permute_batch(*dims), self.row_mask, self.col_mask)

    def _getitem(self, row_index, col_index, *batch_indices):
        if _is_noop_index(row_index) and _is_noop_index(col_index):
            if len(batch_indices):  # batch-only: the masked operator stays one
                return self.__class__(self.base[batch_indices], self.row_mask, self.col_mask)
            return self
        return super()._getitem(row_index, col_index, *batch_indices)

    def _get_indices(self, row_index: Tensor, col_index: Tensor, *batch_indices: Tensor) -> Tensor:
        return self.base._get_indices(self.row_idx[row_index], self.col_idx[col_index], *batch_indices)

    def _get_rows(self, row_index: Tensor) -> Tensor:
        """Row row_index[b] of member b: the base's row idx[row_index[b]] with the masked columns dropped (the access
        the pivoted Cholesky makes per pivot)."""
        return self.base._get_rows(self.row_idx[row_index]).index_select(-1, self.col_idx)

    def to(self, *args, **kwargs):  # the boolean masks change device only, never dtype
        device, dtype = _to_helper(*args, **kwargs)
        new_args = []
        for arg in self._args:
            if torch.is_tensor(arg) and arg.dtype == torch.bool:
                new_args.append(arg.to(device=device))
            elif hasattr(arg, "to"):
                new_args.append(arg.to(device=device, dtype=dtype))
            else:
                new_args.append(arg)
        return self.__class__(*new_args)


__all__ = ["MaskedLinearOperator"]
