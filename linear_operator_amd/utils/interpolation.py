"""Sparse interpolation W (J nonzeros per row; reference: linear_operator/utils/interpolation.py).

`left_interp` (W u) and `left_t_interp` (W^T v) run on the gfx950 kernels of csrc/lo_ski.hip for fp32 HIP tensors with
int64 indices and no autograd graph to record (W^T v is deterministic: a segmented gather over a grid-major copy of W,
no float atomics); otherwise they take the reference's gather / scatter composition in torch.
"""
from __future__ import annotations

import torch

from .broadcasting import _matmul_broadcast_shape


def _native_ok(interp_indices, interp_values, rhs) -> bool:
    if not (rhs.is_cuda and rhs.dtype == torch.float32 and interp_values.is_cuda
            and interp_values.dtype == torch.float32 and interp_indices.is_cuda
            and interp_indices.dtype == torch.int64):
        return False
    return not (torch.is_grad_enabled() and (rhs.requires_grad or interp_values.requires_grad))


def left_interp(interp_indices, interp_values, rhs):
    """W rhs: interp_indices / interp_values [*batch, n, J], rhs [*batch, m, c] or [m] -> [*batch, n, c] or [n]."""
    is_vector = rhs.ndimension() == 1
    if _native_ok(interp_indices, interp_values, rhs) and not (is_vector and interp_indices.dim() > 2):
        from .. import kernels as K

        r = rhs.unsqueeze(-1) if is_vector else rhs
        num_rows, num_interp = interp_indices.shape[-2:]
        shape = _matmul_broadcast_shape(torch.Size((*interp_indices.shape[:-1], r.size(-2))), r.shape)
        batch = shape[:-2]
        idx = interp_indices.expand(*batch, num_rows, num_interp).reshape(-1, num_rows, num_interp)
        vals = interp_values.expand(*batch, num_rows, num_interp).reshape(-1, num_rows, num_interp)
        u = r.expand(*batch, *r.shape[-2:]).reshape(-1, *r.shape[-2:])
        res = K.interp(idx, vals, u).reshape(*batch, num_rows, r.size(-1))
        return res.squeeze(-1) if is_vector else res
    if is_vector:
        res = rhs.index_select(0, interp_indices.view(-1)).view(*interp_values.size())
        res = res.mul(interp_values)
        return res.sum(-1)
    num_rows, num_interp = interp_indices.shape[-2:]
    num_data, num_columns = rhs.shape[-2:]
    interp_shape = torch.Size((*interp_indices.shape[:-1], num_data))
    output_shape = _matmul_broadcast_shape(interp_shape, rhs.shape)
    batch_shape = output_shape[:-2]
    interp_indices_expanded = interp_indices.unsqueeze(-1).expand(*batch_shape, num_rows, num_interp, num_columns)
    interp_values_expanded = interp_values.unsqueeze(-1).expand(*batch_shape, num_rows, num_interp, num_columns)
    rhs_expanded = rhs.unsqueeze(-2).expand(*batch_shape, num_data, num_interp, num_columns)
    res = rhs_expanded.gather(-3, interp_indices_expanded).mul(interp_values_expanded)
    return res.sum(-2)


def left_t_interp(interp_indices, interp_values, rhs, output_dim):
    """W^T rhs: interp_indices / interp_values [*batch, n, J], rhs [*batch, n, c] or [n] -> [*batch, output_dim, c]."""
    is_vector = rhs.ndimension() == 1
    if is_vector:
        rhs = rhs.unsqueeze(-1)
    num_data, num_interp = interp_values.shape[-2:]
    num_cols = rhs.size(-1)
    interp_shape = torch.Size((*interp_indices.shape[:-2], output_dim, num_data))
    output_shape = _matmul_broadcast_shape(interp_shape, rhs.shape)
    batch_shape = output_shape[:-2]
    if _native_ok(interp_indices, interp_values, rhs):
        from .. import kernels as K

        idx = interp_indices.expand(*batch_shape, num_data, num_interp).reshape(-1, num_data, num_interp)
        vals = interp_values.expand(*batch_shape, num_data, num_interp).reshape(-1, num_data, num_interp)
        v = rhs.expand(*batch_shape, num_data, num_cols).reshape(-1, num_data, num_cols)
        res = K.interp_t(idx, vals, v, output_dim).reshape(*batch_shape, output_dim, num_cols)
        return res.squeeze(-1) if is_vector else res
    # the reference sums through a sparse [batch, output_dim, n J] matrix; index_add_ is the same scatter-sum
    values = (rhs.unsqueeze(-2) * interp_values.unsqueeze(-1)).expand(*batch_shape, num_data, num_interp, num_cols)
    batch_size = batch_shape.numel()
    idx = interp_indices.expand(*batch_shape, num_data, num_interp).reshape(batch_size, num_data * num_interp)
    offs = torch.arange(batch_size, device=idx.device).unsqueeze(-1) * output_dim
    res = torch.zeros(batch_size * output_dim, num_cols, dtype=values.dtype, device=values.device)
    res = res.index_add(0, (idx + offs).reshape(-1), values.reshape(-1, num_cols))
    res = res.view(*batch_shape, output_dim, num_cols)
    return res.squeeze(-1) if is_vector else res


__all__ = ["left_interp", "left_t_interp"]
