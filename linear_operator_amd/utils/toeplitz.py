"""Symmetric Toeplitz helpers (reference: linear_operator/utils/toeplitz.py).

`sym_toeplitz_matmul` and `sym_toeplitz_derivative_quadratic_form` run on the gfx950 kernels of csrc/lo_ski.hip for
fp32 HIP tensors with a grid of at most LO_TOEPLITZ_MAX_M points and no autograd graph to record; otherwise (CPU, fp64,
larger grids, inputs that require grad) they take the reference's circulant-FFT composition in torch.
"""
from __future__ import annotations

import torch
from torch.fft import fft, ifft

from . import broadcasting


def _native_ok(*ts) -> bool:
    from .. import _hip

    if not all(t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return False
    return ts[0].size(-1) <= _hip.LO_TOEPLITZ_MAX_M


def toeplitz(toeplitz_column, toeplitz_row):
    """Dense Toeplitz matrix from its first column and first row (vectors of one length n)."""
    if toeplitz_column.ndimension() != 1:
        raise RuntimeError("toeplitz_column must be a vector.")
    if toeplitz_row.ndimension() != 1:
        raise RuntimeError("toeplitz_row must be a vector.")
    if toeplitz_column[0] != toeplitz_row[0]:
        raise RuntimeError(
            "The first column and first row of the Toeplitz matrix should have "
            "the same first otherwise the value of T[0,0] is ambiguous. "
            "Got: c[0]={} and r[0]={}".format(toeplitz_column[0], toeplitz_row[0])
        )
    if len(toeplitz_column) != len(toeplitz_row):
        raise RuntimeError("c and r should have the same length (Toeplitz matrices are necessarily square).")
    if type(toeplitz_column) != type(toeplitz_row):
        raise RuntimeError("toeplitz_column and toeplitz_row should be the same type.")
    n = len(toeplitz_column)
    if n == 1:
        return toeplitz_column.view(1, 1)
    lag = torch.arange(n, device=toeplitz_column.device)
    lag = lag.unsqueeze(-1) - lag.unsqueeze(0)  # i - j
    return torch.where(lag >= 0, toeplitz_column[lag.clamp(min=0)], toeplitz_row[(-lag).clamp(min=0)])


def sym_toeplitz(toeplitz_column):
    """Dense symmetric Toeplitz matrix from its first column."""
    return toeplitz(toeplitz_column, toeplitz_column)


def toeplitz_matmul(toeplitz_column, toeplitz_row, tensor):
    """T M for the Toeplitz matrix of (column, row), by circulant embedding and torch.fft (reference toeplitz.py)."""
    if toeplitz_column.size() != toeplitz_row.size():
        raise RuntimeError("c and r should have the same length (Toeplitz matrices are necessarily square).")
    toeplitz_shape = torch.Size((*toeplitz_column.shape, toeplitz_row.size(-1)))
    output_shape = broadcasting._matmul_broadcast_shape(toeplitz_shape, tensor.shape)
    broadcasted_t_shape = output_shape[:-1] if tensor.dim() > 1 else output_shape
    if tensor.ndimension() == 1:
        tensor = tensor.unsqueeze(-1)
    toeplitz_column = toeplitz_column.expand(*broadcasted_t_shape)
    toeplitz_row = toeplitz_row.expand(*broadcasted_t_shape)
    tensor = tensor.expand(*output_shape)
    if not torch.equal(toeplitz_column[..., 0], toeplitz_row[..., 0]):
        raise RuntimeError(
            "The first column and first row of the Toeplitz matrix should have "
            "the same first element, otherwise the value of T[0,0] is ambiguous. "
            "Got: c[0]={} and r[0]={}".format(toeplitz_column[0], toeplitz_row[0])
        )
    if type(toeplitz_column) != type(toeplitz_row) or type(toeplitz_column) != type(tensor):
        raise RuntimeError("The types of all inputs to ToeplitzMV must match.")
    *batch_shape, orig_size, num_rhs = tensor.size()
    r_reverse = toeplitz_row[..., 1:].flip(dims=(-1,))
    c_r_rev = torch.zeros(*batch_shape, orig_size + r_reverse.size(-1), dtype=tensor.dtype, device=tensor.device)
    c_r_rev[..., :orig_size] = toeplitz_column
    c_r_rev[..., orig_size:] = r_reverse
    temp_tensor = torch.zeros(
        *batch_shape, 2 * orig_size - 1, num_rhs, dtype=toeplitz_column.dtype, device=toeplitz_column.device
    )
    temp_tensor[..., :orig_size, :] = tensor
    fft_M = fft(temp_tensor.mT.contiguous())
    fft_c = fft(c_r_rev).unsqueeze(-2).expand_as(fft_M)
    fft_product = fft_M.mul_(fft_c)
    output = ifft(fft_product).real.mT
    return output[..., :orig_size, :]


def sym_toeplitz_matmul(toeplitz_column, tensor):
    """T M for the symmetric Toeplitz matrix of `toeplitz_column` ([*batch, n]); M [*batch, n, p] or [n]."""
    if _native_ok(toeplitz_column, tensor):
        from .. import kernels as K

        is_vec = tensor.dim() == 1
        rhs = tensor.unsqueeze(-1) if is_vec else tensor
        shape = broadcasting._matmul_broadcast_shape(torch.Size((*toeplitz_column.shape, toeplitz_column.size(-1))),
                                                     rhs.shape)
        batch, M = shape[:-2], toeplitz_column.size(-1)
        col = toeplitz_column.expand(*batch, M).reshape(-1, M)
        res = K.toeplitz_mv(col, rhs.expand(*batch, M, rhs.size(-1)).reshape(-1, M, rhs.size(-1)))
        res = res.reshape(*batch, M, rhs.size(-1))
        return res.squeeze(-1) if is_vec else res
    return toeplitz_matmul(toeplitz_column, toeplitz_column, tensor)


def sym_toeplitz_derivative_quadratic_form(left_vectors, right_vectors):
    r"""g_i = sum_j u_j^T (dT/dc_i) v_j for s vector pairs (u_j, v_j) ([*batch, m, s] or [m]): dT/dc_i has ones on the
    i-th sub- and superdiagonal (the identity for i = 0)."""
    if left_vectors.ndimension() == 1:
        left_vectors = left_vectors.unsqueeze(1)
        right_vectors = right_vectors.unsqueeze(1)
    if _native_ok(left_vectors.mT, right_vectors):
        from .. import kernels as K

        shape = torch.broadcast_shapes(left_vectors.shape, right_vectors.shape)
        batch, m, s = shape[:-2], shape[-2], shape[-1]
        u = left_vectors.expand(shape).reshape(-1, m, s)
        v = right_vectors.expand(shape).reshape(-1, m, s)
        return K.toeplitz_bilinear(u, v).reshape(*batch, m)
    batch_shape = left_vectors.shape[:-2]
    toeplitz_size = left_vectors.size(-2)
    num_vectors = left_vectors.size(-1)
    left_vectors = left_vectors.mT.contiguous()
    right_vectors = right_vectors.mT.contiguous()
    columns = torch.zeros_like(left_vectors)
    columns[..., 0] = left_vectors[..., 0]
    res = toeplitz_matmul(columns, left_vectors, right_vectors.unsqueeze(-1))
    rows = left_vectors.flip(dims=(-1,))
    columns[..., 0] = rows[..., 0]
    res += toeplitz_matmul(columns, rows, torch.flip(right_vectors, dims=(-1,)).unsqueeze(-1))
    res = res.reshape(*batch_shape, num_vectors, toeplitz_size).sum(-2)
    res[..., 0] -= (left_vectors * right_vectors).view(*batch_shape, -1).sum(-1)
    return res


__all__ = ["toeplitz", "sym_toeplitz", "toeplitz_matmul", "sym_toeplitz_matmul", "sym_toeplitz_derivative_quadratic_form"]
