"""Autograd Functions of the dense symmetric eigendecomposition on the exact small-N path: the native batched float64
eigensolver (csrc/lo_eigh_f64.hip, through kernels.eigh) with the pull-back of the ATen call it replaces
(torch.linalg.eigh / eigvalsh, Hermitian case), and the routing between the two.

`impl` holds the kernel wrapper the Functions call.  It is a seam for exactly one purpose: a test substitutes a float64
torch implementation to run `torch.autograd.gradcheck` on the backward formulas without a device.

There is no environment switch: tools and tests turn the native route off (or wide open) by replacing `native_ok` or
the two routing constants."""
from __future__ import annotations

import types

import torch
from torch.autograd.function import once_differentiable

from .. import kernels as K

impl = types.SimpleNamespace(eigh=K.eigh)


def _sym(M: torch.Tensor) -> torch.Tensor:
    return 0.5 * (M + M.mT)


class NativeEigh(torch.autograd.Function):
    """(evals, evecs) = eigh(A), lower triangle read.  Backward, the Hermitian case of ATen's pull-back:
    A_bar = sym(Q (diag(l_bar) + F o (Q^T Q_bar)) Q^T), F_ij = 1 / (l_j - l_i) off the diagonal and 0 on it.  Exactly
    repeated eigenvalues divide by zero, as they do in ATen; a failed member (NaN outputs) has a NaN gradient."""

    @staticmethod
    def forward(ctx, A):
        evals, evecs, _info = impl.eigh(A, want_vectors=True)
        ctx.save_for_backward(evals, evecs)
        return evals, evecs

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_evals, grad_evecs):
        evals, Q = ctx.saved_tensors
        if grad_evecs is None:
            inner = torch.diag_embed(grad_evals)
        else:
            gap = evals.unsqueeze(-2) - evals.unsqueeze(-1)  # [i, j] = l_j - l_i
            gap.diagonal(dim1=-2, dim2=-1).fill_(1.0)
            inner = (Q.mT @ grad_evecs) / gap
            diag = inner.diagonal(dim1=-2, dim2=-1)
            if grad_evals is None:
                diag.zero_()
            else:
                diag.copy_(grad_evals)
        return _sym(Q @ inner @ Q.mT)


class NativeEigvalsh(torch.autograd.Function):
    """evals = eigvalsh(A) when a gradient is required: the vectors are computed for A_bar = sym(Q diag(l_bar) Q^T)."""

    @staticmethod
    def forward(ctx, A):
        evals, evecs, _info = impl.eigh(A, want_vectors=True)
        ctx.save_for_backward(evecs)
        return evals

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_evals):
        (Q,) = ctx.saved_tensors
        return _sym((Q * grad_evals.unsqueeze(-2)) @ Q.mT)


# The routing constants: only shapes measured faster than ATen's float64 eigh on the same device in the same run are
# native (tools/mb_eigh.py on one MI355X; microseconds, native against ATen).
# N = 8, 16 and 32 win at every measured batch, with vectors and without: eigh 64 x 8^2 63 against 508, 16 x 16^2 174
# against 804, 1 / 16 / 256 x 32^2 475 / 529 / 512 against 819 / 2285 / 25728; eigvalsh 1.2 to 3.2 times faster.  At N = 64
# the single matrix loses (1780 against 1630) and eigenvalues-only loses up to a batch of 16 (1718 against 1023); from
# N = 128 on every measured shape loses (256 x 256^2: 22.8 against 19.1 ms; 16 x 1024^2: 509 against 39 ms).
EIGH_NATIVE_MAX_N = 32
# the single matrix of 32 rows already wins (475 against 819): no batch threshold below EIGH_NATIVE_MAX_N
EIGH_NATIVE_MIN_BATCH = 1


def native_ok(A: torch.Tensor) -> bool:
    """The routing predicate: a float64 HIP tensor of square matrices with 1 <= N <= EIGH_NATIVE_MAX_N and a flattened
    batch of at least EIGH_NATIVE_MIN_BATCH goes to csrc/lo_eigh_f64.hip; everything else (CPU, float32 under
    `linalg_dtypes(symeig=torch.float)`, larger N, smaller batches) keeps the ATen call."""
    if not (torch.is_tensor(A) and A.is_cuda and A.dtype == torch.float64 and A.dim() >= 2
            and A.shape[-1] == A.shape[-2]):
        return False
    return 1 <= A.shape[-1] <= min(EIGH_NATIVE_MAX_N, K.EIGH_MAX_N) and A.shape[:-2].numel() >= EIGH_NATIVE_MIN_BATCH


def eigh(A: torch.Tensor):
    """(evals, evecs) of symmetric matrices: NativeEigh where `native_ok`, torch.linalg.eigh unchanged otherwise."""
    if native_ok(A):
        return NativeEigh.apply(A)
    return torch.linalg.eigh(A)


def eigvalsh(A: torch.Tensor) -> torch.Tensor:
    """Eigenvalues of symmetric matrices: native where `native_ok` (without vector work unless a gradient is
    required), torch.linalg.eigvalsh unchanged otherwise."""
    if native_ok(A):
        if A.requires_grad and torch.is_grad_enabled():
            return NativeEigvalsh.apply(A)
        return impl.eigh(A.detach(), want_vectors=False)[0]
    return torch.linalg.eigvalsh(A)


__all__ = ["NativeEigh", "NativeEigvalsh", "native_ok", "eigh", "eigvalsh", "impl", "EIGH_NATIVE_MAX_N",
           "EIGH_NATIVE_MIN_BATCH"]
