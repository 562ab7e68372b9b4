"""Stationary covariance families for KernelLinearOperator: plain, differentiable torch functions with the calling
convention `f(x1, x2, lengthscale, outputscale)` (the `covar_func` of the reference's KernelLinearOperator).

    x1 [..., M, D], x2 [..., N, D], lengthscale [..., 1, D] (ARD) or [..., 1, 1] (shared), outputscale [...]
    (pass num_nonbatch_dimensions={"outputscale": 0} to the operator)

    k(x1_i, x2_j) = outputscale^2 g(r),   r = |(x1_i - x2_j) / lengthscale|

    rbf       g(r) = exp(-r^2 / 2)
    matern12  g(r) = exp(-r)
    matern32  g(r) = (1 + sqrt(3) r) exp(-sqrt(3) r)
    matern52  g(r) = (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)

r^2 is the sum of squared direct differences of the scaled points (no |a|^2 + |b|^2 - 2 a.b, which cancels for near
points).  Each function carries `native_family`, the LO_KERNEL_* code under which csrc/lo_kernel_op.hip evaluates the
same formula tile by tile; on that path the [..., M, N] matrix these functions return is never formed.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _hip

# below this r^2 a pair counts as coincident: the square root's derivative is cut off, so the pair adds nothing to the
# gradients (the Matern families are not differentiable in r at 0; in the hyperparameters their derivative there is 0)
_R2_FLOOR = 1e-30


def scaled_sq_dist(x1: Tensor, x2: Tensor, lengthscale: Tensor) -> Tensor:
    """r^2 [..., M, N] = sum_d ((x1[i, d] - x2[j, d]) / lengthscale[d])^2, points scaled first, then differenced."""
    a = (x1 / lengthscale).unsqueeze(-2)  # [..., M, 1, D]
    b = (x2 / lengthscale).unsqueeze(-3)  # [..., 1, N, D]
    return (a - b).square().sum(-1)


def _scale(outputscale: Tensor) -> Tensor:
    return outputscale.square()[..., None, None]


def _dist(r2: Tensor) -> Tensor:
    return r2.clamp_min(_R2_FLOOR).sqrt()


def rbf(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor) -> Tensor:
    return _scale(outputscale) * torch.exp(-0.5 * scaled_sq_dist(x1, x2, lengthscale))


def matern12(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor) -> Tensor:
    return _scale(outputscale) * torch.exp(-_dist(scaled_sq_dist(x1, x2, lengthscale)))


def matern32(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor) -> Tensor:
    s = math.sqrt(3.0) * _dist(scaled_sq_dist(x1, x2, lengthscale))
    return _scale(outputscale) * ((1.0 + s) * torch.exp(-s))


def matern52(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor) -> Tensor:
    r2 = scaled_sq_dist(x1, x2, lengthscale)
    s = math.sqrt(5.0) * _dist(r2)
    return _scale(outputscale) * ((1.0 + s + (5.0 / 3.0) * r2) * torch.exp(-s))


rbf.native_family = _hip.LO_KERNEL_RBF
matern12.native_family = _hip.LO_KERNEL_MATERN12
matern32.native_family = _hip.LO_KERNEL_MATERN32
matern52.native_family = _hip.LO_KERNEL_MATERN52

FAMILIES = {"rbf": rbf, "matern12": matern12, "matern32": matern32, "matern52": matern52}

__all__ = ["rbf", "matern12", "matern32", "matern52", "scaled_sq_dist", "FAMILIES"]
