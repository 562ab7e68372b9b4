"""Stationary covariance families for KernelLinearOperator: plain, differentiable torch functions with the calling
convention `f(x1, x2, lengthscale, outputscale)` (the `covar_func` of the reference's KernelLinearOperator).

    x1 [..., M, D], x2 [..., N, D], lengthscale [..., 1, D] (ARD) or [..., 1, 1] (shared), outputscale [...]
    (pass num_nonbatch_dimensions={"outputscale": 0} to the operator)

    k(x1_i, x2_j) = outputscale^2 g(r),   r = |(x1_i - x2_j) / lengthscale|

    rbf       g(r) = exp(-r^2 / 2)
    matern12  g(r) = exp(-r)
    matern32  g(r) = (1 + sqrt(3) r) exp(-sqrt(3) r)
    matern52  g(r) = (1 + sqrt(5) r + 5 r^2 / 3) exp(-sqrt(5) r)

    rbf_grad  the covariance of the values AND the D partial derivatives of an RBF GP (a GP with derivative
              observations; GPyTorch's RBFKernelGrad): D + 1 outputs per input, [..., M (D + 1), N (D + 1)], row index
              i (D + 1) + a with a = 0 the value and a = 1 .. D the derivative in coordinate a - 1.  With
              t = 1 / lengthscale, u = t (x1_i - x2_j), e = exp(-|u|^2 / 2) the block of the pair (i, j) is
                  K[0,0] = os^2 e            K[0,b] = os^2 t_b u_b e
                  K[a,0] = -os^2 t_a u_a e   K[a,b] = os^2 t_a t_b (delta_ab - u_a u_b) e
              (pass num_outputs_per_input=(D + 1, D + 1) to the operator)

    *_task    rbf_task, matern12_task, matern32_task, matern52_task: the task-indexed ("Hadamard") multitask kernel,
              `f(x1, x2, lengthscale, outputscale, task_covar)`.  x [..., N, D + 1]: columns 0 .. D - 1 the coordinates,
              column D the task id of the observation, an integer 0 .. T - 1 stored as a float; lengthscale [..., 1, D]
              or [..., 1, 1] over the coordinates; task_covar [..., T, T]:
                  k(x1_i, x2_j) = outputscale^2 g(r_ij) task_covar[t_i, t_j]
              One output per input; the gradient with respect to the task column is zero, as autograd gives it.

    rq        `f(x1, x2, lengthscale, outputscale, alpha)`, alpha [...] > 0, the rational quadratic kernel
                  k = outputscale^2 (1 + r^2 / (2 alpha))^(-alpha),  r as above (alpha -> inf: rbf)
    periodic  `f(x1, x2, lengthscale, outputscale, period_length)`, period_length [..., 1, D] or [..., 1, 1]:
                  phi_k = x1_k / p_k - x2_k / p_k   (scaled first, then differenced)
                  k = outputscale^2 exp(-2 sum_k (sin(pi phi_k) / l_k)^2)
              Both: one output per input, pass num_nonbatch_dimensions={"outputscale": 0, "alpha": 0}.  They carry
              `native_outputs = "param"` and the codes LO_KERNEL_RQ / LO_KERNEL_PERIODIC, which lie outside the codes of
              the families above on purpose: csrc/lo_kernel_param.hip has entry points and a kind of its own.

    spectral_mixture  `f(x1, x2, mixture_weights, mixture_means, mixture_scales)`, GPyTorch's SpectralMixtureKernel:
              mixture_weights [..., Q], mixture_means and mixture_scales [..., Q, D] (GPyTorch keeps the means and scales as
              [Q, 1, D]: squeeze the 1), no lengthscale and no outputscale:
                  tau = x1_i - x2_j   (differenced first, then multiplied by mu or sigma: in float32 the difference of
                                       near points is exact and the phase error is |mu tau| eps, not |mu x| eps)
                  k = sum_q w_q exp(-2 pi^2 sum_k (sigma_qk tau_k)^2) prod_k cos(2 pi mu_qk tau_k)
              One output per input, pass num_nonbatch_dimensions={"mixture_weights": 1}.  It carries
              `native_outputs = "sm"` and NO native_family: csrc/lo_kernel_sm.hip has entry points and a kind of its own,
              and every gate that asks for a family refuses it.  The diagonal is sum_q w_q.

r^2 is the sum of squared direct differences of the scaled points (no |a|^2 + |b|^2 - 2 a.b, which cancels for near
points).  Each function carries `native_family`, the LO_KERNEL_* code under which csrc/lo_kernel_op.hip evaluates the
same formula tile by tile; on that path the [..., M, N] matrix these functions return is never formed.  rbf_grad
carries `native_outputs = "grad"` besides: csrc/lo_kernel_grad.hip forms its blocks pair by pair.
The *_task functions carry the base family's code and `native_outputs = "task"`: csrc/lo_kernel_task.hip stages the ids
with the points and reads one word of task_covar per pair.
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


def rbf_grad(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor) -> Tensor:
    D = x1.shape[-1]
    u = (x1 / lengthscale).unsqueeze(-2) - (x2 / lengthscale).unsqueeze(-3)  # [..., M, N, D], scaled, then differenced
    e = _scale(outputscale) * torch.exp(-0.5 * u.square().sum(-1))  # [..., M, N]
    theta = (1.0 / lengthscale).expand(*lengthscale.shape[:-1], D)  # [..., 1, D]
    tu = theta.unsqueeze(-3) * u  # t_b u_b
    inner = torch.diag_embed(theta.square()).unsqueeze(-3) - tu.unsqueeze(-1) * tu.unsqueeze(-2)  # [..., M, N, D, D]
    top = torch.cat((torch.ones_like(tu[..., :1]), tu), -1).unsqueeze(-2)  # [..., M, N, 1, D + 1]
    block = torch.cat((top, torch.cat((-tu.unsqueeze(-1), inner.expand(*tu.shape, D)), -1)), -2)
    K = e[..., None, None] * block  # [..., M, N, D + 1, D + 1]
    M, N = K.shape[-4:-2]
    return K.transpose(-3, -2).reshape(*K.shape[:-4], M * (D + 1), N * (D + 1))


def _task_gather(x1: Tensor, x2: Tensor, task_covar: Tensor) -> Tensor:
    """task_covar[t_i, t_j] [..., M, N] for the ids in the last columns of x1 and x2."""
    t1, t2 = x1[..., -1].long(), x2[..., -1].long()
    T = task_covar.shape[-1]
    batch = torch.broadcast_shapes(t1.shape[:-1], t2.shape[:-1], task_covar.shape[:-2])
    M, N = t1.shape[-1], t2.shape[-1]
    rows = task_covar.expand(*batch, T, T).gather(-2, t1.expand(*batch, M).unsqueeze(-1).expand(*batch, M, T))
    return rows.gather(-1, t2.expand(*batch, N).unsqueeze(-2).expand(*batch, M, N))


def rbf_task(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor, task_covar: Tensor) -> Tensor:
    return rbf(x1[..., :-1], x2[..., :-1], lengthscale, outputscale) * _task_gather(x1, x2, task_covar)


def matern12_task(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor, task_covar: Tensor) -> Tensor:
    return matern12(x1[..., :-1], x2[..., :-1], lengthscale, outputscale) * _task_gather(x1, x2, task_covar)


def matern32_task(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor, task_covar: Tensor) -> Tensor:
    return matern32(x1[..., :-1], x2[..., :-1], lengthscale, outputscale) * _task_gather(x1, x2, task_covar)


def matern52_task(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor, task_covar: Tensor) -> Tensor:
    return matern52(x1[..., :-1], x2[..., :-1], lengthscale, outputscale) * _task_gather(x1, x2, task_covar)


def rq(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor, alpha: Tensor) -> Tensor:
    a = alpha[..., None, None]
    q = scaled_sq_dist(x1, x2, lengthscale) / (2.0 * a)
    return _scale(outputscale) * (1.0 + q).pow(-a)


def periodic(x1: Tensor, x2: Tensor, lengthscale: Tensor, outputscale: Tensor, period_length: Tensor) -> Tensor:
    phi = (x1 / period_length).unsqueeze(-2) - (x2 / period_length).unsqueeze(-3)  # [..., M, N, D]
    s = torch.sin(math.pi * phi) / lengthscale.unsqueeze(-3)
    return _scale(outputscale) * torch.exp(-2.0 * s.square().sum(-1))


def spectral_mixture(x1: Tensor, x2: Tensor, mixture_weights: Tensor, mixture_means: Tensor,
                     mixture_scales: Tensor) -> Tensor:
    tau = (x1.unsqueeze(-2) - x2.unsqueeze(-3)).unsqueeze(-4)  # [..., 1, M, N, D]
    mu, sg = mixture_means[..., :, None, None, :], mixture_scales[..., :, None, None, :]  # [..., Q, 1, 1, D]
    env = torch.exp((-2.0 * math.pi ** 2) * (sg * tau).square().sum(-1))
    osc = torch.cos((2.0 * math.pi) * (mu * tau)).prod(-1)
    return (mixture_weights[..., :, None, None] * env * osc).sum(-3)


rbf.native_family = _hip.LO_KERNEL_RBF
rbf_grad.native_family = _hip.LO_KERNEL_RBF
rbf_grad.native_outputs = "grad"
matern12.native_family = _hip.LO_KERNEL_MATERN12
matern32.native_family = _hip.LO_KERNEL_MATERN32
matern52.native_family = _hip.LO_KERNEL_MATERN52

for _f, _base in ((rbf_task, rbf), (matern12_task, matern12), (matern32_task, matern32), (matern52_task, matern52)):
    _f.native_family = _base.native_family
    _f.native_outputs = "task"

rq.native_family = _hip.LO_KERNEL_RQ
periodic.native_family = _hip.LO_KERNEL_PERIODIC
rq.native_outputs = periodic.native_outputs = "param"

spectral_mixture.native_outputs = "sm"  # (and no native_family)

FAMILIES = {"rbf": rbf, "matern12": matern12, "matern32": matern32, "matern52": matern52}
# gradient kernels (D + 1 outputs per input): kept apart, FAMILIES holds the one-output families only
GRAD_FAMILIES = {"rbf_grad": rbf_grad}

# task-indexed multitask kernels (one more parameter, task_covar): kept apart as well
TASK_FAMILIES = {"rbf_task": rbf_task, "matern12_task": matern12_task, "matern32_task": matern32_task,
                 "matern52_task": matern52_task}

# families with a shape parameter (alpha, period_length): kept apart as well, with codes outside those of FAMILIES
PARAM_FAMILIES = {"rq": rq, "periodic": periodic}

# mixtures of products over the dimensions (no lengthscale, no outputscale, no family code): kept apart as well
MIXTURE_FAMILIES = {"spectral_mixture": spectral_mixture}

__all__ = ["rbf", "matern12", "matern32", "matern52", "rbf_grad", "rbf_task", "matern12_task", "matern32_task",
           "matern52_task", "rq", "periodic", "spectral_mixture", "scaled_sq_dist", "FAMILIES", "GRAD_FAMILIES",
           "TASK_FAMILIES", "PARAM_FAMILIES", "MIXTURE_FAMILIES"]
