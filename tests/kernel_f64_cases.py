"""The truth of the float64 kernel-operator tests: the kernel matrix and the analytic derivatives of include/lo_amd.h in
numpy `longdouble` (64-bit mantissa on x86-64: 2^-63 against float64's 2^-52), on the float64 inputs themselves.
tests/test_kernel_f64_cpu.py checks these helpers against float64 autograd of linear_operator_amd.covariance, so the
truth of tests/test_gpu_kernel_f64.py is itself tested; tests/golden/make_golden_kernel_f64.py uses them for its exact
values.

    K_ij = theta[D] g(r_ij),  r_ij^2 = sum_d (theta[d] x1[i, d] - theta[d] x2[j, d])^2   (points scaled, then differenced)
    g_theta[d]  = sum_ij W_ij theta[D] h(r_ij) (theta[d] delta_ijd)^2 / theta[d]  (d < D),  g_theta[D] = sum_ij W_ij g(r_ij)
    g_x1[i, d]  = theta[D] theta[d] sum_j W_ij h(r_ij) theta[d] delta_ijd,   h = g'(r) / r,  W = U V^T
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
FAMILY_CODES = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3}
R2_FLOOR = LD(1e-30)  # covariance._R2_FLOOR: a closer pair adds nothing to the Matern-1/2 derivatives
FLOOR = 2.0 ** -52  # a reference error below this is taken as this
REF_FACTOR = 4.0


def rel(a, b):
    """Relative error of a against b over the whole array (Frobenius), in longdouble."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    nb = np.sqrt((b * b).sum())
    return float(np.sqrt(((a - b) ** 2).sum()) / (nb if nb > 0 else LD(1)))


def _diffs(x1, x2, inv):
    """Scaled differences one coordinate at a time: yields (d, delta [B, M, N]) in longdouble; inv [B, D]."""
    x1, x2, inv = (np.asarray(a, dtype=LD) for a in (x1, x2, inv))
    for d in range(x1.shape[-1]):
        a = x1[:, :, d] * inv[:, None, d]
        b = x2[:, :, d] * inv[:, None, d]
        yield d, a[:, :, None] - b[:, None, :]


def sq_dist_ld(x1, x2, inv):
    r2 = LD(0)
    for _, df in _diffs(x1, x2, inv):
        r2 = r2 + df * df
    return r2


def g_h_ld(family, r2):
    """(g(r), h(r) = g'(r) / r) [..] in longdouble from r^2; h of Matern-1/2 is 0 for r^2 <= R2_FLOOR."""
    r2 = np.asarray(r2, dtype=LD)
    if family == "rbf":
        e = np.exp(-r2 / 2)
        return e, -e
    r = np.sqrt(r2)
    if family == "matern12":
        e = np.exp(-r)
        safe = np.where(r2 > R2_FLOOR, r, LD(1))
        return e, np.where(r2 > R2_FLOOR, -e / safe, LD(0))
    if family == "matern32":
        s3 = np.sqrt(LD(3))
        e = np.exp(-s3 * r)
        return (1 + s3 * r) * e, -3 * e
    s5 = np.sqrt(LD(5))
    e = np.exp(-s5 * r)
    return (1 + s5 * r + LD(5) / 3 * r2) * e, -(LD(5) / 3) * (1 + s5 * r) * e


def dense_ld(family, x1, x2, theta):
    """K [B, M, N] in longdouble; x1 [B, M, D], x2 [B, N, D], theta [B, D + 1] (inverse lengthscales, outputscale^2)."""
    theta = np.asarray(theta, dtype=LD)
    D = x1.shape[-1]
    g, _ = g_h_ld(family, sq_dist_ld(x1, x2, theta[:, :D]))
    return theta[:, D, None, None] * g


def theta_ld(lengthscale, outputscale, B, D):
    """theta [B, D + 1] in longdouble from the operator's parameters (1 / l in longdouble: the operator's definition)."""
    inv = np.broadcast_to(1 / np.asarray(lengthscale, dtype=LD).reshape(-1, np.shape(lengthscale)[-1]), (B, D))
    os2 = np.broadcast_to(np.asarray(outputscale, dtype=LD).reshape(-1) ** 2, (B,))
    return np.concatenate((inv, os2[:, None]), -1)


def g_theta_ld(family, x1, x2, theta, U, V):
    """g_theta [B, D + 1] of lo_kernel_bilinear_*: d / d theta of sum_s u_s^T K v_s."""
    theta = np.asarray(theta, dtype=LD)
    B, _, D = x1.shape
    W = np.einsum("bis,bjs->bij", np.asarray(U, dtype=LD), np.asarray(V, dtype=LD))
    g, h = g_h_ld(family, sq_dist_ld(x1, x2, theta[:, :D]))
    out = np.zeros((B, D + 1), dtype=LD)
    for d, df in _diffs(x1, x2, theta[:, :D]):
        out[:, d] = theta[:, D] * (W * h * df * df).sum((1, 2)) / theta[:, d]
    out[:, D] = (W * g).sum((1, 2))
    return out


def g_x1_ld(family, x1, x2, theta, U, V):
    """g_x1 [B, M, D] of lo_kernel_points_grad_*: d / d x1 of sum_s u_s^T K v_s, x2 held fixed."""
    theta = np.asarray(theta, dtype=LD)
    B, M, D = x1.shape
    W = np.einsum("bis,bjs->bij", np.asarray(U, dtype=LD), np.asarray(V, dtype=LD))
    _, h = g_h_ld(family, sq_dist_ld(x1, x2, theta[:, :D]))
    out = np.zeros((B, M, D), dtype=LD)
    for d, df in _diffs(x1, x2, theta[:, :D]):
        out[:, :, d] = (theta[:, D] * theta[:, d])[:, None] * (W * h * df).sum(2)
    return out


def theta_to_params(theta, g_theta, ard: bool):
    """(d / d lengthscale [B, 1, D or 1], d / d outputscale [B]) from d / d theta: theta_d = 1 / l_d, theta_D = os^2."""
    theta, g_theta = np.asarray(theta, dtype=LD), np.asarray(g_theta, dtype=LD)
    D = theta.shape[-1] - 1
    d_ls = -(theta[:, :D] ** 2) * g_theta[:, :D]
    if not ard:
        d_ls = d_ls.sum(-1, keepdims=True)
    return d_ls[:, None, :], 2 * np.sqrt(theta[:, D]) * g_theta[:, D]
