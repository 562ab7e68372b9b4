"""The float64 many-column derivatives of the matrix-free kernel operator on the MI355X: lo_kernel_bilinear_wide_f64 and
lo_kernel_points_grad_wide_f64 (csrc/lo_kernel_bil_wide_f64.hip: W = U V^T on v_mfma_f64_16x16x4_f64, two lane swaps, one
row per lane) against the numpy longdouble analytic values of tests/kernel_f64_cases.py.  The bound is the one of
tests/test_gpu_kernel_f64.py: at most REF_FACTOR = 4 times max(the error of float64 autograd through the dense covariance
function on the same inputs, 2^-52); every case prints its ratios."""
from unittest import mock

import pytest
import torch

from test_gpu_kernel_f64 import DEV, F64, T, autograd_all, dev, host, kernel_op, problem, rng, theta_of, within_bound

from linear_operator_amd import _hip
from linear_operator_amd import kernels as K
from linear_operator_amd.operators import KernelLinearOperator

pytestmark = pytest.mark.gpu

# (family, B, M, N, D, t, ARD, duplicated points).  Both sides are taken, so M and N change places in the second call.
# M: a 16-row tile (1, 15), live rows in exactly one, two or three 16-lane groups beside the first (17, 33, 49: the
# transpose), a wave (63, 65), a row block (257); N: a 16-point block (1, 2, 15, 17), the 128-point tile and js > 1 (127,
# 129, 257); t: a ragged contraction step of four (1, 3, 5, 15), a full sweep and one past it for 16, 28, 48 and 52 columns
# (16, 17, 33, 65); every family meets every padded dimension.
CASES = [
    ("rbf", 1, 1, 2, 1, 1, False, False), ("rbf", 3, 15, 127, 8, 15, True, False),
    ("rbf", 1, 257, 257, 16, 17, False, False), ("rbf", 1, 65, 129, 32, 33, True, False),
    ("rbf", 1, 17, 15, 3, 65, True, False), ("rbf", 1, 33, 17, 3, 5, False, False),
    ("rbf", 3, 130, 77, 3, 17, True, False),
    ("matern12", 1, 49, 129, 3, 65, True, False), ("matern12", 1, 257, 2, 8, 3, False, False),
    ("matern12", 3, 63, 129, 16, 16, True, False), ("matern12", 1, 1, 127, 17, 17, False, False),
    ("matern12", 1, 17, 257, 32, 33, True, False),
    ("matern32", 1, 65, 1, 1, 33, True, False), ("matern32", 1, 33, 15, 8, 65, False, False),
    ("matern32", 1, 15, 129, 16, 1, True, False), ("matern32", 1, 257, 257, 17, 15, False, False),
    ("matern32", 1, 49, 17, 3, 5, True, False),
    ("matern32", 512, 33, 129, 3, 17, True, False),  # B ceil(M / 256) = 512: no column split
    ("matern52", 1, 257, 127, 1, 33, False, False), ("matern52", 1, 65, 257, 16, 65, False, False),
    ("matern52", 3, 63, 2, 32, 3, True, False), ("matern52", 1, 77, 130, 8, 17, False, False),
    ("matern52", 1, 257, 257, 32, 65, True, False),
    ("rbf", 1, 130, 130, 3, 17, True, True), ("matern12", 1, 130, 130, 3, 17, True, True),
    ("matern32", 1, 130, 130, 3, 17, True, True), ("matern52", 1, 130, 130, 3, 17, True, True),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_wide_f64_derivatives_against_longdouble(case):
    name, B, M, N, D, t, ard, dup = case
    seed, fam = 9800 + 7 * CASES.index(case), T.FAMILY_CODES[name]
    x1, x2, ls, os_ = problem(seed, B, M, N, D, ard)
    if dup:  # coincident pairs: x2 holds the values of x1 (a tensor of its own), every second point repeats its neighbour
        x1[:, 1::2] = x1[:, 0::2]
        x2 = x1.copy()
    U, V = rng(seed + 1).standard_normal((B, M, t)), rng(seed + 2).standard_normal((B, N, t))
    theta = theta_of(ls, os_, B, D)
    th = host(theta)
    g1_ref, g2_ref, gl_ref, go_ref = autograd_all(name, x1, x2, ls, os_, U, V, False)
    t1, t2, tU, tV = dev(x1), dev(x2), dev(U), dev(V)
    if B == 512:
        assert _hip.load().lo_kernel_points_grad_wide_f64_workspace_bytes(B, M, N, D, t) == 256  # (the tail: no partials)
    g = K.kernel_bilinear_wide(t1, t2, theta, fam, tU, tV)
    p1 = K.kernel_points_grad_wide(t1, t2, theta, fam, tU, tV)
    p2 = K.kernel_points_grad_wide(t2, t1, theta, fam, tV, tU)
    assert g.dtype == F64 and tuple(g.shape) == (B, D + 1) and p1.dtype == F64 and tuple(p1.shape) == (B, M, D)
    d_ls, d_os = T.theta_to_params(th, T.g_theta_ld(name, x1, x2, th, U, V), ard)
    got_ls = -(theta[:, :D] ** 2) * g[:, :D]
    got_ls = (got_ls if ard else got_ls.sum(-1, keepdim=True))[:, None, :]
    label = "bil_wide " + "-".join(str(x) for x in case)
    within_bound("d lengthscale " + label, got_ls, d_ls, gl_ref)
    within_bound("d outputscale " + label, 2 * dev(os_) * g[:, D], d_os, go_ref)
    within_bound("d x1 " + label, p1, T.g_x1_ld(name, x1, x2, th, U, V), g1_ref)
    within_bound("d x2 " + label, p2, T.g_x1_ld(name, x2, x1, th, V, U), g2_ref)
    assert torch.equal(K.kernel_bilinear_wide(t1, t2, theta, fam, tU, tV), g)  # two calls give equal bits
    assert torch.equal(K.kernel_points_grad_wide(t1, t2, theta, fam, tU, tV), p1)


@pytest.mark.parametrize("stem", ["lo_kernel_bilinear", "lo_kernel_points_grad"])
def test_wide_f64_entry_points_return_the_error_codes_of_their_twins(stem):
    lib, p = _hip.load(), _hip.ptr
    B, M, N, D, t = 1, 300, 300, 3, 17
    x, theta = torch.rand(B, M, D, dtype=F64, device=DEV), torch.ones(B, D + 1, dtype=F64, device=DEV)
    U, V = torch.randn(B, M, t, dtype=F64, device=DEV), torch.randn(B, N, t, dtype=F64, device=DEV)
    g = torch.full((B, M, D), -7.0, dtype=F64, device=DEV)  # (room for either result)
    st = _hip.stream_ptr(U.device)
    need = getattr(lib, stem + "_wide_f64_workspace_bytes")(B, M, N, D, t)  # (> 256: a split member, partials)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)

    def both(x1=x, dim=D, w=ws, wb=need):
        a = (p(x1), p(x), p(theta), 0, B, M, N, dim, p(U), p(V), t, p(g), p(w), wb, st)
        codes = getattr(lib, stem + "_wide_f64")(*a), getattr(lib, stem + "_f64")(*a)
        assert codes[0] == codes[1], codes
        return codes[0]

    assert need > 256 and both(x1=None) == -1  # a null pointer
    assert both(dim=33) == _hip.LO_ERR_UNSUPPORTED
    assert both(wb=need - 1) == -3 and both(w=None, wb=0) == -3  # refused before anything is launched: g keeps its fill
    torch.cuda.synchronize()
    assert bool((g == -7.0).all()) and both() == 0


# what ko64_bil_wide (csrc/lo_kernel_shape.h) says at D = 3 after the measurement of DESIGN.md section 6za
ROUTED = {17: True, 4: False}


@pytest.mark.parametrize("t", [17, 4])
def test_the_f64_operator_takes_the_wide_derivatives_where_the_rule_says_so(t):
    B, M, N, D = 2, 130, 77, 3
    x1, x2, ls, os_ = problem(9790, B, M, N, D, True)
    tU, tV = dev(rng(9791).standard_normal((B, M, t))), dev(rng(9792).standard_normal((B, N, t)))
    theta = theta_of(ls, os_, B, D)
    leaves = [dev(a).requires_grad_(True) for a in (x1, x2, ls, os_)]
    with mock.patch.object(KernelLinearOperator, "_dense_covar", side_effect=AssertionError("dense evaluation")):
        grads = kernel_op("matern52", *leaves)._bilinear_derivative(tU, tV)
    bil, pts = ((K.kernel_bilinear_wide, K.kernel_points_grad_wide) if ROUTED[t]
                else (K.kernel_bilinear, K.kernel_points_grad))
    t1, t2 = leaves[0].detach(), leaves[1].detach()
    g = bil(t1, t2, theta, 3, tU, tV)
    assert torch.equal(grads[0], pts(t1, t2, theta, 3, tU, tV)) and torch.equal(grads[1], pts(t2, t1, theta, 3, tV, tU))
    assert torch.equal(grads[2], (-(theta[:, :D] ** 2) * g[:, :D]).reshape(B, 1, D))
    assert torch.equal(grads[3], 2.0 * dev(os_) * g[:, D])
