"""The float64 matrix-free kernel operator without a GPU (ABI 31): the binding and the exports of the six entry points,
the gate `_native_f64_refusal`, kernel_theta in float64, the fp32 fusion gates that must keep float64 operators out, and
the longdouble helpers of tests/kernel_f64_cases.py -- the truth of tests/test_gpu_kernel_f64.py -- against float64
autograd of the covariance functions."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import kernel_f64_cases as T  # noqa: E402
from make_golden_kernel_f64 import CASES, inputs  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import KernelLinearOperator  # noqa: E402
from linear_operator_amd.operators.sum_linear_operator import _kernel_groups  # noqa: E402

NB = {"outputscale": 0}
NEW = ("lo_kernel_mv_f64", "lo_kernel_mv_f64_workspace_bytes", "lo_kernel_bilinear_f64",
       "lo_kernel_bilinear_f64_workspace_bytes", "lo_kernel_points_grad_f64", "lo_kernel_points_grad_f64_workspace_bytes")


def op_of(fn, N=9, D=3, dtype=torch.float64, ls_shape=None, ls_dtype=None, **extra):
    g = torch.Generator().manual_seed(3100 + D)
    x = torch.rand(N, D, generator=g, dtype=dtype)
    ls = 0.5 + torch.rand(ls_shape or (1, D), generator=g, dtype=ls_dtype or dtype)
    return KernelLinearOperator(x, x, fn, num_nonbatch_dimensions=NB, lengthscale=ls,
                                outputscale=torch.tensor(1.3, dtype=dtype), **extra)


def test_binding_of_abi_31():
    assert _hip.ABI_VERSION >= 31
    for name in NEW:
        assert name in _hip._PROTOTYPES and name in _hip.EXPORTS, name
    assert len(_hip._PROTOTYPES["lo_kernel_mv_f64"][1]) == 16
    assert len(_hip._PROTOTYPES["lo_kernel_bilinear_f64"][1]) == 15
    assert len(_hip._PROTOTYPES["lo_kernel_points_grad_f64"][1]) == 15
    raw = ctypes.CDLL(_hip.lib_path())
    for name in NEW:
        assert hasattr(raw, name), f"liblo_amd.so does not export {name}"
    lib = _hip.load()
    assert lib.lo_abi_version() == _hip.ABI_VERSION
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "lo_amd.h")).read()
    for name in NEW:
        assert name + "(" in hdr
    # the sizers are host code: what the kernels take, what they do not
    assert lib.lo_kernel_mv_f64_workspace_bytes(1, 1013, 1013, 8, 1) > lib.lo_kernel_mv_workspace_bytes(1, 1013, 1013, 8, 1)
    assert lib.lo_kernel_mv_f64_workspace_bytes(1, 10, 10, 33, 1) == 0
    assert lib.lo_kernel_mv_f64_workspace_bytes(0, 1, 1, 1, 1) == 0
    assert lib.lo_kernel_bilinear_f64_workspace_bytes(2, 77, 130, 32, 3) > 0
    assert lib.lo_kernel_bilinear_f64_workspace_bytes(2, 77, 130, 33, 3) == 0
    assert lib.lo_kernel_points_grad_f64_workspace_bytes(1, 257, 257, 3, 8) > 0
    assert lib.lo_kernel_points_grad_f64_workspace_bytes(1, 257, 257, 0, 8) == 0


def test_routing_tables_hold_the_kernel_kind():
    assert K._F64_KIND_NAMES[_hip.LO_OP_KERNEL_DIAG] == "kernel"
    assert K._NATIVE_MATMUL_F64[("kernel", 1)] is True and K._NATIVE_MATMUL_F64[("kernel", 2)] is True
    from linear_operator_amd.utils.linear_cg import _F64_KINDS

    assert _hip.LO_OP_KERNEL_DIAG in _F64_KINDS
    assert K._f64_route_kind(op_of(covariance.rbf)) == "kernel"
    assert K._f64_route_kind(op_of(covariance.rbf, dtype=torch.float32)) is None


@pytest.mark.parametrize("name", list(covariance.FAMILIES))
def test_the_float64_gate_takes_the_four_families(name):
    op = op_of(covariance.FAMILIES[name])
    assert op._native_f64_refusal(check_device=False) is None
    assert op._native_f64_refusal() == "not on the device" and not op._is_native_f64()
    assert op._native_refusal(check_device=False) == "not float32"  # (the fp32 gate and what relies on it do not move)
    shared = op_of(covariance.FAMILIES[name], ls_shape=(1, 1))
    assert shared._native_f64_refusal(check_device=False) is None


def test_the_float64_gate_names_its_reason():
    refusal = lambda op: op._native_f64_refusal(check_device=False)  # noqa: E731
    assert refusal(op_of(covariance.rbf, dtype=torch.float32)) == "not float64"
    g = op_of(covariance.rbf_grad)
    assert refusal(KernelLinearOperator(g.x1, g.x2, covariance.rbf_grad, num_outputs_per_input=(4, 4),
                                        num_nonbatch_dimensions=NB, **g.tensor_params)) == "more than one output per input"
    assert "beyond LO_KERNEL_MAX_DIM" in refusal(op_of(covariance.rbf, D=33))
    assert refusal(op_of(covariance.rbf, period=2.0)) == "parameters other than lengthscale and outputscale"
    assert refusal(op_of(covariance.rbf, extra=torch.ones(1, 1, dtype=torch.float64))) == \
        "parameters other than lengthscale and outputscale"
    assert refusal(op_of(covariance.rbf, ls_shape=(1, 2))).startswith("lengthscale of shape")
    assert refusal(op_of(covariance.rbf, ls_dtype=torch.float32)) == "not float64"
    assert refusal(op_of(lambda a, b, **kw: a @ b.mT)) == "covar_func has no native_family"


def test_outside_the_gate_nothing_changes_on_the_cpu():
    op = op_of(covariance.matern32)
    assert op._kernel_descriptor() is None and op._kernel_descriptor_f64() is None
    v = torch.randn(9, 2, dtype=torch.float64)
    ls, os_ = op.tensor_params["lengthscale"], op.tensor_params["outputscale"]
    assert torch.equal(op._matmul(v), covariance.matern32(op.x1, op.x2, ls, os_) @ v)
    assert torch.equal(op._diagonal(), os_.square().expand(9))


def test_kernel_theta_in_float64():
    g = torch.Generator().manual_seed(3111)
    ls = 0.5 + torch.rand(2, 1, 3, generator=g, dtype=torch.float64)
    os_ = 0.5 + torch.rand(2, generator=g, dtype=torch.float64)
    t64 = K.kernel_theta(ls, os_, (2,), 3, dtype=torch.float64)
    t32 = K.kernel_theta(ls, os_, (2,), 3)
    assert t64.dtype == torch.float64 and t32.dtype == torch.float32 and t64.shape == (2, 4)
    assert torch.equal(t64[:, :3], (1.0 / ls)[:, 0]) and torch.equal(t64[:, 3], os_.square())
    assert torch.allclose(t64, t32.double(), rtol=2.0 ** -23, atol=0)
    shared = K.kernel_theta(ls[..., :1], os_, (2,), 3, dtype=torch.float64)
    assert torch.equal(shared[:, :3], (1.0 / ls[:, 0, :1]).expand(2, 3))


def test_kernel_groups_do_not_group_float64_operators():
    a, b = op_of(covariance.rbf), op_of(covariance.matern52)
    b = KernelLinearOperator(a.x1, a.x1, covariance.matern52, num_nonbatch_dimensions=NB, **b.tensor_params)
    a = KernelLinearOperator(a.x1, a.x1, covariance.rbf, num_nonbatch_dimensions=NB, **a.tensor_params)
    items = _kernel_groups([a, b], check_device=False)
    assert items == [a, b] or (len(items) == 2 and items[0] is a and items[1] is b)


def test_mixed_dtypes_raise_before_the_library_is_asked():
    x = torch.rand(1, 5, 2, dtype=torch.float64)
    theta = torch.ones(1, 3, dtype=torch.float32)
    with pytest.raises(_hip.HipExtensionError, match="all be float32 or all be float64"):
        K.kernel_mv(x, x, theta, 0, torch.ones(1, 5, 1, dtype=torch.float64))
    with pytest.raises(_hip.HipExtensionError, match="all be float32 or all be float64"):
        K.kernel_bilinear(x, x, theta.double(), 0, torch.ones(1, 5, 1), torch.ones(1, 5, 1, dtype=torch.float64))
    with pytest.raises(_hip.HipExtensionError, match="all be float32 or all be float64"):
        K.kernel_points_grad(x.float(), x, theta.double(), 0, torch.ones(1, 5, 1).double(), torch.ones(1, 5, 1).double())
    with pytest.raises(_hip.HipExtensionError):
        K.kernel_diag_descriptor(x, theta, 0, dtype=torch.float64)


@pytest.mark.parametrize("ard", [True, False])
@pytest.mark.parametrize("name", list(covariance.FAMILIES))
def test_longdouble_helpers_equal_float64_autograd(name, ard):
    """The dense K and the analytic g_theta / g_x1 of the header, in longdouble, against float64 autograd of
    covariance.* on a 9 x 7 problem, to 1e-12: the truth of the GPU tests is itself tested."""
    assert np.finfo(np.longdouble).eps < 1e-18
    g = torch.Generator().manual_seed(3120)
    B, M, N, D, t = 2, 9, 7, 3, 2
    x1 = torch.rand(B, M, D, generator=g, dtype=torch.float64).requires_grad_(True)
    x2 = torch.rand(B, N, D, generator=g, dtype=torch.float64).requires_grad_(True)
    ls = (0.5 + torch.rand(B, 1, D if ard else 1, generator=g, dtype=torch.float64)).requires_grad_(True)
    os_ = (0.7 + torch.rand(B, generator=g, dtype=torch.float64)).requires_grad_(True)
    U = torch.randn(B, M, t, generator=g, dtype=torch.float64)
    V = torch.randn(B, N, t, generator=g, dtype=torch.float64)
    Kd = covariance.FAMILIES[name](x1, x2, ls, os_)
    (U * (Kd @ V)).sum().backward()
    n = lambda a: a.detach().numpy()  # noqa: E731
    theta = n(K.kernel_theta(ls, os_, (B,), D, dtype=torch.float64))
    assert T.rel(T.dense_ld(name, n(x1), n(x2), theta), n(Kd)) <= 1e-12
    assert T.rel(T.dense_ld(name, n(x1), n(x2), T.theta_ld(n(ls), n(os_), B, D)), n(Kd)) <= 1e-12
    gt = T.g_theta_ld(name, n(x1), n(x2), theta, n(U), n(V))
    d_ls, d_os = T.theta_to_params(theta, gt, ard)
    assert T.rel(d_ls, n(ls.grad)) <= 1e-12 and T.rel(d_os, n(os_.grad)) <= 1e-12
    assert T.rel(T.g_x1_ld(name, n(x1), n(x2), theta, n(U), n(V)), n(x1.grad)) <= 1e-12
    assert T.rel(T.g_x1_ld(name, n(x2), n(x1), theta, n(V), n(U)), n(x2.grad)) <= 1e-12


def test_longdouble_helpers_at_coincident_points():
    """r = 0 off the diagonal: K is outputscale^2 there, Matern-1/2 adds nothing to the derivatives, the others are finite."""
    x = np.array([[[0.1, 0.2], [0.1, 0.2], [0.4, 0.9]]])
    theta = np.array([[1.5, 0.7, 1.3]])
    U = V = np.ones((1, 3, 1))
    for name in covariance.FAMILIES:
        Kd = T.dense_ld(name, x, x, theta)
        assert Kd[0, 0, 1] == T.LD(1.3) and np.isfinite(Kd.astype(np.float64)).all()
        assert np.isfinite(T.g_theta_ld(name, x, x, theta, U, V).astype(np.float64)).all()
        assert np.isfinite(T.g_x1_ld(name, x, x, theta, U, V).astype(np.float64)).all()


def test_goldens_are_in_place_and_their_inputs_are_float64():
    for p, (family, B, N, D, ard, _) in CASES.items():
        G = np.load(os.path.join(HERE, "golden", f"g42_kernel_f64_{p}.npz"))
        x = inputs(p)
        assert all(v.dtype == np.float64 for v in x.values())
        assert x["x"].shape == (B, N, D) and x["lengthscale"].shape == (B, 1, D if ard else 1)
        for q in ("mv", "diag", "solve", "iq", "ld", "L", "gl", "go", "gx"):
            assert G[q].dtype == np.float64 and G[q].shape == G[q + "_exact"].shape and float(G[q + "_err"]) >= 0
        assert G["piv"].shape == (B, 15)
        # the fixture's exact product is the longdouble one of the helpers on the same inputs
        theta = T.theta_ld(x["lengthscale"], x["outputscale"], B, D)
        want = T.dense_ld(family, x["x"], x["x"], theta) @ x["V"].astype(T.LD)
        assert T.rel(G["mv_exact"], want) <= 2.0 ** -52
