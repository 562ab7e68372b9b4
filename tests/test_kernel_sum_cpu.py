"""Sums of KernelLinearOperators without a GPU: the binding of ABI 28 (symbols, constants, the host-side sizers), the
packing of the families and the layout of theta, the grouping rules of SumLinearOperator's lowering (decided on CPU tensors
through the `check_device=False` gate) and the CPU algebra of a sum of kernel operators against the dense sum and the
reference's goldens (tests/golden/g39_kernel_sum_*.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_sum import CASES, ERR_FLOOR, inputs, rel  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator, RootLinearOperator, SumLinearOperator)
from linear_operator_amd.operators import sum_linear_operator as slo  # noqa: E402

REF_FACTOR = 4.0
NB = {"outputscale": 0}


def kernel(x, name, D=None, x2=None, ls=None):
    D = x.shape[-1] if D is None else D
    ls = torch.full((1, D), 0.6) if ls is None else ls
    return KernelLinearOperator(x, x if x2 is None else x2, covariance.FAMILIES[name], num_nonbatch_dimensions=NB,
                                lengthscale=ls, outputscale=torch.tensor(1.1))


def shapes(items):
    return [len(i) if isinstance(i, list) else type(i).__name__ for i in items]


def test_binding_of_abi_28():
    assert _hip.ABI_VERSION >= 28 and _hip.LO_OP_KERNEL_SUM_DIAG == 12 and _hip.LO_KERNEL_MAX_TERMS == 4
    names = ("lo_kernel_sum_mv", "lo_kernel_sum_bilinear", "lo_kernel_sum_points_grad")
    for name in names:
        assert name + "_workspace_bytes" in _hip.EXPORTS and name + "_f32" in _hip.EXPORTS
        assert len(_hip._PROTOTYPES[name + "_workspace_bytes"][1]) == 6
    assert len(_hip._PROTOTYPES["lo_kernel_sum_mv_f32"][1]) == 17
    assert len(_hip._PROTOTYPES["lo_kernel_sum_bilinear_f32"][1]) == 16
    assert len(_hip._PROTOTYPES["lo_kernel_sum_points_grad_f32"][1]) == 16
    for fn in ("kernel_sum_theta", "kernel_sum_diag_descriptor", "kernel_sum_mv", "kernel_sum_bilinear",
               "kernel_sum_points_grad"):
        assert callable(getattr(K, fn))
    lib = _hip.load()  # (the sizers are host code)
    assert lib.lo_abi_version() >= 28
    assert lib.lo_kernel_sum_mv_workspace_bytes(1, 1013, 1013, 8, 3, 1) > 256  # (a split member: partials)
    assert lib.lo_kernel_sum_mv_workspace_bytes(128, 1024, 300, 1, 2, 17) == 256  # (no split, fused: the tail alone)
    # a narrow product runs term by term: one more vector for the terms beyond the first (none for a single term)
    assert lib.lo_kernel_sum_mv_workspace_bytes(128, 1024, 300, 1, 2, 1) == 256 + 4 * 128 * 1024
    assert lib.lo_kernel_sum_mv_workspace_bytes(128, 1024, 300, 1, 1, 1) == 256
    assert K.kernel_sum_fused_bilinear(3, 2) and not K.kernel_sum_fused_bilinear(8, 2)
    assert K.kernel_sum_fused_points_grad(3, 3) and not K.kernel_sum_fused_points_grad(3, 2)
    assert lib.lo_kernel_sum_mv_workspace_bytes(1, 10, 10, 33, 2, 1) == 0
    assert lib.lo_kernel_sum_mv_workspace_bytes(1, 10, 10, 3, 5, 1) == 0 and \
        lib.lo_kernel_sum_mv_workspace_bytes(1, 10, 10, 3, 0, 1) == 0
    # the derivative's partials grow with the number of terms, the other two workspaces do not
    one, four = (lib.lo_kernel_sum_bilinear_workspace_bytes(2, 77, 130, 8, T, 3) for T in (1, 4))
    assert four - 256 == 4 * (one - 256) > 0
    assert lib.lo_kernel_sum_points_grad_workspace_bytes(1, 300, 300, 3, 1, 2) == \
        lib.lo_kernel_sum_points_grad_workspace_bytes(1, 300, 300, 3, 4, 2) == \
        lib.lo_kernel_points_grad_workspace_bytes(1, 300, 300, 3, 2)
    assert lib.lo_kernel_sum_bilinear_workspace_bytes(2, 77, 130, 33, 2, 3) == 0


def test_family_packing_and_theta_layout():
    assert K.kernel_sum_pack_families([0]) == 0 and K.kernel_sum_pack_families([3, 0, 2, 1]) == 3 + (2 << 8) + (1 << 12)
    assert K.kernel_sum_pack_families([1, 2]) == 0x21
    for bad in ([], [0] * 5, [4], [0, -1]):
        with pytest.raises(ValueError):
            K.kernel_sum_pack_families(bad)
    B, D = 3, 4
    ls = [torch.rand(B, 1, D) + 0.5, torch.rand(B, 1, 1) + 0.5]  # ARD and shared
    os_ = [torch.rand(B) + 0.5, torch.rand(B) + 0.5]
    theta = K.kernel_sum_theta(ls, os_, (B,), D)
    assert theta.shape == (B, 2, D + 1) and theta.dtype == torch.float32 and theta.is_contiguous()
    for t in range(2):
        assert torch.equal(theta[:, t], K.kernel_theta(ls[t], os_[t], (B,), D))
    assert torch.allclose(theta[:, 1, :D], (1.0 / ls[1][:, 0]).expand(B, D)) and torch.allclose(theta[:, 0, D], os_[0] ** 2)
    # the struct of the kind: T rides in `nterms`, the packed families in n2, no `terms`
    desc = K.OperatorDescriptor(_hip.LO_OP_KERNEL_SUM_DIAG, B, 10, R=D, n2=0x21, kernel_terms=2)
    s = desc.c_struct()
    assert (s.kind, s.nterms, s.n2, s.R) == (12, 2, 0x21, D) and not s.terms
    assert desc.without_diag().kernel_terms == 2


def test_grouping_rules():
    x = torch.rand(30, 3)
    same = [kernel(x, "rbf"), kernel(x, "matern52"), kernel(x, "matern12")]
    assert shapes(slo._kernel_groups(same, check_device=False)) == [3]
    assert shapes(slo._kernel_groups(same)) == ["KernelLinearOperator"] * 3  # (CPU tensors: the device gate refuses)
    # a clone of the points is another tensor: its operator does not join the group
    assert shapes(slo._kernel_groups([same[0], kernel(x.clone(), "rbf"), same[1]], check_device=False)) == [2, 1]
    # more than LO_KERNEL_MAX_TERMS: the group splits
    five = [kernel(x, n) for n in ("rbf", "matern12", "matern32", "matern52", "rbf")]
    assert shapes(slo._kernel_groups(five, check_device=False)) == [4, 1]
    # non-native terms stay on their own, in place: another callable, D > 32, float64, a rectangular pair, a root
    other = KernelLinearOperator(x, x, lambda a, b, **kw: covariance.rbf(a, b, **kw), num_nonbatch_dimensions=NB,
                                 lengthscale=torch.ones(1, 3), outputscale=torch.tensor(1.0))
    wide = kernel(torch.rand(30, 33), "rbf")
    dbl = KernelLinearOperator(x.double(), x.double(), covariance.rbf, num_nonbatch_dimensions=NB,
                               lengthscale=torch.ones(1, 3).double(), outputscale=torch.tensor(1.0).double())
    rect = kernel(x, "rbf", x2=torch.rand(30, 3))
    root = RootLinearOperator(torch.rand(30, 2))
    items = slo._kernel_groups([same[0], other, wide, root, same[1], dbl, rect], check_device=False)
    assert shapes(items) == [2, "KernelLinearOperator", "KernelLinearOperator", "RootLinearOperator",
                             "KernelLinearOperator", "KernelLinearOperator"]
    assert items[0] == [same[0], same[1]]
    # the flattening the lowering groups over: nested sums and the diagonal of an AddedDiag
    nested = AddedDiagLinearOperator(same[0] + same[1] + root, DiagLinearOperator(torch.ones(30)))
    flat = slo._flatten_terms(nested.linear_ops)
    assert [type(o).__name__ for o in flat] == ["KernelLinearOperator", "KernelLinearOperator", "RootLinearOperator",
                                                "DiagLinearOperator"]
    # on the CPU nothing lowers
    assert (same[0] + same[1])._kernel_descriptor() is None and nested._kernel_descriptor() is None


def test_whole_sum_pair_rule_is_refused_off_the_device():
    x, xs = torch.rand(30, 3), torch.rand(7, 3)
    rect = [kernel(xs, "rbf", x2=x), kernel(xs, "matern32", x2=x)]
    assert slo._kernel_group_pair(rect) is None  # (the products of CPU tensors stay with the general path)
    S = rect[0] + rect[1]
    v = torch.randn(30, 2)
    assert torch.allclose(S._matmul(v), sum(op.to_dense() for op in rect) @ v, atol=1e-5)
    w = torch.randn(7, 2)
    assert torch.allclose(S._t_matmul(w), S.to_dense().mT @ w, atol=1e-5)


def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g39_kernel_sum_{p}.npz"))


def tensors(p, dtype=torch.float32):
    return {k: torch.from_numpy(v).to(dtype) for k, v in inputs(p).items()}


def kernel_sum(p, t):
    ops = [KernelLinearOperator(t["x"], t["x"], covariance.FAMILIES[f], num_nonbatch_dimensions=NB,
                                lengthscale=t[f"lengthscale{k}"], outputscale=t[f"outputscale{k}"])
           for k, f in enumerate(CASES[p][0])]
    total = ops[0]
    for op in ops[1:]:
        total = total + op
    return total, ops


@pytest.mark.parametrize("p", list(CASES))
def test_cpu_algebra_of_a_kernel_sum_equals_the_dense_sum(p):
    G, t = golden(p), tensors(p)
    S, ops = kernel_sum(p, t)
    assert isinstance(S, SumLinearOperator) and len(S.linear_ops) == len(ops)
    dense = sum(op.to_dense() for op in ops)
    assert torch.equal(S.to_dense(), dense)
    err, ref = rel((S @ t["V"]).double().numpy(), G["mv_64"]), max(float(G["mv_err"]), ERR_FLOOR)
    assert err <= REF_FACTOR * ref, (err, ref)
    assert torch.allclose(S.diagonal(), sum(t[f"outputscale{k}"] ** 2 for k in range(len(ops))).unsqueeze(-1)
                          .expand(*S.batch_shape, S.shape[-1]))
    assert torch.allclose(S._t_matmul(t["V"]), dense.mT @ t["V"], rtol=1e-4, atol=1e-5)
    # the derivative through the general path: per operator (x1, x2, parameters) in sum order, equal to autograd
    t64 = {k: v.double() for k, v in tensors(p).items()}
    for k in t64:
        if k.startswith(("lengthscale", "outputscale")):
            t64[k].requires_grad_(True)
    S64, ops64 = kernel_sum(p, t64)
    grads = S64._bilinear_derivative(t64["V"], t64["V"])
    assert len(grads) == 4 * len(ops64)
    (t64["V"] * (S64.to_dense() @ t64["V"])).sum().backward()
    for k in range(len(ops64)):
        assert grads[4 * k] is None and grads[4 * k + 1] is None
        assert torch.allclose(grads[4 * k + 2], t64[f"lengthscale{k}"].grad)
        assert torch.allclose(grads[4 * k + 3], t64[f"outputscale{k}"].grad)
