"""KernelLinearOperator without a GPU: the constructor's broadcasting and error messages, dense evaluation, diagonal,
entries, slicing and transpose against the reference's goldens (tests/golden/g38_kernel_op_*.npz), the general path for
an arbitrary callable, the gate of the native path and the binding of ABI 26."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_op import CASES, ERR_FLOOR, inputs, rel  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DiagLinearOperator, KernelLinearOperator, LinearOperator)

REF_FACTOR = 4.0  # allowed multiple of the reference's own recorded error
NB = {"outputscale": 0}


def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g38_kernel_op_{p}.npz"))


def tensors(p, dtype=torch.float32):
    return {k: torch.from_numpy(v).to(dtype) if v.dtype.kind == "f" else torch.from_numpy(v) for k, v in inputs(p).items()}


def kernel_op(p, t=None, fn=None):
    t = tensors(p) if t is None else t
    fn = covariance.FAMILIES[CASES[p][0]] if fn is None else fn
    return KernelLinearOperator(t["x"], t["x"], fn, num_nonbatch_dimensions=NB, lengthscale=t["lengthscale"],
                                outputscale=t["outputscale"])


def check(G, q, value):
    err, ref = rel(value.detach().double().numpy(), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
    assert err <= REF_FACTOR * ref, (q, err, ref)


def test_binding_of_abi_26():
    assert _hip.ABI_VERSION >= 26 and _hip.LO_OP_KERNEL_DIAG == 11 and _hip.LO_KERNEL_MAX_DIM == 32
    for name in ("lo_kernel_mv_workspace_bytes", "lo_kernel_mv_f32", "lo_kernel_bilinear_workspace_bytes",
                 "lo_kernel_bilinear_f32"):
        assert name in _hip._PROTOTYPES and name in _hip.EXPORTS
    assert len(_hip._PROTOTYPES["lo_kernel_mv_f32"][1]) == 16
    assert len(_hip._PROTOTYPES["lo_kernel_bilinear_f32"][1]) == 15
    assert [f.native_family for f in (covariance.rbf, covariance.matern12, covariance.matern32, covariance.matern52)] == \
        [0, 1, 2, 3]
    lib = _hip.load()  # the sizers are host code
    assert lib.lo_kernel_mv_workspace_bytes(1, 1013, 1013, 8, 1) > 0
    assert lib.lo_kernel_mv_workspace_bytes(1, 10, 10, 33, 1) == 0 and lib.lo_kernel_mv_workspace_bytes(0, 1, 1, 1, 1) == 0
    assert lib.lo_kernel_bilinear_workspace_bytes(2, 77, 130, 32, 3) > 0
    assert lib.lo_kernel_bilinear_workspace_bytes(2, 77, 130, 33, 3) == 0


def test_covariance_formulas_against_numpy():
    g = np.random.Generator(np.random.PCG64(11))
    x1, x2 = g.standard_normal((2, 5, 3)), g.standard_normal((2, 4, 3))
    ls, os_ = 0.5 + g.random((2, 1, 3)), 0.5 + g.random(2)
    r = np.sqrt((((x1 / ls)[:, :, None, :] - (x2 / ls)[:, None, :, :]) ** 2).sum(-1))
    want = {"rbf": np.exp(-r ** 2 / 2), "matern12": np.exp(-r),
            "matern32": (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r),
            "matern52": (1 + np.sqrt(5) * r + 5 * r ** 2 / 3) * np.exp(-np.sqrt(5) * r)}
    T = torch.from_numpy
    for name, fn in covariance.FAMILIES.items():
        got = fn(T(x1), T(x2), T(ls), T(os_)).numpy()
        np.testing.assert_allclose(got, os_[:, None, None] ** 2 * want[name], rtol=1e-12)
        shared = fn(T(x1), T(x2), T(ls[..., :1]), T(os_)).numpy()
        assert shared.shape == (2, 5, 4)


def test_coincident_points_have_finite_zero_lengthscale_gradients():
    x = torch.tensor([[0.1, 0.2], [0.1, 0.2]], dtype=torch.float64)
    for fn in covariance.FAMILIES.values():
        ls = torch.tensor([[0.7, 0.9]], dtype=torch.float64, requires_grad=True)
        xg = x.clone().requires_grad_(True)
        fn(xg, xg, ls, torch.tensor(1.3, dtype=torch.float64)).sum().backward()
        assert torch.equal(ls.grad, torch.zeros_like(ls)) and torch.isfinite(xg.grad).all()


def test_constructor_broadcasts_data_and_parameters():
    x1, x2 = torch.randn(3, 1, 6, 2), torch.randn(4, 5, 2)
    op = KernelLinearOperator(x1, x2, covariance.rbf, num_nonbatch_dimensions=NB, lengthscale=torch.ones(1, 2),
                              outputscale=torch.ones(4))
    assert op.shape == (3, 4, 6, 5) and op.x1.shape == (3, 4, 6, 2) and op.x2.shape == (3, 4, 5, 2)
    assert op.tensor_params["lengthscale"].shape == (3, 4, 1, 2) and op.tensor_params["outputscale"].shape == (3, 4)
    assert len(op.representation()) == 4
    dense = covariance.rbf(x1, x2, torch.ones(1, 2), torch.ones(4))
    assert torch.allclose(op.to_dense(), dense)
    assert op.mT.shape == (3, 4, 5, 6) and torch.allclose(op.mT.to_dense(), dense.mT)
    two = KernelLinearOperator(torch.randn(6, 2), torch.randn(5, 2), lambda a, b, **kw: torch.ones(12, 15),
                               num_outputs_per_input=(2, 3))
    assert two.shape == (12, 15)


def test_constructor_error_messages():
    with pytest.raises(RuntimeError, match="Incompatible data shapes for a kernel matrix"):
        KernelLinearOperator(torch.randn(3, 6, 2), torch.randn(4, 5, 2), covariance.rbf)
    with pytest.raises(RuntimeError, match="Shape of kernel parameters"):
        KernelLinearOperator(torch.randn(3, 6, 2), torch.randn(3, 5, 2), covariance.rbf, num_nonbatch_dimensions=NB,
                             lengthscale=torch.ones(2, 1, 2), outputscale=torch.ones(3))
    with pytest.raises(RuntimeError, match="Recall that parameters passed to KernelLinearOperator"):
        KernelLinearOperator(torch.randn(6, 2), torch.randn(5, 2), covariance.rbf, lengthscale=torch.ones(1, 2),
                             outputscale=torch.ones(3, 1, 2), other=torch.ones(4, 1, 1))


@pytest.mark.parametrize("p", list(CASES))
def test_dense_diagonal_entries_against_the_goldens(p):
    G, t = golden(p), tensors(p)
    op = kernel_op(p, t)
    dense = op.to_dense()
    check(G, "mv", dense @ t["V"])
    check(G, "mv", op @ t["V"])
    check(G, "diag", op.diagonal())
    assert torch.equal(op._diagonal(), t["outputscale"].square().unsqueeze(-1).expand(*op.shape[:-1]))
    check(G, "idx", op[t["ib"], t["ir"], t["ic"]])
    check(G, "idx", op._get_indices(t["ir"], t["ic"], t["ib"]))
    rows = op._get_rows(torch.zeros(op.batch_shape, dtype=torch.long) + 2)
    assert torch.allclose(rows, dense[..., 2, :], rtol=1e-6, atol=1e-7)


def test_diagonal_of_a_rectangular_pairing_and_of_another_callable():
    t = tensors("rbf")
    x2 = t["x"].flip(-2).contiguous()
    op = KernelLinearOperator(t["x"], x2, covariance.matern32, num_nonbatch_dimensions=NB,
                              lengthscale=t["lengthscale"], outputscale=t["outputscale"])
    assert not op._same_points()
    assert torch.allclose(op._diagonal(), op.to_dense().diagonal(dim1=-2, dim2=-1), rtol=1e-6)


def test_slicing_transpose_and_batch_reshapes():
    p = "rbf"
    t = tensors(p)
    op = kernel_op(p, t)
    dense = op.to_dense()
    sub = op[1:3, 5:40, 7:19]
    assert isinstance(sub, KernelLinearOperator) and sub.shape == (2, 35, 12)
    assert torch.equal(sub.to_dense(), dense[1:3, 5:40, 7:19])
    same = op[:, 10:50, 10:50]
    assert same._same_points() and torch.equal(same.to_dense(), dense[:, 10:50, 10:50])
    assert torch.equal(op[2].to_dense(), dense[2]) and op[2].shape == (257, 257)
    assert torch.equal(op[0, 3], dense[0, 3]) and torch.equal(op[..., 4], dense[..., 4])
    assert torch.equal(op.mT.to_dense(), dense.mT)
    assert op._expand_batch((2, 3)).shape == (2, 3, 257, 257)
    un = op._unsqueeze_batch(0)
    assert un.shape == (1, 3, 257, 257) and un._same_points() and torch.equal(un.to_dense()[0], dense)
    two = op._expand_batch((2, 3))._permute_batch(1, 0)
    assert two.shape == (3, 2, 257, 257) and torch.equal(two.to_dense()[:, 1], dense)
    det = op.detach()
    assert isinstance(det, KernelLinearOperator) and det.covar_func is op.covar_func
    rebuilt = op.representation_tree()(*op.representation())
    assert isinstance(rebuilt, KernelLinearOperator) and rebuilt._same_points()
    assert rebuilt.num_nonbatch_dimensions["outputscale"] == 0 and rebuilt.num_nonbatch_dimensions["lengthscale"] == 2


def test_arbitrary_callable_takes_the_general_path():
    def poly(x1, x2, c, degree=2):
        return (x1 @ x2.mT + c) ** degree

    x1, x2 = torch.randn(2, 9, 3, dtype=torch.float64), torch.randn(2, 7, 3, dtype=torch.float64)
    c = torch.tensor([[[0.5]], [[1.5]]], dtype=torch.float64, requires_grad=True)
    op = KernelLinearOperator(x1, x2, poly, c=c, degree=3)
    assert op._native_refusal(check_device=False) == "covar_func has no native_family" and op._kernel_descriptor() is None
    dense = poly(x1, x2, c, 3)
    v = torch.randn(2, 7, 2, dtype=torch.float64)
    assert torch.allclose(op @ v, dense @ v) and torch.allclose(op.to_dense(), dense)
    assert torch.allclose(op._diagonal() if op.is_square else op[:, :7, :]._diagonal(), dense[:, :7, :].diagonal(dim1=-2, dim2=-1))
    i, r, col = torch.tensor([0, 1, 1]), torch.tensor([8, 0, 3]), torch.tensor([6, 6, 2])
    assert torch.allclose(op[i, r, col], dense[i, r, col])
    (op @ v).sum().backward()
    (want,) = torch.autograd.grad((poly(x1, x2, c, 3) @ v).sum(), c)
    assert torch.allclose(c.grad, want)


def test_general_path_gradients_match_dense_autograd():
    p = "m12"
    t = tensors(p, torch.float64)
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("x", "lengthscale", "outputscale")}
    op = KernelLinearOperator(leaves["x"], leaves["x"], covariance.matern12, num_nonbatch_dimensions=NB,
                              lengthscale=leaves["lengthscale"], outputscale=leaves["outputscale"])
    u, v = torch.randn(1, 63, 2, dtype=torch.float64), torch.randn(1, 63, 2, dtype=torch.float64)
    gx1, gx2, gl, go = op._bilinear_derivative(u, v)
    ref = {k: t[k].clone().requires_grad_(True) for k in leaves}
    (u * (covariance.matern12(ref["x"], ref["x"], ref["lengthscale"], ref["outputscale"]) @ v)).sum().backward()
    assert torch.allclose(gx1 + gx2, ref["x"].grad) and torch.allclose(gl, ref["lengthscale"].grad)
    assert torch.allclose(go, ref["outputscale"].grad)


def test_gate_of_the_native_path():
    t = tensors("rbf")
    op = kernel_op("rbf", t)
    assert op._native_refusal(check_device=False) is None
    assert op._native_refusal() == "not on the device" and op._kernel_descriptor() is None  # (CPU tensors)
    wide = KernelLinearOperator(torch.randn(5, 33), torch.randn(5, 33), covariance.rbf, num_nonbatch_dimensions=NB,
                                lengthscale=torch.ones(1, 33), outputscale=torch.tensor(1.0))
    assert "LO_KERNEL_MAX_DIM" in wide._native_refusal(check_device=False)
    edge = KernelLinearOperator(torch.randn(5, 32), torch.randn(5, 32), covariance.rbf, num_nonbatch_dimensions=NB,
                                lengthscale=torch.ones(1, 1), outputscale=torch.tensor(1.0))
    assert edge._native_refusal(check_device=False) is None
    assert kernel_op("rbf", tensors("rbf", torch.float64))._native_refusal(check_device=False) == "not float32"
    two = KernelLinearOperator(torch.randn(5, 2), torch.randn(5, 2), covariance.rbf, num_outputs_per_input=(2, 2),
                               num_nonbatch_dimensions=NB, lengthscale=torch.ones(1, 2), outputscale=torch.tensor(1.0))
    assert two._native_refusal(check_device=False) == "more than one output per input"
    extra = KernelLinearOperator(t["x"], t["x"], covariance.rbf, num_nonbatch_dimensions=NB,
                                 lengthscale=t["lengthscale"], outputscale=t["outputscale"], period=torch.ones(3, 1, 1))
    assert "parameters other than" in extra._native_refusal(check_device=False)
    no_nb = KernelLinearOperator(t["x"][0], t["x"][0], covariance.rbf, lengthscale=t["lengthscale"][0],
                                 outputscale=torch.ones(1, 1))
    assert "outputscale" in no_nb._native_refusal(check_device=False)
    # x1 is not x2: the product is native (rectangular kernel), but there is no square descriptor
    other = KernelLinearOperator(t["x"], t["x"].clone(), covariance.rbf, num_nonbatch_dimensions=NB,
                                 lengthscale=t["lengthscale"], outputscale=t["outputscale"])
    assert other._native_refusal(check_device=False) is None and not other._same_points()
    assert other._kernel_descriptor() is None
    view = KernelLinearOperator(t["x"], t["x"].view(3, 257, 3), covariance.rbf, num_nonbatch_dimensions=NB,
                                lengthscale=t["lengthscale"], outputscale=t["outputscale"])
    assert view._same_points()  # (equal address, shape and strides)


def test_added_diag_on_the_cpu_keeps_the_reference_algebra():
    t = tensors("m12")
    A = AddedDiagLinearOperator(kernel_op("m12", t), DiagLinearOperator(t["noise"]))
    assert isinstance(A, LinearOperator) and A._kernel_descriptor() is None
    want = covariance.matern12(t["x"], t["x"], t["lengthscale"], t["outputscale"]) @ t["V"] + t["noise"].unsqueeze(-1) * t["V"]
    assert torch.allclose(A._matmul(t["V"]), want, rtol=1e-5, atol=1e-6)
    assert torch.allclose(A._diagonal(), t["outputscale"].square().unsqueeze(-1) + t["noise"])
