"""The matrix-free multitask operator Kron(Kernel, Dense(Bt)) without a GPU: the binding of ABI 29 (symbols, constants,
the host-side sizer against the closed form of its layout), the gate of the lowering decided on CPU tensors through its
`check_device=False` form, the CPU general path against the reference's goldens (tests/golden/g40_kernel_kron_*.npz) and
the composed `_bilinear_derivative` against float64 autograd of the dense matrix."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_kernel_kron import CASES, ERR_FLOOR, dense_kron, inputs, rel  # noqa: E402

from linear_operator_amd import _hip, covariance  # noqa: E402
from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    DenseLinearOperator, KernelLinearOperator, KroneckerProductLinearOperator, RootLinearOperator)

REF_FACTOR = 4.0
NB = {"outputscale": 0}


def kernel(x, name="rbf", x2=None, dtype=torch.float32):
    D = x.shape[-1]
    return KernelLinearOperator(x, x if x2 is None else x2, covariance.FAMILIES[name], num_nonbatch_dimensions=NB,
                                lengthscale=torch.full((1, D), 0.6, dtype=dtype), outputscale=torch.tensor(1.1, dtype=dtype))


def split_count(B, n):
    """ko_shape of csrc/lo_kernel_shape.h: the workgroups the points j of a member are split over."""
    rb, tiles = -(-n // 256), -(-n // 128)
    wgs = rb * B
    js = 1 if wgs >= 512 else min(tiles, -(-512 // wgs), 64)
    jchunk = -(-tiles // js) * 128
    return -(-n // jchunk)


def test_binding_of_abi_29():
    assert _hip.ABI_VERSION >= 29 and _hip.LO_OP_KERNEL_KRON_DIAG == 13 and _hip.LO_KERNEL_KRON_MAX_TASKS == 8
    assert "lo_kernel_kron_mv_workspace_bytes" in _hip.EXPORTS and "lo_kernel_kron_mv_f32" in _hip.EXPORTS
    assert len(_hip._PROTOTYPES["lo_kernel_kron_mv_workspace_bytes"][1]) == 5
    assert len(_hip._PROTOTYPES["lo_kernel_kron_mv_f32"][1]) == 16
    assert callable(K.kernel_kron_diag_descriptor) and callable(K.kernel_kron_mv)
    lib = _hip.load()  # (the sizer is host code)
    assert lib.lo_abi_version() >= 29
    # the struct of the kind: T rides in `nterms`, the family in n2, the union slot holds the device pointer of Bt as given
    Bt = torch.eye(3).expand(2, 3, 3).contiguous()
    desc = K.OperatorDescriptor(_hip.LO_OP_KERNEL_KRON_DIAG, 2, 30, R=4, n2=2, kernel_terms=3, task=Bt)
    s = desc.c_struct()
    import ctypes

    assert (s.kind, s.nterms, s.n2, s.R, s.N) == (13, 3, 2, 4, 30)
    assert ctypes.cast(s.terms, ctypes.c_void_p).value == Bt.data_ptr()
    assert desc.without_diag().task is Bt and desc.without_diag().kernel_terms == 3


@pytest.mark.parametrize("B,n,D,T,c", [(512, 40, 2, 2, 2), (128, 1024, 1, 8, 17), (1, 1, 1, 1, 1), (1, 300, 8, 3, 17),
                                       (3, 257, 3, 2, 1), (1, 16384, 4, 4, 1), (8, 4096, 16, 8, 17)])
def test_sizer_is_the_closed_form_of_the_layout(B, n, D, T, c):
    """The tail alone without a split; with one, js copies of the product [B, n T, c] (one take: no padding between)."""
    lib = _hip.load()
    js = split_count(B, n)
    want = 256 + (4 * js * B * n * T * c if js > 1 else 0)
    assert lib.lo_kernel_kron_mv_workspace_bytes(B, n, D, T, c) == want
    if (B, n) in ((512, 40), (128, 1024), (1, 1)):
        assert js == 1
    if (B, n) in ((1, 300), (3, 257), (1, 16384)):
        assert js > 1


def test_sizer_refuses_what_the_entry_point_refuses():
    lib = _hip.load()
    for args in ((1, 10, 33, 2, 1), (1, 10, 3, 9, 1), (1, 10, 3, 0, 1), (0, 10, 3, 2, 1), (1, 0, 3, 2, 1), (1, 10, 0, 2, 1),
                 (1, 10, 3, 2, 0)):
        assert lib.lo_kernel_kron_mv_workspace_bytes(*args) == 0, args


def test_gate_on_cpu_tensors():
    x = torch.rand(30, 3)
    Bt = torch.eye(2) + 0.1
    ok = KroneckerProductLinearOperator(kernel(x), DenseLinearOperator(Bt))
    assert ok._kernel_kron_refusal(check_device=False) is None
    assert "device" in ok._kernel_kron_refusal()  # (CPU tensors: the full gate refuses, nothing lowers)
    assert ok._kernel_descriptor() is None
    # T = 8 is taken, T = 9 is not
    assert KroneckerProductLinearOperator(kernel(x), DenseLinearOperator(torch.eye(8)))._kernel_kron_refusal(False) is None
    nine = KroneckerProductLinearOperator(kernel(x), DenseLinearOperator(torch.eye(9)))
    assert "LO_KERNEL_KRON_MAX_TASKS" in nine._kernel_kron_refusal(check_device=False)
    three = KroneckerProductLinearOperator(kernel(x), DenseLinearOperator(Bt), DenseLinearOperator(Bt))
    assert "3 factors" in three._kernel_kron_refusal(check_device=False)
    dbl = KroneckerProductLinearOperator(kernel(x.double(), dtype=torch.float64), DenseLinearOperator(Bt.double()))
    assert "float32" in dbl._kernel_kron_refusal(check_device=False)
    half = KroneckerProductLinearOperator(kernel(x), DenseLinearOperator(Bt.double()))
    assert "task factor not float32" == half._kernel_kron_refusal(check_device=False)
    rect = KroneckerProductLinearOperator(kernel(x, x2=torch.rand(30, 3)), DenseLinearOperator(Bt))
    assert "two different point tensors" in rect._kernel_kron_refusal(check_device=False)
    root = KroneckerProductLinearOperator(kernel(x), RootLinearOperator(torch.rand(2, 1)))
    assert "not a DenseLinearOperator" in root._kernel_kron_refusal(check_device=False)
    swapped = KroneckerProductLinearOperator(DenseLinearOperator(Bt), kernel(x))
    assert "not a KernelLinearOperator" in swapped._kernel_kron_refusal(check_device=False)
    other = KernelLinearOperator(x, x, lambda a, b, **kw: covariance.rbf(a, b, **kw), num_nonbatch_dimensions=NB,
                                 lengthscale=torch.ones(1, 3), outputscale=torch.tensor(1.0))
    assert "native_family" in KroneckerProductLinearOperator(other, DenseLinearOperator(Bt))._kernel_kron_refusal(False)
    wide = KroneckerProductLinearOperator(kernel(torch.rand(30, 33)), DenseLinearOperator(Bt))
    assert "LO_KERNEL_MAX_DIM" in wide._kernel_kron_refusal(check_device=False)
    # two dense factors still lower as before: the gate only adds a case
    assert KroneckerProductLinearOperator(DenseLinearOperator(Bt), DenseLinearOperator(Bt))._two_groups() is None  # (CPU)


def golden(p):
    return np.load(os.path.join(HERE, "golden", f"g40_kernel_kron_{p}.npz"))


def tensors(p, dtype=torch.float32):
    return {k: torch.from_numpy(v).to(dtype) for k, v in inputs(p).items()}


def kron_op(p, t):
    kern = KernelLinearOperator(t["x"], t["x"], covariance.FAMILIES[CASES[p][0]], num_nonbatch_dimensions=NB,
                                lengthscale=t["lengthscale"], outputscale=t["outputscale"])
    return KroneckerProductLinearOperator(kern, DenseLinearOperator(t["task"]))


@pytest.mark.parametrize("p", list(CASES))
def test_fixtures_load_and_the_cpu_general_path_meets_them(p):
    G, t = golden(p), tensors(p)
    family, B, n, D, T, ard, seed = CASES[p]
    assert G["mv"].shape == (B, n * T, 4) and G["piv"].shape == (B, 15) and G["gB"].shape == (B, T, T)
    for q in ("mv", "diag", "solve", "iq", "L", "ld", "gl", "go", "gx", "gB"):
        assert q in G.files and q + "_64" in G.files and float(G[q + "_err"]) < 2e-3, q
    op = kron_op(p, t)
    assert op._kernel_kron_refusal(check_device=False) is None
    fn = covariance.FAMILIES[family]
    dense = dense_kron(fn(t["x"], t["x"], t["lengthscale"], t["outputscale"]), t["task"])
    assert torch.allclose(op.to_dense(), dense, rtol=1e-6, atol=1e-7)
    for q, val in (("mv", op @ t["V"]), ("diag", op.diagonal())):
        err, ref = rel(val.double().numpy(), G[q + "_64"]), max(float(G[q + "_err"]), ERR_FLOOR)
        assert err <= REF_FACTOR * ref, (q, err, ref)
    # the diagonal is outputscale^2 (x) diag(Bt), index i T + t
    want = (t["outputscale"] ** 2)[:, None, None] * t["task"].diagonal(dim1=-1, dim2=-2)[:, None, :]
    assert torch.allclose(op._diagonal(), want.expand(B, n, T).reshape(B, n * T))


@pytest.mark.parametrize("ard", [True, False])
def test_composed_bilinear_derivative_equals_float64_autograd(ard):
    """n = 9, T = 2, a NON-symmetric Bt and a batch of 2; every leaf of the representation."""
    g = torch.Generator().manual_seed(11)
    B, n, D, T, S = 2, 9, 3, 2, 3
    leaves = {
        "x": torch.rand(B, n, D, generator=g, dtype=torch.float64),
        "lengthscale": 0.5 + torch.rand(B, 1, D if ard else 1, generator=g, dtype=torch.float64),
        "outputscale": 0.7 + torch.rand(B, generator=g, dtype=torch.float64),
        "task": torch.eye(T, dtype=torch.float64) + 0.3 * torch.rand(B, T, T, generator=g, dtype=torch.float64),
    }
    for v in leaves.values():
        v.requires_grad_(True)
    U = torch.randn(B, n * T, S, generator=g, dtype=torch.float64)
    V = torch.randn(B, n * T, S, generator=g, dtype=torch.float64)
    kern = KernelLinearOperator(leaves["x"], leaves["x"], covariance.matern52, num_nonbatch_dimensions=NB,
                                lengthscale=leaves["lengthscale"], outputscale=leaves["outputscale"])
    op = KroneckerProductLinearOperator(kern, DenseLinearOperator(leaves["task"]))
    grads = op._bilinear_derivative(U, V)
    assert len(grads) == len(op.representation()) == 5  # x1, x2, lengthscale, outputscale, Bt
    dense = dense_kron(covariance.matern52(leaves["x"], leaves["x"], leaves["lengthscale"], leaves["outputscale"]),
                       leaves["task"])
    (U * (dense @ V)).sum().backward()
    gx = grads[0] + grads[1]  # (one leaf on both sides: autograd adds the two)
    for got, name in ((gx, "x"), (grads[2], "lengthscale"), (grads[3], "outputscale"), (grads[4], "task")):
        assert got.shape == leaves[name].shape
        assert torch.allclose(got, leaves[name].grad, rtol=1e-9, atol=1e-11), name
    # a task factor that asks for no gradient gets None, and the kernel factor's are unchanged
    op2 = KroneckerProductLinearOperator(kern, DenseLinearOperator(leaves["task"].detach()))
    g2 = op2._bilinear_derivative(U, V)
    assert g2[4] is None and torch.allclose(g2[2], grads[2])
