"""Kronecker product of Toeplitz factors without a GPU: the torch closed form of the column gradients against the
reference's goldens (tests/golden/g36_toeplitz_kron.npz) and an fp64 dense formula, the lowering rules and the binding."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_toeplitz_kron import CASES, inputs  # noqa: E402

from linear_operator_amd import _hip  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DenseLinearOperator, DiagLinearOperator, InterpolatedLinearOperator,
    KroneckerProductLinearOperator, ToeplitzLinearOperator)

X = inputs()
G = np.load(os.path.join(HERE, "golden", "g36_toeplitz_kron.npz"))


def kron(cols):
    return KroneckerProductLinearOperator(*[ToeplitzLinearOperator(c) for c in cols])


def dense_grads64(cols, u, v):
    """g_k[l] = sum_s u_s^T (dK / dt_k[l]) v_s for one member in fp64, with the dense matrices: dK / dt_k[l] is the
    Kronecker product with factor k replaced by E_l, ones on the l-th sub- and superdiagonal (the identity for l = 0)."""
    mats = []
    for t in cols:
        m = t.shape[-1]
        mats.append(t.astype(np.float64)[np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])])
    u, v = u.astype(np.float64), v.astype(np.float64)
    out = []
    for k, t in enumerate(cols):
        m = t.shape[-1]
        lag = np.abs(np.arange(m)[:, None] - np.arange(m)[None, :])
        g = np.zeros(m)
        for l in range(m):
            K = np.ones((1, 1))
            for j, Tj in enumerate(mats):
                K = np.kron(K, (lag == l).astype(np.float64) if j == k else Tj)
            g[l] = (u * (K @ v)).sum()
        out.append(g)
    return out


@pytest.mark.parametrize("p", list(CASES))
def test_closed_form_column_gradients_against_the_reference(p):
    grid, B = CASES[p]
    cols = [torch.from_numpy(X[f"{p}_c{k + 1}"]) for k in range(len(grid))]
    grads = kron(cols)._bilinear_derivative(torch.from_numpy(X[p + "_u"]), torch.from_numpy(X[p + "_v"]))
    assert len(grads) == len(grid)
    for k, g in enumerate(grads):
        ref = G[f"{p}_g{k + 1}"]
        assert tuple(g.shape) == ref.shape == tuple(cols[k].shape)
        # fp32 on both sides (the reference: autograd through its FFT composition): 2e-4 of the largest entry
        assert np.abs(g.numpy() - ref).max() <= 2e-4 * np.abs(ref).max()


@pytest.mark.parametrize("grid,B", [((5, 7), 1), ((4, 3, 5), 1), ((3, 4, 2, 3), 1), ((5, 7), 3)])
def test_closed_form_in_float64_against_the_dense_formula(grid, B):
    r = np.random.Generator(np.random.PCG64(41))
    cols = [0.2 + r.random((B, m)) for m in grid]
    N = int(np.prod(grid))
    u, v = r.standard_normal((B, N, 3)), r.standard_normal((B, N, 3))
    grads = kron([torch.from_numpy(c) for c in cols])._bilinear_derivative(torch.from_numpy(u), torch.from_numpy(v))
    assert len(grads) == len(grid)  # (four factors: the closed form takes any number)
    for b in range(B):
        ref = dense_grads64([c[b] for c in cols], u[b], v[b])
        for k in range(len(grid)):
            assert np.abs(grads[k][b].numpy() - ref[k]).max() <= 1e-10 * max(1.0, np.abs(ref[k]).max())


def test_shared_columns_receive_the_summed_gradient():
    """A column without a batch dimension under batched vectors: the gradient is summed to the column's own shape."""
    r = np.random.Generator(np.random.PCG64(42))
    c1, c2 = torch.from_numpy(0.2 + r.random(4)), torch.from_numpy(0.2 + r.random(5))
    u, v = torch.from_numpy(r.standard_normal((3, 20, 2))), torch.from_numpy(r.standard_normal((3, 20, 2)))
    g1, g2 = kron([c1, c2])._bilinear_derivative(u, v)
    assert g1.shape == c1.shape and g2.shape == c2.shape
    ref = [sum(x) for x in zip(*[dense_grads64([c1.numpy(), c2.numpy()], u[b].numpy(), v[b].numpy()) for b in range(3)])]
    assert np.abs(g1.numpy() - ref[0]).max() <= 1e-10 and np.abs(g2.numpy() - ref[1]).max() <= 1e-10


def test_matmul_backward_reaches_the_columns():
    cols = [torch.from_numpy(X[f"g2_c{k}"].astype(np.float64)).requires_grad_(True) for k in (1, 2)]
    v = torch.from_numpy(X["g2_v"].astype(np.float64))
    kron(cols).matmul(v).sum().backward()
    ref = dense_grads64([c.detach().numpy()[0] for c in cols], np.ones_like(X["g2_v"][0]), X["g2_v"][0])
    for c, g in zip(cols, ref):
        assert c.grad is not None and np.abs(c.grad.numpy()[0] - g).max() <= 1e-9 * np.abs(g).max()


def test_mixed_toeplitz_and_dense_factors_stay_not_implemented():
    c1 = torch.from_numpy(X["g2_c1"][0])
    dense = DenseLinearOperator(ToeplitzLinearOperator(torch.from_numpy(X["g2_c2"][0])).to_dense())
    A = KroneckerProductLinearOperator(ToeplitzLinearOperator(c1), dense)
    with pytest.raises(NotImplementedError):
        A._bilinear_derivative(torch.from_numpy(X["g2_u"][0]), torch.from_numpy(X["g2_v"][0]))


def test_no_descriptor_on_the_cpu_or_in_float64():
    cols = [torch.from_numpy(X[f"g2_c{k}"]) for k in (1, 2)]
    assert kron(cols)._kernel_descriptor() is None
    assert kron([c.double() for c in cols])._kernel_descriptor() is None
    A = AddedDiagLinearOperator(kron(cols), DiagLinearOperator(torch.from_numpy(X["g2_d"])))
    assert A._kernel_descriptor() is None


def test_binding_carries_the_abi_24_entry_points():
    assert _hip.ABI_VERSION >= 24 and _hip.LO_OP_TOEPLITZ_KRON_DIAG == 10
    for name in ("lo_toeplitz_kron_bilinear_workspace_bytes", "lo_toeplitz_kron_bilinear_f32"):
        assert name in _hip._PROTOTYPES and name in _hip.EXPORTS
    assert ctypes.sizeof(_hip.GridDesc) == 32 and _hip.GridDesc.m.offset == 8
    assert ctypes.sizeof(_hip.OpDesc) == 80 and _hip.OpDesc.terms.offset == 72  # the layout of ABI 15


def test_interpolated_operator_over_such_a_base_still_refuses_column_gradients():
    c1 = torch.from_numpy(X["g2_c1"]).requires_grad_(True)
    base = kron([c1, torch.from_numpy(X["g2_c2"])])
    idx = torch.arange(192).reshape(1, 192, 1)
    A = InterpolatedLinearOperator(base, idx, torch.ones(1, 192, 1), idx, torch.ones(1, 192, 1))
    with pytest.raises(NotImplementedError):
        A.matmul(torch.from_numpy(X["g2_rhs"])).sum().backward()
