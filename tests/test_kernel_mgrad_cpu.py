"""covariance.matern52_grad and the gate of its native variant, without a GPU: every block of the function against float64
autograd of covariance.matern52, and `_native_mgrad_refusal` through check_device=False.

The one exactly coincident pair: covariance._dist cuts the square root's derivative off there, so autograd of
covariance.matern52 has no usable second derivative (it differentiates only the 5 r^2 / 3 term and gives -2 times the
limit).  The value and first-derivative entries of that block are held to autograd like every other pair's, its
second-derivative entries to the limit r -> 0 of the block formula, os^2 diag((5 / 3) / l_a^2)."""
import pytest
import torch

from linear_operator_amd import _hip, covariance
from linear_operator_amd.operators import KernelLinearOperator

NB = {"outputscale": 0}


def autograd_block(a, b, ls, os_):
    """[D + 1, D + 1]: k, dk/db (row 0), dk/da (column 0) and d2k / da db of covariance.matern52 at the pair (a, b)."""
    D = a.numel()
    a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    k = covariance.matern52(a[None], b[None], ls, os_)[0, 0]
    ga, gb = torch.autograd.grad(k, (a, b), create_graph=True)
    blk = torch.zeros(D + 1, D + 1, dtype=torch.float64)
    blk[0, 0], blk[1:, 0], blk[0, 1:] = k, ga, gb
    for p in range(D):
        blk[p + 1, 1:] = torch.autograd.grad(ga[p], b, retain_graph=True)[0]
    return blk.detach()


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("ard", [False, True], ids=["shared", "ard"])
def test_blocks_against_fp64_autograd_of_matern52(D, ard):
    g = torch.Generator().manual_seed(4100 + D)
    M, N, T = 4, 5, D + 1
    x1 = torch.rand(M, D, generator=g, dtype=torch.float64)
    x2 = torch.rand(N, D, generator=g, dtype=torch.float64)
    x2[2] = x1[1]  # the coincident pair (1, 2)
    ls = 0.3 + torch.rand(1, D if ard else 1, generator=g, dtype=torch.float64)
    os_ = torch.tensor(1.3, dtype=torch.float64)
    Kd = covariance.matern52_grad(x1, x2, ls, os_)
    assert Kd.shape == (M * T, N * T)
    for i in range(M):
        for j in range(N):
            got, want = Kd[i * T:(i + 1) * T, j * T:(j + 1) * T], autograd_block(x1[i], x2[j], ls, os_)
            if (i, j) == (1, 2):
                want[1:, 1:] = torch.diag_embed((5.0 / 3.0) * os_ ** 2 / ls.expand(1, D)[0] ** 2)
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), (i, j)
    Ks = covariance.matern52_grad(x1, x1, ls, os_)
    assert torch.equal(Ks, Ks.mT)
    assert torch.linalg.eigvalsh(Ks + 1e-6 * torch.eye(M * T, dtype=torch.float64)).min() > 0
    diag = torch.cat((torch.ones(1, dtype=torch.float64), (5.0 / 3.0) / ls.expand(1, D)[0] ** 2)) * os_ ** 2
    assert torch.allclose(Ks.diagonal(), diag.repeat(M), rtol=1e-14)


def op(D=3, outputs=None, func=covariance.matern52_grad, dtype=torch.float32, **extra):
    x = torch.rand(6, D).to(dtype)
    return KernelLinearOperator(x, x, func, num_outputs_per_input=outputs or (D + 1, D + 1), num_nonbatch_dimensions=NB,
                                lengthscale=torch.ones(1, D, dtype=dtype), outputscale=torch.tensor(1.0, dtype=dtype), **extra)


def test_gate():
    assert covariance.matern52_grad.native_outputs == "mgrad" and not hasattr(covariance.matern52_grad, "native_family")
    assert covariance.MGRAD_FAMILIES == {"matern52_grad": covariance.matern52_grad}
    assert _hip.LO_OP_KERNEL_MGRAD_DIAG == 20 and _hip.ABI_VERSION >= 41
    for D in (1, 3, _hip.LO_KERNEL_GRAD_MAX_DIM):
        S = op(D)
        assert S._native_mgrad_refusal(check_device=False) is None
        assert S._native_variant(check_device=False).tag == "mgrad" and S._native_variant() is None
        assert S._native_mgrad_refusal() == "not on the device"
        # the other gates answer what they answer for any function without their attributes
        assert S._native_refusal(check_device=False) == "covar_func has no native_family"
        assert S._native_grad_refusal(check_device=False) == "covar_func has no native_outputs == 'grad'"
        want = torch.cat((torch.ones(1), torch.full((D,), 5.0 / 3.0))).repeat(6)
        assert torch.allclose(S._diagonal(), want) and torch.allclose(S._diagonal(), S.to_dense().diagonal())
    assert op(17)._native_mgrad_refusal(check_device=False) == "D = 17 beyond LO_KERNEL_GRAD_MAX_DIM"
    assert op(3, outputs=(1, 1))._native_mgrad_refusal(check_device=False) == "num_outputs_per_input is not (4, 4)"
    assert (op(3, alpha=torch.ones(1, 1))._native_mgrad_refusal(check_device=False)
            == "parameters other than lengthscale and outputscale")
    assert op(3, dtype=torch.float64)._native_mgrad_refusal(check_device=False) == "not float32"
    sub = op(3)[4:12, 0:8]  # slices of whole points rebuild the operator, as for rbf_grad
    assert isinstance(sub, KernelLinearOperator) and sub.shape == (8, 8) and sub.x1.shape == (2, 3)
