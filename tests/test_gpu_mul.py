"""MulLinearOperator / ConstantMulLinearOperator on the MI355X: the LO_OP_HADAMARD_DIAG kind and
lo_hadamard_bilinear_f32 (csrc/lo_hadamard.hip) against fp64 numpy, the torch compositions and the reference's goldens
(tests/golden/g30_mul_*.npz)."""
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_golden_mul import mul_inputs  # noqa: E402
from make_golden_ski import column, interp  # noqa: E402

from linear_operator_amd import kernels as K  # noqa: E402
from linear_operator_amd import settings  # noqa: E402
from linear_operator_amd.functions import pivoted_cholesky  # noqa: E402
from linear_operator_amd.operators import (  # noqa: E402
    AddedDiagLinearOperator, DiagLinearOperator, InterpolatedLinearOperator, MulLinearOperator, RootLinearOperator,
    ToeplitzLinearOperator)

pytestmark = pytest.mark.gpu
X = mul_inputs()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    return t.detach().cpu().numpy()


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def close(a, b, rel=1e-4):
    a, b = (host(a) if torch.is_tensor(a) else np.asarray(a)), np.asarray(b)
    return a.shape == b.shape and np.abs(a - b).max() <= rel * max(np.abs(b).max(), 1e-30)


def hadamard64(F, G, d, v):
    """(F F^T o G G^T) v + d o v in fp64: sum_r f_r o (G (G^T (f_r o v)))."""
    F, G, d, v = (a.astype(np.float64) for a in (F, G, d, v))
    y = d[..., None] * v
    for r in range(F.shape[-1]):
        w = F[..., r:r + 1] * v
        y += F[..., r:r + 1] * (G @ (G.swapaxes(-1, -2) @ w))
    return y


def inputs(seed, B, N, p, q, t):
    r = np.random.default_rng(seed)
    F = (r.standard_normal((B, N, p)) / np.sqrt(p)).astype(np.float32)
    G = (r.standard_normal((B, N, q)) / np.sqrt(q)).astype(np.float32)
    d = (0.5 + r.random((B, N))).astype(np.float32)
    v = r.standard_normal((B, N, t)).astype(np.float32)
    return F, G, d, v


@pytest.mark.parametrize("p,q", [(1, 1), (7, 5), (32, 32), (33, 97), (100, 60), (128, 128)])
@pytest.mark.parametrize("t", [1, 17, 33])
@pytest.mark.parametrize("B", [1, 8])
def test_native_matvec_against_fp64(p, q, t, B):
    N = 1013  # (no multiple of any tile: 32-row stages, 64-row workgroups)
    F, G, d, v = inputs(3900 + p + 7 * q + t + B, B, N, p, q, t)
    desc = K.hadamard_diag_descriptor(dev(F), dev(G), dev(d))
    assert desc.kind == K._hip.LO_OP_HADAMARD_DIAG
    y = host(K.matvec(desc, dev(v)))
    ref = hadamard64(F, G, d, v)
    err = np.abs(y - ref).max() / np.abs(ref).max()
    assert err < 2e-6, err
    assert np.array_equal(y, host(K.matvec(desc, dev(v))))  # bitwise the same from call to call


def test_constant_diag_and_operator_matmul():
    F, G, d, v = inputs(3990, 2, 517, 9, 11, 5)
    D = DiagLinearOperator(dev(d))
    A = AddedDiagLinearOperator(MulLinearOperator(RootLinearOperator(dev(F)), RootLinearOperator(dev(G))), D)
    assert A._kernel_descriptor().kind == K._hip.LO_OP_HADAMARD_DIAG
    assert close(A._matmul(dev(v)), hadamard64(F, G, d, v), rel=2e-6)
    sig = np.full((2, 1), 0.3, np.float32)
    desc = K.hadamard_diag_descriptor(dev(F), dev(G), dev(sig[:, 0]), const_diag=True)
    assert close(K.matvec(desc, dev(v)), hadamard64(F, G, np.broadcast_to(sig, d.shape), v), rel=2e-6)


def test_rank_above_cap_falls_back():
    F, G, d, v = inputs(3991, 2, 300, 129, 20, 3)
    A = MulLinearOperator(RootLinearOperator(dev(F)), RootLinearOperator(dev(G)))
    assert A._kernel_descriptor() is None
    assert close(A._matmul(dev(v)), hadamard64(F, G, np.zeros_like(d), v), rel=1e-5)


@pytest.mark.parametrize("p,q", [(1, 1), (7, 5), (32, 32), (100, 60)])
def test_goldens_forward_and_native_path(p, q):
    k = f"mv{p}x{q}"
    A = MulLinearOperator(RootLinearOperator(dev(X[k + "_F"])), RootLinearOperator(dev(X[k + "_G"])))
    with mock.patch.object(MulLinearOperator, "_matmul_composition", side_effect=AssertionError("torch path ran")):
        for t in (1, 17):
            assert close(A._matmul(dev(X[f"{k}_rhs{t}"])), golden("g30_mul_matvec")[f"{k}_y{t}"], rel=1e-5)


def test_pivoted_cholesky_pivots():
    g = golden("g30_mul_pivchol")
    A = MulLinearOperator(RootLinearOperator(dev(X["pc_F"])), RootLinearOperator(dev(X["pc_G"])))
    assert A._kernel_descriptor() is not None
    with mock.patch.object(K, "pivoted_cholesky_generic", side_effect=AssertionError("generic path ran")):
        L, piv = pivoted_cholesky(A, 12, error_tol=1e-8, return_pivots=True)
        L2, piv2 = pivoted_cholesky(A, 12, error_tol=1e-8, return_pivots=True)
    assert np.array_equal(host(piv), g["pc_piv"])
    assert close(L, g["pc_L"], rel=1e-4)
    assert np.array_equal(host(piv2), host(piv)) and np.array_equal(host(L2), host(L))


@pytest.mark.parametrize("B,N,p,q,S", [(2, 1013, 7, 5, 3), (1, 700, 100, 60, 4), (3, 333, 128, 33, 1)])
def test_native_bilinear_against_composition(B, N, p, q, S):
    F, G, _, U = inputs(3995 + p, B, N, p, q, S)
    V = np.random.default_rng(3996 + q).standard_normal((B, N, S)).astype(np.float32)
    Ft, Gt = dev(F).requires_grad_(True), dev(G).requires_grad_(True)
    A = MulLinearOperator(RootLinearOperator(Ft), RootLinearOperator(Gt))
    dF, dG = A._bilinear_derivative(dev(U), dev(V))
    cF, cG = A._bilinear_derivative_composition(dev(U), dev(V))
    assert close(dF, host(cF), rel=1e-4) and close(dG, host(cG), rel=1e-4)
    # fp64: d/dF of sum_s u_s^T (F F^T o G G^T) v_s by autograd
    F64, G64 = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (F, G))
    Kd = (F64 @ F64.mT) * (G64 @ G64.mT)
    (torch.from_numpy(U.astype(np.float64)) * (Kd @ torch.from_numpy(V.astype(np.float64)))).sum().backward()
    assert close(dF, F64.grad.numpy(), rel=1e-5) and close(dG, G64.grad.numpy(), rel=1e-5)
    dF2, _ = K.bilinear_hadamard(dev(F), dev(G), dev(U), dev(V))
    assert np.array_equal(host(dF2), host(dF))


def _scaled_mul(F, G, c, d, cls=AddedDiagLinearOperator):
    return cls(MulLinearOperator(RootLinearOperator(F), RootLinearOperator(G)).mul(c), DiagLinearOperator(d))


def test_solves_and_gradients_against_golden():
    g = golden("g30_mul_solve")
    Z = dev(X["so_Z"])

    class Probed(AddedDiagLinearOperator):
        def _probe_vectors_and_norms(self):
            n = Z.norm(dim=-2, keepdim=True)
            return Z / n, n

    F, G, c, d, rhs = (dev(X["so_" + k]) for k in ("F", "G", "c", "d", "rhs"))

    def boom(*a, **k):
        raise AssertionError("the closure path ran instead of the Hadamard kind")

    with mock.patch.object(K, "_wrap_closure", side_effect=boom), \
            mock.patch.object(K, "pivoted_cholesky_generic", side_effect=boom), \
            settings.cg_tolerance(1e-5), settings.max_cg_iterations(400), settings.num_trace_samples(6):
        A = _scaled_mul(F, G, c, d)
        assert A._kernel_descriptor().kind == K._hip.LO_OP_HADAMARD_DIAG
        K._hip.prof_enable(True)
        x = A.solve(rhs)
        torch.cuda.synchronize()
        prof = K._hip.prof_report()
        K._hip.prof_enable(False)
        assert "k_hd_expand" in prof and "k_hd_contract" in prof, prof.keys()
        assert np.allclose(host(x), g["so_solve"], rtol=1e-3, atol=1e-3 * np.abs(g["so_solve"]).max())
        Fg, Gg, cg, dg = (t.clone().requires_grad_(True) for t in (F, G, c, d))
        A = _scaled_mul(Fg, Gg, cg, dg, cls=Probed)
        iq, ld = A.inv_quad_logdet(rhs, logdet=True)
        assert np.allclose(host(iq), g["so_iq"], rtol=1e-4, atol=0)
        assert np.allclose(host(ld), g["so_ld"], rtol=1e-4, atol=2048 * 1.2e-7 * 10.0)
        (iq.sum() + ld.sum()).backward()
    assert close(Fg.grad, g["so_dF"], rel=2e-3) and close(Gg.grad, g["so_dG"], rel=2e-3)
    assert close(cg.grad, g["so_dc"], rel=2e-3) and close(dg.grad, g["so_dd"], rel=2e-3)


def _ski_batch(seed, B, N, M, J):
    col = dev(column(seed, B, M, ls=0.15))
    li, lv = interp(seed + 1, B, N, M, J)
    return InterpolatedLinearOperator(ToeplitzLinearOperator(col), dev(li), dev(lv), dev(li), dev(lv))


def test_skip_prod_matches_elementwise_product():
    """SKIP: prod over d = 3 one-dimensional KISS operators equals the elementwise product of their dense matrices."""
    A = _ski_batch(3980, 3, 60, 40, 4)
    P = A.prod(-3)
    assert isinstance(P, MulLinearOperator) and P._kernel_descriptor() is not None
    want = A.to_dense().prod(0)
    assert close(P.to_dense(), host(want), rel=1e-3)
    v = torch.randn(60, 4, device="cuda")
    assert close(P._matmul(v), host(want @ v), rel=1e-3)


def test_scale_kernel_shaped_solve_and_constant_gradient():
    """AddedDiag(Interpolated(...).mul(c), Diag): GPyTorch's ScaleKernel over a KISS-GP kernel solves natively and
    hands a gradient to the scale."""
    A = _ski_batch(3985, 2, 300, 64, 4)
    d = torch.full((2, 300), 0.2, device="cuda")
    rhs = torch.randn(2, 300, 2, device="cuda")
    c = torch.tensor(1.7, device="cuda", requires_grad=True)
    op = AddedDiagLinearOperator(A.mul(c), DiagLinearOperator(d))
    assert op._kernel_descriptor().kind == K._hip.LO_OP_SKI_DIAG
    with mock.patch.object(K, "_wrap_closure", side_effect=AssertionError("closure path ran")), \
            settings.cg_tolerance(1e-6), settings.max_cg_iterations(600):
        x = op.solve(rhs)
        (x * rhs).sum().backward()
    Kd = A.to_dense().double()
    c64 = torch.tensor(1.7, dtype=torch.float64, requires_grad=True)
    x64 = torch.linalg.solve(c64 * Kd + torch.diag_embed(d.double()), rhs.double())
    (x64 * rhs.double()).sum().backward()
    assert np.allclose(host(x), host(x64), rtol=1e-3, atol=1e-3 * host(x64).__abs__().max())
    assert c.grad is not None and abs(c.grad.item() - c64.grad.item()) <= 2e-3 * abs(c64.grad.item())
